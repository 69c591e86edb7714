"""CPU: the numpy restatement of the epoch exchange (tests/exchange_ref.py) against its own contract -- the record layout of
include/hfpf.h, round trip, idempotence, order and launch independence, duplicates inside one array, the invalid-record rules."""
import numpy as np
import pytest

import exchange_ref as E

DIMS = (107, 75, 90)   # lattice.DIMS: 7 bits an axis
MAX_FRAMES = 4096


def _cells(n, seed=1):
    rng = np.random.default_rng(seed)
    lin = rng.choice((DIMS[0] + 1) * (DIMS[1] + 1) * (DIMS[2] + 1), n, replace=False)
    return np.stack([lin // ((DIMS[1] + 1) * (DIMS[2] + 1)), (lin // (DIMS[2] + 1)) % (DIMS[1] + 1), lin % (DIMS[2] + 1)], axis=1)


def _export(n=300, frames=(7, 3, 11), seed=1):
    rng = np.random.default_rng(seed + 100)
    cells = _cells(n, seed)
    ff = rng.choice(np.asarray(frames), n).astype(np.uint32)
    vps = rng.normal(size=(len(frames), 3)).astype(np.float32)
    return cells, ff, np.asarray(frames), vps, E.export_records(cells, ff, frames, vps, DIMS)


def test_record_layout():
    assert E.key_shifts(DIMS) == (7, 14, 21) and E.key_shifts((128, 127, 1)) == (1, 8, 16)
    rec = E.export_records([[3, 2, 1], [107, 75, 90]], [5, 9], [6], [[1.5, -2.0, 0.25]], DIMS)
    assert rec.dtype == E.REC_DTYPE and len(rec) == 4
    assert rec["key"].tolist() == [(3 << 14) | (2 << 7) | 1, (107 << 14) | (75 << 7) | 90, (1 << 63) | 6, (1 << 63) | (1 << 62) | 6]
    assert rec["first_frame"][:2].tolist() == [5, 9] and rec["pad"][:2].tolist() == [0, 0]
    raw = rec.tobytes()
    assert np.frombuffer(raw[40:48], "<f4").tolist() == [1.5, -2.0] and np.frombuffer(raw[56:64], "<f4").tolist() == [0.25, 0.0]
    assert np.frombuffer(raw[0:8], "<u8")[0] == rec["key"][0] and np.frombuffer(raw[8:12], "<u4")[0] == 5
    assert E.key_cells(DIMS, rec["key"][:2]).tolist() == [[3, 2, 1], [107, 75, 90]]
    assert E.is_frame(rec).tolist() == [False, False, True, True]


def test_round_trip():
    cells, ff, frames, vps, rec = _export()
    s = E.State()
    new = E.import_records(s, rec, DIMS, MAX_FRAMES)
    assert new == [tuple(c) for c in cells.tolist()]
    assert s.latch == {tuple(c): int(f) for c, f in zip(cells.tolist(), ff)}
    assert sorted(s.viewpoint) == sorted(frames.tolist())
    for f, vp in zip(frames.tolist(), vps):
        assert s.viewpoint[f].tobytes() == vp.tobytes()
    back = s.cell_records(DIMS)
    want = rec[:len(cells)]
    assert back.tobytes() == want[np.argsort(want["key"])].tobytes()


def test_importing_twice_adds_nothing():
    rec = _export()[4]
    s = E.State()
    E.import_records(s, rec, DIMS, MAX_FRAMES)
    once = s.copy()
    assert E.import_records(s, rec, DIMS, MAX_FRAMES) == [] and s.same(once)


@pytest.mark.parametrize("seed", range(4))
def test_any_order_and_any_split_gives_the_same_state(seed):
    """Two exporters that share half their cells with different latches, every frame's viewpoint the same from both."""
    cells, ff, frames, vps, a = _export(seed=seed)
    b = a.copy()
    b["first_frame"][:150] = (ff[:150] + 1) % 13
    b = b[150:]
    rec = np.concatenate([a, b])
    ref = E.State()
    E.import_records(ref, rec, DIMS, MAX_FRAMES)
    rng = np.random.default_rng(seed)
    for _ in range(5):
        s = E.State()
        cuts = np.sort(rng.integers(0, len(rec) + 1, 3))
        new = []
        for part in np.split(rec[rng.permutation(len(rec))], cuts):
            new += E.import_records(s, part, DIMS, MAX_FRAMES)
        assert s.same(ref) and sorted(new) == sorted(ref.occupied) and len(new) == len(set(new))


def test_duplicates_inside_one_array():
    c = np.array([[5, 6, 7]])
    rec = np.concatenate([E.cell_records(DIMS, c, [9]), E.cell_records(DIMS, c, [4]), E.cell_records(DIMS, c, [E.NO_FRAME]), E.cell_records(DIMS, c, [6])])
    s = E.State()
    assert E.import_records(s, rec, DIMS, MAX_FRAMES) == [(5, 6, 7)]
    assert s.occupied == {(5, 6, 7)} and s.latch == {(5, 6, 7): 4}


def test_invalid_records_change_nothing():
    cells, ff, frames, vps, rec = _export(50)
    s = E.State()
    E.import_records(s, rec, DIMS, MAX_FRAMES)
    before = s.copy()
    sy, sx, bits = E.key_shifts(DIMS)
    bad = np.zeros(9, E.REC_DTYPE)
    bad["key"][:6] = [(108 << sx) | 1, (127 << sx), (3 << sx) | (76 << sy), (3 << sx) | (2 << sy) | 91, (1 << 31) << sx, ((1 << 32) + 3) << sx]
    bad["key"][6:] = [(1 << 63) | MAX_FRAMES, (1 << 63) | (1 << 62) | MAX_FRAMES, (1 << 63) | 0xFFFFFFFF]
    bad["first_frame"][6:] = np.array([np.nan], np.float32).view(np.uint32)[0]
    assert (bad["key"][:6] < (1 << 63)).all()
    assert E.import_records(s, bad, DIMS, MAX_FRAMES) == [] and s.same(before)
    # a latch at or above max_frames: the cell is kept (a new one without a latch), the latch left alone
    late = E.cell_records(DIMS, np.vstack([cells[:2], [[0, 0, 0]], [[107, 75, 90]]]), [MAX_FRAMES, E.NO_FRAME, MAX_FRAMES, 2])
    assert E.import_records(s, late, DIMS, MAX_FRAMES) == [(0, 0, 0), (107, 75, 90)]
    assert s.latch[tuple(cells[0])] == ff[0] and s.latch[tuple(cells[1])] == ff[1] and s.latch[(0, 0, 0)] == E.NO_FRAME and s.latch[(107, 75, 90)] == 2
    # the halves of a frame are written independently
    half = E.frame_records([3], [[1.0, 2.0, 3.0]])[1:]
    old = s.viewpoint[3].copy()
    E.import_records(s, half, DIMS, MAX_FRAMES)
    assert s.viewpoint[3].tolist() == [old[0], old[1], 3.0]
