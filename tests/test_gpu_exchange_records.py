"""GPU: k_epoch_import and k_epoch_export on hand-built record arrays, against tests/exchange_ref.py.

A fresh handle on the dyadic box imports an array and exports before any clean: the exported cell records, sorted by key, must be
exchange_ref.import_records of the same array -- every cell once, its latch the minimum of the valid ids offered.  The arrays sit on
the import kernel's seams: 256 records a tile, kImportTiles = 8 tiles a workgroup (2048 records), one occ_list reservation a
workgroup; the same key twice in one wave, 64 times in one wave, in two workgroups; 64 new bricks in one wave; frame records between
cell records.  Then the export's bookkeeping (it advances at the clean, not at the export), the records a transport may hand in that
the import must ignore, the capacity errors an import can cause, and the refusal of hfpf_epoch_import_gathered."""
import numpy as np
import pytest

import crafted as X
import exchange_ref as E
from gpu_support import SMALL_CAPS

pytestmark = pytest.mark.gpu

DIMS = X.DIMS
MAX_FRAMES = SMALL_CAPS["max_frames"]
TILE, GROUP = 256, 2048   # records a tile and a workgroup of k_epoch_import (kernels.hpp: 256 threads, kImportTiles = HFPF_REG_TILES = 8)
BOUNDARY_COUNTS = (1, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097)


def _fresh(hfpf_mod, **caps):
    g = hfpf_mod.OccupancyGrid(resolution=X.RES, bbox=X.BBOX, **dict(SMALL_CAPS, **caps))
    assert g.dims[0] == DIMS
    return g


def _import(g, rec):
    rec = np.ascontiguousarray(rec)
    dev = g.device_alloc(max(rec.nbytes, 16))
    try:
        g.device_upload(dev, rec)
        g.epoch_import(dev, len(rec))
    finally:
        g.device_free(dev)


def _export(g):
    ptr, n = g.epoch_export()
    return g.device_download(ptr, n * 16).view(E.REC_DTYPE).copy() if n else np.zeros(0, E.REC_DTYPE)


def _by_key(rec):
    return rec[np.argsort(rec["key"], kind="stable")]


def _distinct_cells(n, seed, inclusive=True):
    """n distinct cells of the storage extent (0..dim an axis) or of the box proper (0..dim-1)."""
    ext = [d + 1 if inclusive else d for d in DIMS]
    lin = np.random.default_rng(seed).choice(ext[0] * ext[1] * ext[2], n, replace=False)
    return np.stack([lin // (ext[1] * ext[2]), (lin // ext[2]) % ext[1], lin % ext[2]], axis=1)


def _round_trip(hfpf_mod, rec, what):
    """import -> export on a fresh handle against the model; returns the model state."""
    ref = E.State()
    new = E.import_records(ref, rec, DIMS, MAX_FRAMES)
    with _fresh(hfpf_mod) as g:
        _import(g, rec)
        out = _export(g)
        occ = g.occupied().copy()
        n_occ = g.counters()["voxels_occupied"]
    assert not E.is_frame(out).any(), "%s: the handle has integrated no frame and exports frame records" % what
    want = ref.cell_records(DIMS)
    assert len(out) == len(want) == len(new), "%s: %d records exported, the model holds %d cells" % (what, len(out), len(want))
    assert _by_key(out).tobytes() == want.tobytes(), "%s: exported cell records differ from the model's" % what
    assert n_occ == len(new) and sorted(map(tuple, occ.tolist())) == sorted(ref.occupied), "%s: occupied list" % what
    return ref


@pytest.mark.parametrize("n", BOUNDARY_COUNTS)
def test_import_distinct_cells_at_tile_and_workgroup_boundaries(hfpf_mod, n):
    """n records of n distinct cells (some on the faces x = dim, y = dim, z = dim of the storage extent): the last tile partly filled,
    exactly filled, one record into the next tile or the next workgroup, whose other tiles are empty."""
    cells = _distinct_cells(n, 0xE100 + n)
    rec = E.cell_records(DIMS, cells, np.random.default_rng(n).integers(0, MAX_FRAMES, n))
    _round_trip(hfpf_mod, rec, "%d distinct cells" % n)


@pytest.mark.parametrize("n", [1, 2046, 2047, 4094])
def test_import_with_frame_records_behind_the_cells(hfpf_mod, n):
    """The shape of a real export: n cell records and two frame records, n + 2 on the boundaries 2048, 2049 and 4096 (and 3, the
    smallest an exporter with a cell can send)."""
    rec = E.export_records(_distinct_cells(n, 0xE200 + n), 7, [7], [[0.5, -1.0, 2.0]], DIMS)
    assert len(rec) == n + 2
    _round_trip(hfpf_mod, rec, "%d cells and a frame" % n)


@pytest.mark.parametrize("layout", ["adjacent", "2048_apart"])
def test_every_key_twice_with_different_latches(hfpf_mod, layout):
    """2048 cells, each offered twice: next to each other (two lanes of one wave race on the occ_mask word and both must reach the
    latch) or 2048 records apart (the same slot in two workgroups).  The smaller id comes first for half of them."""
    n = GROUP
    cells = _distinct_cells(n, 0xE300)
    rng = np.random.default_rng(0xE301)
    lo = rng.integers(0, MAX_FRAMES - 1, n)
    hi = lo + 1 + rng.integers(0, MAX_FRAMES - 1 - lo)
    swap = rng.integers(0, 2, n).astype(bool)
    a = E.cell_records(DIMS, cells, np.where(swap, hi, lo))
    b = E.cell_records(DIMS, cells, np.where(swap, lo, hi))
    if layout == "adjacent":
        rec = np.stack([a, b], axis=1).reshape(-1)
    else:
        rec = np.concatenate([a, b])
        assert (rec["key"][:n] == rec["key"][n:]).all()
    ref = _round_trip(hfpf_mod, rec, "every key twice, %s" % layout)
    assert len(ref.occupied) == n and sorted(ref.latch[tuple(c)] for c in cells.tolist()) == sorted(lo.tolist())


def test_one_key_64_times_in_one_wave(hfpf_mod):
    """Records 64..127 (the second wave of the first tile) all name one cell, with 64 different latches, the smallest in the middle;
    the waves around it hold distinct cells."""
    cells = _distinct_cells(193, 0xE400)
    rec = E.cell_records(DIMS, cells[:192], 9)
    rec[64:128] = E.cell_records(DIMS, np.repeat(cells[192:], 64, axis=0), 1000 + (np.arange(64) * 37 + 11) % 64)
    ref = _round_trip(hfpf_mod, rec, "one key 64 times")
    assert len(ref.occupied) == 129 and ref.latch[tuple(cells[192])] == 1000


def test_one_wave_over_64_new_bricks(hfpf_mod):
    """Every lane of a wave claims a brick of its own (brick_acquire_wave with 64 leaders), three waves of it, and a fourth whose
    lanes share 16 of those bricks."""
    nb = [(d + 1 + 7) // 8 for d in DIMS]
    bricks = np.stack(np.meshgrid(*[np.arange(k - 1) for k in nb], indexing="ij"), -1).reshape(-1, 3)   # whole bricks only
    rng = np.random.default_rng(0xE500)
    bricks = bricks[rng.permutation(len(bricks))[:192]]
    again = bricks[rng.integers(0, 16, 64)] * 8 + rng.integers(0, 8, (64, 3))
    rec = E.cell_records(DIMS, np.vstack([bricks * 8 + rng.integers(0, 8, bricks.shape), again]), 3)
    ref = E.State()
    E.import_records(ref, rec, DIMS, MAX_FRAMES)
    with _fresh(hfpf_mod) as g:
        _import(g, rec)
        out = _export(g)
        assert g.counters()["bricks_allocated"] == 192
    assert _by_key(out).tobytes() == ref.cell_records(DIMS).tobytes()


def test_frame_records_interleaved_between_cell_records(hfpf_mod):
    """The exporter never sends this, the ABI allows it: every third record is a frame half (lanes of a wave that want no brick
    between lanes that do).  The frames' viewpoints are read back through a clean: a sheet of cells whose latch names a frame
    above them gets normals that look up, one that names a frame below them normals that look down."""
    sheet = X.sheet((40,))
    below, above = X.pose_of(False)[:, 3], X.pose_of(True)[:, 3]
    up = sheet[:, 0] % 2 == 0
    cells = E.cell_records(DIMS, sheet, np.where(up, 21, 20))
    frames = E.frame_records([20, 21, 22, 23], [below, above, [np.nan] * 3, [0, 0, 0]])
    rec = np.zeros(len(cells) + len(cells) // 2, E.REC_DTYPE)
    is_fr = np.arange(len(rec)) % 3 == 2
    rec[~is_fr] = cells
    rec[is_fr] = np.resize(frames, int(is_fr.sum()))
    _round_trip(hfpf_mod, rec, "interleaved frame records")
    with _fresh(hfpf_mod) as g:
        _import(g, rec)
        g.clean()
        rows = g.extract().copy()
    assert len(rows) >= 400, "%d rows: the 20 x 20 interior cells of the sheet have full stencils" % len(rows)
    assert ((rows["nz"] > 0) == (rows["ix"] % 2 == 0)).all(), "a normal does not look at the viewpoint its cell's latch names"


# ---- export bookkeeping -------------------------------------------------------------------------------------------------------------

def _integrate(g, frames, poses, ids):
    import shards
    shards.integrate(g, frames, poses, ids, len(frames[0]))


def test_export_repeats_until_the_clean_and_is_empty_behind_it(hfpf_mod):
    rec = E.cell_records(DIMS, _distinct_cells(3000, 0xE600, inclusive=False), 5)
    with _fresh(hfpf_mod) as g:
        assert len(_export(g)) == 0, "an empty handle exports records"
        _import(g, rec)
        first, second = _export(g), _export(g)
        assert len(first) == 3000 and _by_key(first).tobytes() == _by_key(second).tobytes(), "a second export without a clean differs"
        g.clean()
        assert len(_export(g)) == 0, "an export straight after a clean returns records"


def test_export_after_integrate_and_import(oracle_mod, hfpf_mod):
    """Two frames with the ids 5 and 2 (one call, the camera below and above) on overlapping halves of a sheet: exactly the oracle's
    cells, each with the smallest id that touched it, and two records a frame whose floats are the pose's translation as f32.  Then,
    before any clean, an import offers half of those cells and some new ones the ids 3 and 1: the next export holds all of them
    with the minimum, and the same frame records.  Behind the clean a further frame exports its own new cells and itself alone."""
    sh = X.sheet((40,))
    f5, p5 = X.points(sh[sh[:, 0] < 48], 0xE700)
    f2, p2 = X.points(sh[sh[:, 0] >= 40], 0xE701, flip=True)
    og = oracle_mod.OracleGrid(resolution=X.RES, bbox=X.BBOX)
    c5, v5 = X.cells_of(og, f5, p5)
    c2, v2 = X.cells_of(og, f2, p2)
    f9, p9 = X.points(X.sheet((60,)), 0xE702)
    c9, v9 = X.cells_of(og, f9, p9)
    og.close()
    assert v5.all() and v2.all() and v9.all()
    local = E.State()
    for c, fid in ((c5, 5), (c2, 2)):
        E.import_records(local, E.cell_records(DIMS, np.unique(c, axis=0), fid), DIMS, MAX_FRAMES)
    assert 0 < sum(1 for v in local.latch.values() if v == 5) < len(local.latch)
    vps = {fid: oracle_mod.probe_transform(p, np.zeros((1, 3), np.float32))[0] for fid, p in ((5, p5), (2, p2), (9, p9))}
    assert vps[5].tobytes() == p5[:, 3].astype(np.float32).tobytes()
    offered = np.concatenate([E.cell_records(DIMS, sh[::2], 3), E.cell_records(DIMS, X.sheet((50,)), 1)])
    with _fresh(hfpf_mod) as g:
        _integrate(g, [f5, f2], [p5, p2], [5, 2])
        out = _export(g)
        n = len(local.occupied)
        assert len(out) == n + 4 and not E.is_frame(out[:n]).any() and E.is_frame(out[n:]).all()
        assert _by_key(out[:n]).tobytes() == local.cell_records(DIMS).tobytes(), "the cells of a local integrate and their latches"
        want_frames = _by_key(E.frame_records([5, 2], [vps[5], vps[2]]))
        assert _by_key(out[n:]).tobytes() == want_frames.tobytes(), "frame records: %r" % (out[n:],)
        _import(g, offered)
        E.import_records(local, offered, DIMS, MAX_FRAMES)
        out = _export(g)
        n = len(local.occupied)
        assert len(out) == n + 4 and _by_key(out[:n]).tobytes() == local.cell_records(DIMS).tobytes(), "local and imported cells, latches min'd"
        assert _by_key(out[n:]).tobytes() == want_frames.tobytes()
        g.clean()
        assert len(_export(g)) == 0
        _integrate(g, [f9], [p9], [9])
        out = _export(g)
        new = np.unique(c9, axis=0)
        assert len(out) == len(new) + 2 and _by_key(out[:len(new)]).tobytes() == _by_key(E.cell_records(DIMS, new, 9)).tobytes()
        assert out[len(new):].tobytes() == E.frame_records([9], [vps[9]]).tobytes()


# ---- records a transport may hand in ------------------------------------------------------------------------------------------------

def _valid_array():
    """Two sheets whose latches name frame 1 (below) and frame 2 (above) by the parity of x, and those frames."""
    sh = X.sheet((40, 43))
    cells = E.cell_records(DIMS, sh, np.where(sh[:, 0] % 2 == 0, 2, 1))
    return sh, np.concatenate([cells, E.frame_records([1, 2], [X.pose_of(False)[:, 3], X.pose_of(True)[:, 3]])])


def _invalid_records(sh):
    sy, sx, _ = E.key_shifts(DIMS)
    nan = np.array([np.nan], np.float32).view(np.uint32)[0]
    bad = np.zeros(12, E.REC_DTYPE)
    # a coordinate at dim + 1 or beyond it on every axis; an x field with bit 31 set and one that is 2^32 + a valid x
    bad["key"][:7] = [(DIMS[0] + 1) << sx | (3 << sy) | 4, 127 << sx, (3 << sx) | ((DIMS[1] + 1) << sy), (3 << sx) | (127 << sy) | 5,
                      (3 << sx) | (2 << sy) | (DIMS[2] + 1), ((1 << 31) | 40) << sx | (30 << sy) | 41, ((1 << 32) | 40) << sx | (30 << sy) | 41]
    bad["first_frame"][:7] = 0
    # latches a valid cell must not take
    bad["key"][7:9] = E.make_key(DIMS, sh[[10, 11]])
    bad["first_frame"][7:9] = [MAX_FRAMES, 0xFFFFFFFF]
    # frame records with ids at and beyond max_frames (the low 32 bits are the id), NaN floats
    bad["key"][9:] = [(1 << 63) | MAX_FRAMES, (1 << 63) | (1 << 62) | MAX_FRAMES, (1 << 63) | 0xFFFFFFFF]
    bad["first_frame"][9:], bad["pad"][9:] = nan, nan
    return bad


def test_invalid_records_are_ignored_and_the_handle_goes_on(hfpf_mod):
    sh, valid = _valid_array()
    bad = _invalid_records(sh)
    mixed = np.concatenate([valid, bad])
    mixed = mixed[np.random.default_rng(0xE800).permutation(len(mixed))]
    ref = E.State()
    E.import_records(ref, valid, DIMS, MAX_FRAMES)
    _round_trip(hfpf_mod, mixed, "invalid records mixed in")
    # a cell at a coordinate EQUAL to dim is inside the storage extent (include/hfpf.h)
    edge = E.cell_records(DIMS, [[DIMS[0], 3, 4], [3, DIMS[1], 4], [3, 4, DIMS[2]], list(DIMS)], 0)
    assert len(_round_trip(hfpf_mod, edge, "cells at dim").occupied) == 4
    f, p = X.points(X.sheet((46,)), 0xE801)
    results = []
    for rec in (valid, mixed):
        with _fresh(hfpf_mod) as g:
            _import(g, rec)
            out = _export(g)
            assert _by_key(out).tobytes() == ref.cell_records(DIMS).tobytes()
            g.clean()
            rows = g.extract().copy()
            _integrate(g, [f], [p], [3])
            g.clean()
            results.append((rows, g.extract().copy(), g.occupied().copy()))
    (r0, r1, occ), (m0, m1, mocc) = results
    assert len(r0) >= 800 and((r0["nz"] > 0) == (r0["ix"] % 2 == 0)).all(), "the valid array alone: %d rows" % len(r0)
    assert m0.tobytes() == r0.tobytes(), "rows behind the clean differ from the run without the invalid records"
    assert len(m1) > len(m0) and m1.tobytes() == r1.tobytes() and np.array_equal(mocc, occ), "the handle did not go on as the other"


def _poisoned_until_clear(hfpf_mod, g, which):
    with pytest.raises(hfpf_mod.HfpfError) as e:
        g.clean()
    assert e.value.code == -3 and which in str(e.value), str(e.value)
    f, p = X.points(X.sheet((46,)), 0xE901)
    for call in (lambda: g.integrate(f, p), g.clean, g.extract):
        with pytest.raises(hfpf_mod.HfpfError) as e2:
            call()
        assert e2.value.code == -5 and "hfpf_clear" in str(e2.value)
    g.clear()
    assert len(g.extract()) == 0 and len(g.occupied()) == 0


def test_import_beyond_the_occupied_list_is_a_capacity_error_at_the_clean(hfpf_mod):
    """max_normals = 256 gives an occupied list of 1024 entries; 1100 cells are imported (k_epoch_import keeps every occ_list write
    below max_occ and raises the error bit; the bricks and their masks have room).  The import returns OK, the clean fails with the
    capacity code, the handle is poisoned until hfpf_clear, and a roomy handle beside it is unaffected."""
    sh = X.sheet((40, 43))[:1100]
    rec = np.concatenate([E.cell_records(DIMS, sh, 1), E.frame_records([1], [X.pose_of(False)[:, 3]])])
    with _fresh(hfpf_mod, max_normals=256) as g, _fresh(hfpf_mod) as roomy:
        _import(g, rec)
        _import(roomy, rec)
        _poisoned_until_clear(hfpf_mod, g, "occupied list")
        roomy.clean()
        assert len(roomy.extract()) > 600 and len(roomy.occupied()) == 1100
        _import(g, rec[:1000])   # and after the clear the handle takes what fits
        assert len(g.occupied()) == 1000


def test_import_beyond_the_brick_pool_is_a_capacity_error_at_the_clean(hfpf_mod):
    """max_bricks = 8 and an import of 12 cells in 12 bricks, in one wave: a claim beyond the pool gives its directory entry back and
    returns no brick, the lanes write nothing, the error bit is raised."""
    bricks = np.array([[bx, by, 5] for bx in range(2, 6) for by in range(2, 5)])
    rec = E.cell_records(DIMS, bricks * 8 + 3, 1)
    with _fresh(hfpf_mod, max_bricks=8) as g, _fresh(hfpf_mod) as roomy:
        _import(g, rec)
        _import(roomy, rec)
        _poisoned_until_clear(hfpf_mod, g, "brick pool")
        roomy.clean()
        assert len(roomy.occupied()) == 12
        _import(g, rec[:8])
        assert len(g.occupied()) == 8


def test_gathered_import_refuses_a_count_beyond_the_stride(hfpf_mod):
    """World 3, importing rank 0: rank 1's count fits, rank 2's does not.  HFPF_ERR_BAD_ARG, and rank 1's slice is not imported
    either; the handle stays usable and takes the same buffer with honest counts."""
    stride = 64
    buf = E.cell_records(DIMS, _distinct_cells(3 * stride, 0xEA00), 0)
    with _fresh(hfpf_mod) as g:
        dev = g.device_alloc(buf.nbytes)
        try:
            g.device_upload(dev, buf)
            for counts in ([0, 10, stride + 1], [0, stride + 1, 10], [0, 10, 1 << 61]):
                with pytest.raises(hfpf_mod.HfpfError) as e:
                    g.epoch_import_gathered(dev, stride * 16, 3, 0, np.array(counts, np.uint64))
                assert e.value.code == -2, "HFPF_ERR_BAD_ARG"
                assert len(g.occupied()) == 0 and len(_export(g)) == 0, "a refused call imported records (counts %r)" % (counts,)
            g.epoch_import_gathered(dev, stride * 16, 3, 0, np.array([1 << 61, 10, stride], np.uint64))   # its own count is not looked at
            got = _by_key(_export(g))
        finally:
            g.device_free(dev)
    assert got.tobytes() == _by_key(np.concatenate([buf[stride:stride + 10], buf[2 * stride:]])).tobytes()
