"""GPU: a clean pass whose front half runs beside the update kernel of the integrate call before it (HFPF_CLEAN_OVERLAP, default on;
csrc/hfpf.hip clean_locked) computes what the plain sequence on one stream computes.  Every scene is run three ways -- knob on, knob
off, oracle: the engine's rows byte-identical on and off, fourteen columns byte-identical with the oracle's exact rows, the counters
a pass produces equal.  HFPF_TRACE_CLEAN=1 says on stderr which stream the front half of each pass took, so every test also knows
that the path it is about ran (and that it did not with the knob off).

A pass overlaps only behind a batch of at least four frames that had a bin plan and ran the update kernel: from the second batch of
a session on.  Batches of four 160x120 frames at 1 mm, SMALL capacities."""
import numpy as np
import pytest

import scenes
from gpu_support import SMALL_CAPS, contract_counters

pytestmark = pytest.mark.gpu

W, H, RES, FX = 160, 120, 0.001, 615.0
BATCH = 4
EQUAL_COUNTERS = ("voxels_with_normal", "registrations", "dep_entries", "replay_members")
BESIDE, ALONE = "beside the update kernel", "on the engine's stream"


def _scene(n_frames=12):
    """Random poses (30 degrees, 5 cm): every batch looks into space the batches before it left unoccupied but registered on, so
    the cells it occupies carry a pre-dependant that the next pass files -- what k_clean_begin was split for."""
    return scenes.Scene(n_frames, W, H, RES, fx=FX)


class Stream:
    """The scene's frames in HBM of one handle, handed over in batches with hfpf_integrate_device."""

    def __init__(self, g, sc):
        self.g, self.sc = g, sc
        self.stride = W * H * 16
        clouds = np.concatenate([np.ascontiguousarray(sc.frame(f)).view(np.uint8).reshape(-1) for f in range(sc.n_frames)])
        assert clouds.nbytes == self.stride * sc.n_frames
        self.dev = g.device_alloc(clouds.nbytes)
        g.device_upload(self.dev, clouds)

    def integrate(self, first, n):
        poses = np.stack([np.asarray(self.sc.poses[f], np.float64).reshape(12) for f in range(first, first + n)])
        self.g.integrate_device(self.dev + first * self.stride, n, self.stride, W * H, poses)

    def free(self):
        self.g.device_free(self.dev)


def _plan(sc, batch=BATCH, clean_after_batch=True):
    """[('integrate', first, n) | ('clean',)]: batches with a clean after each (or only at the end)."""
    ops = []
    for first in range(0, sc.n_frames, batch):
        ops.append(("integrate", first, min(batch, sc.n_frames - first)))
        if clean_after_batch:
            ops.append(("clean",))
    if not clean_after_batch:
        ops.append(("clean",))
    return ops


def _drive(g, st, ops):
    for op in ops:
        if op[0] == "integrate":
            st.integrate(op[1], op[2])
        elif op[0] == "clean":
            g.clean()
        elif op[0] == "counters":
            g.counters()
        elif op[0] == "sync":
            g.sync()
        elif op[0] == "clear":
            g.clear()
        else:
            raise AssertionError(op)


def _passes(capfd):
    """(overlapped, plain) clean passes since the last call, from the HFPF_TRACE_CLEAN lines."""
    err = capfd.readouterr().err
    lines = [ln for ln in err.splitlines() if ln.startswith("hfpf: clean pass")]
    return sum(BESIDE in ln for ln in lines), sum(ALONE in ln for ln in lines)


def _engine(hfpf_mod, monkeypatch, capfd, sc, ops, overlap, **kw):
    """One engine run of `ops` on a fresh handle with the knob set: (rows, counters, overlapped passes, plain passes)."""
    monkeypatch.setenv("HFPF_CLEAN_OVERLAP", "1" if overlap else "0")
    monkeypatch.setenv("HFPF_TRACE_CLEAN", "1")
    capfd.readouterr()
    with hfpf_mod.OccupancyGrid(resolution=sc.resolution, bbox=sc.bbox, **dict(SMALL_CAPS, **kw)) as g:
        st = Stream(g, sc)
        _drive(g, st, ops)
        rows = g.extract().copy()
        ctr = g.counters()
        st.free()
    n_beside, n_alone = _passes(capfd)
    return rows, ctr, n_beside, n_alone


_oracle_cache = {}


def _oracle(oracle_mod, sc, key, ops, color=False):
    """Exact rows of the oracle driven through the same schedule (frame by frame: a batch is the engine's affair), once per key."""
    if key not in _oracle_cache:
        og = oracle_mod.OracleGrid(resolution=sc.resolution, bbox=sc.bbox, exact_moments=True, **(dict(fuse_color=True) if color else {}))
        lay = sc.layout
        kw = dict(point_step=lay["point_step"], off_x=lay["off_x"], off_y=lay["off_y"], off_z=lay["off_z"])
        if color:
            kw["off_rgb"] = lay["off_rgb"]
        for op in ops:
            if op[0] == "integrate":
                for f in range(op[1], op[1] + op[2]):
                    og.capture(sc.frame(f), sc.poses[f], **kw)
            elif op[0] == "clean":
                og.clean()
        og.extract()
        exact = og.extract_exact()
        og.close()
        exact.setflags(write=False)
        _oracle_cache[key] = exact
    return _oracle_cache[key]


def _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, sc, ops, key, min_beside, oracle_ops=None, max_beside=None, **kw):
    on, c_on, beside, alone = _engine(hfpf_mod, monkeypatch, capfd, sc, ops, True, **kw)
    off, c_off, beside_off, alone_off = _engine(hfpf_mod, monkeypatch, capfd, sc, ops, False, **kw)
    print("clean passes: knob on %d beside the update kernel + %d alone, knob off %d + %d" % (beside, alone, beside_off, alone_off))
    assert beside_off == 0, "HFPF_CLEAN_OVERLAP=0 must keep every pass on the engine's stream"
    assert beside + alone == beside_off + alone_off
    assert beside >= min_beside, "the schedule was chosen so that %d passes overlap; %d did" % (min_beside, beside)
    assert max_beside is None or beside <= max_beside, "%d passes overlapped, at most %d can" % (beside, max_beside)
    assert on.tobytes() == off.tobytes(), "rows differ between HFPF_CLEAN_OVERLAP=1 and 0"
    for k in EQUAL_COUNTERS:
        assert c_on[k] == c_off[k], "counter %s: %d with the overlap, %d without" % (k, c_on[k], c_off[k])
    exact = _oracle(oracle_mod, sc, key, oracle_ops or ops, color=bool(kw.get("fuse_color")))
    rep = scenes.compare_rows_exact(exact, on)
    assert rep["exact_bytes_differing"] == 0
    return on, c_on


# ---- 1, 2: several batches, a clean after each (the filing of pre-dependants moves behind k_register) ---------------------------
@pytest.mark.parametrize("color", [False, True], ids=["plain", "colour"])
def test_batches_with_a_clean_after_each(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd, color):
    sc = _scene()
    rows, ctr = _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, sc, _plan(sc), ("batches", color), 2, max_beside=2, fuse_color=color)
    assert len(rows) > 10000 and ctr["dep_pairs_member"] > 0 and ctr["clean_passes"] == 3
    if color:
        assert len(np.unique(rows["rgb"])) > 1000


# ---- 3: the two ends of the clean cadence (neither overlaps: single frames publish nothing early, a first pass has no update) ----
def test_clean_after_every_frame(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd):
    sc = _scene(5)
    _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, sc, _plan(sc, batch=1), "every_frame", 0)


def test_clean_only_at_the_end(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd):
    sc = _scene(8)
    rows, ctr = _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, sc, _plan(sc, clean_after_batch=False), "at_end", 0)
    assert ctr["clean_passes"] == 1 and ctr["replay_members"] > 0


# ---- 4: host orderings ----------------------------------------------------------------------------------------------------
def _between(sc, what):
    """The plan with `what` put between every integrate call and its clean."""
    ops = []
    for op in _plan(sc):
        if op[0] == "clean":
            ops += what
        ops.append(op)
    return ops


@pytest.mark.parametrize("which", ["counters_then_clean", "sync_then_clean", "two_cleans", "clean_on_empty_grid", "no_sync_anywhere"])
def test_host_orderings(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd, which):
    """A read-back between the call and the pass (hfpf_get_counters, hfpf_sync) consumes the publishes: the pass runs alone.  A second
    pass in a row and a pass on an empty grid find no call pending.  All of them compute the rows of the plain plan."""
    sc = _scene()
    plain = _plan(sc)
    ops, min_beside, max_beside = {
        "counters_then_clean": (_between(sc, [("counters",)]), 0, 0),
        "sync_then_clean": (_between(sc, [("sync",)]), 0, 0),
        "two_cleans": (_between(sc, [("clean",)]), 2, 2),       # the first of each pair overlaps, the second finds no call pending
        "clean_on_empty_grid": ([("clean",)] + plain, 2, 2),
        "no_sync_anywhere": (plain, 2, 2),
    }[which]
    _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, sc, ops, ("batches", False), min_beside, oracle_ops=plain, max_beside=max_beside)


def test_clear_after_an_overlapped_clean(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd):
    """hfpf_clear right behind an overlapped pass (its back half still queued), then the whole scene on the same handle: the rows
    and counters of a fresh handle."""
    sc = _scene()
    plain = _plan(sc)
    fresh, c_fresh = _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, sc, plain, ("batches", False), 2)
    reused, c_reused, beside, alone = _engine(hfpf_mod, monkeypatch, capfd, sc, plain[:4] + [("clear",)] + plain, True)
    assert beside >= 3  # one before the clear, two after
    assert reused.tobytes() == fresh.tobytes()
    for k in EQUAL_COUNTERS + ("voxels_occupied", "dep_pairs_member", "points_buffered"):
        assert c_reused[k] == c_fresh[k], k


# ---- 5: snapshot right behind an overlapped clean ------------------------------------------------------------------------------
def test_snapshot_after_an_overlapped_clean(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd):
    sc = _scene()
    plain = _plan(sc)
    whole, c_whole = _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, sc, plain, ("batches", False), 2)
    monkeypatch.setenv("HFPF_CLEAN_OVERLAP", "1")
    monkeypatch.setenv("HFPF_TRACE_CLEAN", "1")
    capfd.readouterr()
    with hfpf_mod.OccupancyGrid(resolution=sc.resolution, bbox=sc.bbox, **SMALL_CAPS) as src:
        st = Stream(src, sc)
        _drive(src, st, plain[:4])  # two batches, two passes: the second one overlapped
        blob = src.snapshot()
        assert _passes(capfd) == (1, 1)
        with hfpf_mod.OccupancyGrid(resolution=sc.resolution, bbox=sc.bbox, **SMALL_CAPS) as dst:
            dst.restore(blob)
            assert contract_counters(src) == contract_counters(dst)
            st2 = Stream(dst, sc)
            _drive(dst, st2, plain[4:])
            rows = dst.extract().copy()
            c_dst = contract_counters(dst)
            st2.free()
        _drive(src, st, plain[4:])  # the source goes on as if nothing had happened
        assert src.extract().tobytes() == whole.tobytes()
        c_src = contract_counters(src)
        st.free()
    assert rows.tobytes() == whole.tobytes(), "the restored handle's continuation differs from the uninterrupted run"
    assert c_dst == c_src and all(c_src[k] == c_whole[k] for k in c_src)


# ---- 6: a pool that overflows around an overlapped pass --------------------------------------------------------------------------
def _until_error(hfpf_mod, g, st, ops):
    """Drives ops + a final sync until one raises: (index of the raising op, its HfpfError)."""
    for i, op in enumerate(ops + [("sync",)]):
        try:
            _drive(g, st, [op])
        except hfpf_mod.HfpfError as e:
            return i, e
    return None, None


@pytest.mark.parametrize("pool", ["max_normals", "max_log_points"])
def test_capacity_error_around_an_overlapped_pass(hfpf_mod, synth_mod, monkeypatch, capfd, pool):
    """The pool sized between what the first and the second batch + pass need.  max_normals: the second pass runs out of normal
    records (and, sized from them, of registrations and dependant entries) -- in its front half beside the update kernel, or, when
    the host's space estimate already makes it a compacting pass, alone.  max_log_points: k_buffer of the second call overflows the
    point log, which the early publish behind it shows to the pass.  Either way the schedule ends in HFPF_ERR_CAPACITY at the
    next read-back at the latest and in HFPF_ERR_STATE from then on, never in a silent success, and the error comes up at the same
    call with the knob on and off."""
    sc = _scene(8)
    plain = _plan(sc)
    monkeypatch.setenv("HFPF_TRACE_CLEAN", "1")
    with hfpf_mod.OccupancyGrid(resolution=sc.resolution, bbox=sc.bbox, **SMALL_CAPS) as g:
        st = Stream(g, sc)
        _drive(g, st, plain[:2])
        c1 = g.counters()
        _drive(g, st, plain[2:])
        c2 = g.counters()
        st.free()
    field = {"max_normals": "voxels_with_normal", "max_log_points": "points_buffered"}[pool]
    assert 1000 < c1[field] and c1[field] + 1000 < c2[field]
    cap = (c1[field] + c2[field]) // 2
    seen = {}
    for overlap in (True, False):
        monkeypatch.setenv("HFPF_CLEAN_OVERLAP", "1" if overlap else "0")
        capfd.readouterr()
        with hfpf_mod.OccupancyGrid(resolution=sc.resolution, bbox=sc.bbox, **dict(SMALL_CAPS, **{pool: cap})) as g:
            st = Stream(g, sc)
            at, err = _until_error(hfpf_mod, g, st, plain)
            print("%s = %d, HFPF_CLEAN_OVERLAP=%d: op %r raised %r; passes (beside, alone) = %r" % (pool, cap, overlap, at, err, _passes(capfd)))
            assert err is not None, "the overflow went unreported"
            assert err.code == -3  # HFPF_ERR_CAPACITY
            with pytest.raises(hfpf_mod.HfpfError) as e:
                g.clean()
            assert e.value.code == -5  # HFPF_ERR_STATE: poisoned until hfpf_clear
            g.clear()
            st.integrate(0, BATCH)
            g.clean()
            g.sync()
            st.free()
        seen[overlap] = (at, str(err))
    assert seen[True] == seen[False]
