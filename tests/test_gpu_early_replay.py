"""GPU: the buffer replay of a small overlapped clean pass fed from the pass's registrations, beside the update kernel of the integrate
call before it (k_replay_reg, HFPF_EARLY_REPLAY, default on; csrc/hfpf.hip clean_locked), computes what the replay behind the
dependant-table update computes.  Every case is run three ways -- knob on, knob off, oracle (exact moments) through the same
schedule: the engine's rows byte-identical on and off, fourteen columns byte-identical with the oracle's exact rows, the counters a
pass produces equal; the HFPF_TRACE_CLEAN lines say which replay every pass took, so every case knows that the registration-fed form
ran with the knob on and never with it off.  Each case also asserts the precondition that makes it a test of what it is about.

Batches of four 160x120 frames at 1 mm, SMALL capacities (the shapes of test_gpu_clean_overlap.py); a pass replays early only where
it overlaps: from the second batch of a session on.

The fallback case has no compacting leg.  dep[] holds 14 x max_normals entries and the host's space estimate for the fifth pass of
that schedule (20 frames, 81797 records) stays below 0.9 M entries: a pool that still holds the records (84000: 1.18 M entries) never
makes a pass of it a compacting one -- measured from 84000 to 200000 in steps of 4000 -- and a schedule long enough to fill dep[]
would take far more than a few seconds.  test_gpu_parity.py's compacting case runs frame by frame, where no pass overlaps."""
import numpy as np
import pytest

import scenes
from gpu_support import SMALL_CAPS, contract_counters

pytestmark = pytest.mark.gpu

W, H, RES, FX = 160, 120, 0.001, 615.0
BATCH = 4
EQUAL_COUNTERS = ("voxels_with_normal", "registrations", "dep_entries", "replay_members")
BESIDE, ALONE = "front half beside the update kernel", "front half on the engine's stream"
FED, BEHIND = "replay fed from the registrations", "replay behind the dependant-table update"
WATCHED_CELLS = 20000  # occupied cells whose dependant lists the oracle run looks at around the watched pass


def _scene(n_frames=12):
    """Random poses (30 degrees, 5 cm): every batch sees cells of the batches before it again, and its new normals register on cells
    that have been buffering points without a normal since."""
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


def _plan(sc):
    """[('integrate', first, n), ('clean',), ...]: batches with a clean after each."""
    ops = []
    for first in range(0, sc.n_frames, BATCH):
        ops += [("integrate", first, min(BATCH, sc.n_frames - first)), ("clean",)]
    return ops


def _drive(g, st, ops):
    """Runs ops; returns what every ('counters',) read."""
    seen = []
    for op in ops:
        if op[0] == "integrate":
            st.integrate(op[1], op[2])
        elif op[0] == "clean":
            g.clean()
        elif op[0] == "counters":
            seen.append(g.counters())
        else:
            raise AssertionError(op)
    return seen


def _passes(capfd):
    """One (front half beside?, replay fed from the registrations?) per clean pass since the last call, from the trace lines."""
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("hfpf: clean pass")]
    for ln in lines:
        assert (BESIDE in ln) != (ALONE in ln) and (FED in ln) != (BEHIND in ln), ln
    return [(BESIDE in ln, FED in ln) for ln in lines]


def _engine(hfpf_mod, monkeypatch, capfd, sc, ops, early, **kw):
    """One engine run of `ops` on a fresh handle with the knob set: (rows, final counters, counters read on the way, passes)."""
    monkeypatch.setenv("HFPF_EARLY_REPLAY", "1" if early else "0")
    monkeypatch.setenv("HFPF_TRACE_CLEAN", "1")
    capfd.readouterr()
    with hfpf_mod.OccupancyGrid(resolution=sc.resolution, bbox=sc.bbox, **dict(SMALL_CAPS, **kw)) as g:
        st = Stream(g, sc)
        seen = _drive(g, st, ops)
        rows = g.extract().copy()
        ctr = g.counters()
        st.free()
    return rows, ctr, seen, _passes(capfd)


_oracle_cache = {}


def _oracle(oracle_mod, sc, key, ops, color=False, watch_pass=None):
    """The oracle driven through the schedule (frame by frame: a batch is the engine's affair), once per key: (exact rows, the largest
    number of registrants one of the first WATCHED_CELLS occupied cells gained in clean pass number watch_pass (0-based), or None)."""
    if key not in _oracle_cache:
        og = oracle_mod.OracleGrid(resolution=sc.resolution, bbox=sc.bbox, exact_moments=True, **(dict(fuse_color=True) if color else {}))
        lay = sc.layout
        kw = dict(point_step=lay["point_step"], off_x=lay["off_x"], off_y=lay["off_y"], off_z=lay["off_z"])
        if color:
            kw["off_rgb"] = lay["off_rgb"]
        n_pass, gained = 0, None
        for op in ops:
            if op[0] == "integrate":
                for f in range(op[1], op[1] + op[2]):
                    og.capture(sc.frame(f), sc.poses[f], **kw)
            elif op[0] == "clean":
                if n_pass == watch_pass:
                    cells = [tuple(int(v) for v in c) for c in og.occupied()[:WATCHED_CELLS]]
                    before = [len(og.dependants(*c)) for c in cells]
                    og.clean()
                    gained = max(len(og.dependants(*c)) - b for c, b in zip(cells, before))
                else:
                    og.clean()
                n_pass += 1
        og.extract()
        exact = og.extract_exact()
        og.close()
        exact.setflags(write=False)
        _oracle_cache[key] = (exact, gained)
    return _oracle_cache[key]


def _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, sc, ops, key, min_fed, watch_pass=None, **kw):
    """Knob on, knob off, oracle: what every case asserts.  Returns (rows, final counters, counters on the way, passes) of the run
    with the knob on and the oracle's watched gain."""
    on, c_on, seen_on, p_on = _engine(hfpf_mod, monkeypatch, capfd, sc, ops, True, **kw)
    off, c_off, seen_off, p_off = _engine(hfpf_mod, monkeypatch, capfd, sc, ops, False, **kw)
    print("passes (beside, fed): knob on %r, knob off %r" % (p_on, p_off))
    assert not any(fed for _, fed in p_off), "HFPF_EARLY_REPLAY=0 must keep every replay behind the dependant-table update"
    assert [b for b, _ in p_on] == [b for b, _ in p_off], "the knob must not change which passes overlap"
    assert all(b for b, fed in p_on if fed), "a replay fed from the registrations belongs to an overlapped pass"
    n_fed = sum(fed for _, fed in p_on)
    assert n_fed >= max(min_fed, 1), "the schedule was chosen so that %d passes replay early; %d did" % (min_fed, n_fed)
    assert on.tobytes() == off.tobytes(), "rows differ between HFPF_EARLY_REPLAY=1 and 0"
    for k in EQUAL_COUNTERS:
        assert c_on[k] == c_off[k], "counter %s: %d with the early replay, %d without" % (k, c_on[k], c_off[k])
        for a, b in zip(seen_on, seen_off):
            assert a[k] == b[k], "counter %s on the way: %d with the early replay, %d without" % (k, a[k], b[k])
    oracle_ops = [op for op in ops if op[0] != "counters"]
    exact, gained = _oracle(oracle_mod, sc, key, oracle_ops, color=bool(kw.get("fuse_color")), watch_pass=watch_pass)
    rep = scenes.compare_rows_exact(exact, on)
    assert rep["exact_bytes_differing"] == 0
    return (on, c_on, seen_on, p_on), gained


def _after_first_pass(sc):
    """The plan with a counters read behind the first pass (it stands between a pass and the next call: every later pass still
    finds its call's early publish)."""
    plan = _plan(sc)
    return plan[:2] + [("counters",)] + plan[2:]


# ---- 1: cells that stayed without a normal over several batches gain registrants ----------------------------------------------
def test_multi_batch_replay(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd):
    sc = _scene()
    (rows, ctr, seen, passes), gained = _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, sc, _after_first_pass(sc), ("batches", False), 2,
                                                    watch_pass=2)
    assert passes == [(False, False), (True, True), (True, True)]
    later = ctr["replay_members"] - seen[0]["replay_members"]
    print("replay members: %d in the first pass, %d in the overlapped ones; largest gain of a watched cell in the last pass: %d" %
          (seen[0]["replay_members"], later, gained))
    assert later > 0, "no buffered point became a member in an overlapped pass: the early replay had nothing to do"
    assert gained >= 2, "no watched cell gained two registrants in the watched pass"
    assert len(rows) > 10000 and ctr["clean_passes"] == 3


# ---- 2: part of the buffered points reaches the log through k_integrate_overflow's direct append ----------------------------------
def test_directly_appended_entries(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd):
    monkeypatch.setenv("HFPF_TEST_BIN_SCALE", "0.16")
    sc = _scene()
    (rows, ctr, seen, passes), _ = _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, sc, _after_first_pass(sc), ("batches", False), 2, watch_pass=2)
    print("points_direct %d of %d buffered; replay members of the overlapped passes %d" %
          (ctr["points_direct"], ctr["points_buffered"], ctr["replay_members"] - seen[0]["replay_members"]))
    assert ctr["points_direct"] > 0, "no point took the direct forms: the bin plan was not shrunk far enough"
    assert ctr["replay_members"] - seen[0]["replay_members"] > 0


# ---- 3: the COLOR instantiation --------------------------------------------------------------------------------------------------------
def test_colour(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd):
    sc = _scene()
    (rows, ctr, seen, passes), _ = _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, sc, _after_first_pass(sc), ("batches", True), 2, fuse_color=True)
    assert ctr["replay_members"] - seen[0]["replay_members"] > 0
    assert len(np.unique(rows["rgb"])) > 1000


# ---- 4: passes of every form in one session ----------------------------------------------------------------------------------------
def test_fallbacks_in_one_session(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd):
    """First pass (no update kernel before it), a pass behind a counters read (no early publish: the plain order), two early-replay
    passes, again a pass behind a counters read: what a pass of one form leaves -- dep_tmp all zero, the lists, the statistics --
    is what a pass of the other form expects."""
    sc = _scene(20)
    plan = _plan(sc)
    ops = plan[:3] + [("counters",)] + plan[3:9] + [("counters",)] + plan[9:]
    (rows, ctr, seen, passes), _ = _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, sc, ops, ("fallbacks", False), 2)
    assert passes == [(False, False), (False, False), (True, True), (True, True), (False, False)]
    assert ctr["clean_passes"] == 5 and ctr["replay_members"] > seen[1]["replay_members"] > seen[0]["replay_members"]


# ---- 5: snapshot right behind an early-replay pass ------------------------------------------------------------------------------
def test_snapshot_after_an_early_replay(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd):
    """hfpf_snapshot checks the lists and that the scratch words are zero: it would reject a note that k_depinc_fill left with no replay behind it to clear it.  The
    restored handle finishes the schedule with the rows of the uninterrupted run."""
    sc = _scene()
    plain = _plan(sc)
    (whole, c_whole, _, _), _ = _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, sc, _after_first_pass(sc), ("batches", False), 2, watch_pass=2)
    monkeypatch.setenv("HFPF_EARLY_REPLAY", "1")
    monkeypatch.setenv("HFPF_TRACE_CLEAN", "1")
    capfd.readouterr()
    with hfpf_mod.OccupancyGrid(resolution=sc.resolution, bbox=sc.bbox, **SMALL_CAPS) as src:
        st = Stream(src, sc)
        _drive(src, st, plain[:4])  # two batches, two passes: the second one replayed early
        blob = src.snapshot()
        assert _passes(capfd) == [(False, False), (True, True)]
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
