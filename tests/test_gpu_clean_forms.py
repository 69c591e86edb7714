"""GPU: the forms of a clean pass that the host picks by size (CleanLimits, csrc/host_plan.hpp) -- the waited pass with its mid-pass
read-back, the streaming replay of single-run bricks beside the chain walk (k_replay with skip_single), the sorted chain walk,
k_gate<4>, k_register<kRegTilesLarge> -- compute what their small siblings compute.  At their default sizes only the benchmark and
full-size sessions reach them; here HFPF_TEST_*_MIN lower the sizes (stream 256, sort 1024, register 1024, gate 4096) and
HFPF_CLEAN_NOWAIT=0 makes a pass wait, so that 160 x 120 frames run them.

Every case is run three ways -- the form forced, the defaults (the small forms every other test pins), the oracle with exact moments
through the same schedule: rows byte-identical between the two engine runs, fourteen columns byte-identical with the oracle's exact
rows, the occupied lists equal, the contract's counters equal between the engine runs; and the `hfpf: clean forms` lines of
HFPF_TRACE_CLEAN=1 say which form every pass took, so every case knows that its form ran when forced and never by default.  Those
lines are printed for the reader of the log.

The scene is fed the way the benchmark feeds its own: one hfpf_integrate_device call of 12 frames per epoch (more than the probe's 8,
so the first call makes a bin plan), then a clean; three epochs.  The passes have 71159, 31749 new + 11786 pending and 26406 new +
9275 pending candidates and touch 59388, 45938 and 40618 cells -- every figure many times the lowered size it is held against.  How
many touched cells lie in single-run bricks is engine state: the trace reports it, and the cases assert it."""
import collections
import sys

import numpy as np
import pytest

import scenes
from gpu_support import (FORM_VARIABLES, GATE4_MIN, LARGE, SMALL_CAPS, SORT, SORT_MIN, STREAM, STREAM_MIN, WAITED, DeviceFrames, clean_trace,
                         contract_counters, frame_bytes)

pytestmark = pytest.mark.gpu

EPOCH = 12

Run = collections.namedtuple("Run", "rows occ contract counters passes")

_scene_cache = {}
_oracle_cache = {}
_default_cache = {}


def _scene():
    """(scene, its frames as bytes), rendered once."""
    if not _scene_cache:
        sc = scenes.Scene(36, 160, 120, 0.001, fx=615.0, clean_every=EPOCH)
        clouds = frame_bytes(sc)
        clouds.setflags(write=False)
        _scene_cache["sc"] = (sc, clouds)
    return _scene_cache["sc"]


def _plan(sc, epochs=3):
    """[('integrate', first, n), ('clean',), ...]: one call per epoch with a clean behind it."""
    ops = []
    for first in range(0, min(sc.n_frames, epochs * EPOCH), EPOCH):
        ops += [("integrate", first, min(EPOCH, sc.n_frames - first)), ("clean",)]
    return ops


def _drive(g, st, ops):
    for op in ops:
        if op[0] == "integrate":
            st.integrate(op[1], op[2])
        elif op[0] == "counters":
            g.counters()
        else:
            g.clean()


def _set_env(monkeypatch, env):
    """Exactly `env` of the variables that pick a form, and the trace."""
    for v in FORM_VARIABLES:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        assert k in FORM_VARIABLES, k
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("HFPF_TRACE_CLEAN", "1")


def _stderr(capfd):
    """What stderr has gathered since the last call.  (What the test has printed since is printed again: it is captured too, and
    would be lost with the read.)"""
    cap = capfd.readouterr()
    sys.stdout.write(cap.out)
    return cap.err


def _trace(capfd, what):
    lines, passes = clean_trace(_stderr(capfd))
    print("%s:" % what)
    for ln in lines:
        print("    " + ln)
    return passes


def _read(g, passes):
    rows, occ = g.extract().copy(), g.occupied().copy()
    return Run(rows, occ, contract_counters(g), g.counters(), passes)


def _engine(hfpf_mod, monkeypatch, capfd, env, what, color=False, epochs=3, **kw):
    """One run of the whole schedule on a fresh handle created under `env`."""
    sc, clouds = _scene()
    _set_env(monkeypatch, env)
    _stderr(capfd)
    with hfpf_mod.OccupancyGrid(resolution=sc.resolution, bbox=sc.bbox, fuse_color=color, **dict(SMALL_CAPS, **kw)) as g:
        st = DeviceFrames(g, sc, clouds)
        _drive(g, st, _plan(sc, epochs))
        run = _read(g, None)
        st.free()
    return run._replace(passes=_trace(capfd, what))


def _default(hfpf_mod, monkeypatch, capfd, color=False, epochs=3, **kw):
    """The run with no variable set, once per configuration (read-only)."""
    key = (color, epochs) + tuple(sorted(kw.items()))
    if key not in _default_cache:
        run = _engine(hfpf_mod, monkeypatch, capfd, {}, "defaults %r" % (key,), color=color, epochs=epochs, **kw)
        for a in (run.rows, run.occ):
            a.setflags(write=False)
        _default_cache[key] = run
    return _default_cache[key]


def _oracle(oracle_mod, color=False, K=3, epochs=3):
    """(exact rows, occupied list) of the oracle through the same schedule (frame by frame: a batch is the engine's affair), once per
    (colour, K, epochs)."""
    if (color, K, epochs) not in _oracle_cache:
        sc, _ = _scene()
        og = oracle_mod.OracleGrid(resolution=sc.resolution, bbox=sc.bbox, exact_moments=True, K=K, **(dict(fuse_color=True) if color else {}))
        lay = sc.layout
        kw = dict(point_step=lay["point_step"], off_x=lay["off_x"], off_y=lay["off_y"], off_z=lay["off_z"])
        if color:
            kw["off_rgb"] = lay["off_rgb"]
        for op in _plan(sc, epochs):
            if op[0] == "integrate":
                for f in range(op[1], op[1] + op[2]):
                    og.capture(sc.frame(f), sc.poses[f], **kw)
            else:
                og.clean()
        og.extract()
        exact, occ = og.extract_exact(), og.occupied()
        og.close()
        for a in (exact, occ):
            a.setflags(write=False)
        _oracle_cache[(color, K, epochs)] = (exact, occ)
    return _oracle_cache[(color, K, epochs)]


def _forms(p):
    """The size-gated forms a pass took, as a set of names."""
    f = set()
    if p["waited"]:
        f.add("waited")
        if p["single"]:
            f.add("streamed")
        if p["sorted"]:
            f.add("sorted")
    if p["gate_tiles"] == 4:
        f.add("gate4")
    if p["register"] == "large":
        f.add("register large")
    if p["compacting"] != "no":
        f.add("compacting")
    return f


def _same(forced, ref, oracle, what, epochs=3):
    """What every case asserts of two engine runs and the oracle, but for the forms."""
    exact, occ_ref = oracle
    assert len(forced.rows) > 50000 and forced.counters["clean_passes"] == epochs, "%s: %d rows, %d passes" % (what, len(forced.rows), forced.counters["clean_passes"])
    assert forced.rows.tobytes() == ref.rows.tobytes(), "%s: rows differ from the default run's" % what
    rep = scenes.compare_rows_exact(exact, forced.rows)
    assert rep["exact_bytes_differing"] == 0
    assert np.array_equal(forced.occ, ref.occ), "%s: occupied list differs from the default run's" % what
    assert np.array_equal(forced.occ, occ_ref), "%s: occupied list differs from the oracle's" % what
    for k in forced.contract:
        assert forced.contract[k] == ref.contract[k], "%s: counter %s: %d, default run %d" % (what, k, forced.contract[k], ref.contract[k])
    assert forced.contract["replay_members"] > 0 and (forced.contract["dep_pairs_member"] > 0 or epochs == 1)  # (one epoch: no update kernel ran)


def _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, env, what, default_forms=frozenset(), color=False, K=None, epochs=3, **kw):
    """Forced, defaults, oracle.  The default run takes none of the forms (default_forms: but these).  Returns (forced, default)."""
    if K is not None:
        kw["K"] = K
    ref = _default(hfpf_mod, monkeypatch, capfd, color=color, epochs=epochs, **kw)
    forced = _engine(hfpf_mod, monkeypatch, capfd, env, what, color=color, epochs=epochs, **kw)
    assert len(ref.passes) == epochs and len(forced.passes) == epochs, "passes traced: %d by default, %d forced" % (len(ref.passes), len(forced.passes))
    for p in ref.passes:
        assert _forms(p) <= default_forms, "the default run took %r in pass %d" % (sorted(_forms(p)), p["pass"])
    for a, b in zip(forced.passes, ref.passes):
        assert (a["candidates"], a["pending"], a["new"]) == (b["candidates"], b["pending"], b["new"]), "pass %d: %r vs %r" % (a["pass"], a, b)
    _same(forced, ref, _oracle(oracle_mod, color, 3 if K is None else K, epochs), what, epochs)
    return forced, ref


def _all_waited(passes):
    for p in passes:
        assert p["waited"] and p["compacting"] == "no" and p["use_marks"] == 1, p
        assert not p["fed"], "a waited pass replays behind its read-back: %r" % (p,)
        assert p["single"] + p["walked"] > 0, "pass %d touched no cell" % p["pass"]


# ---- 1: the waited pass, its replay an unsorted chain walk ----------------------------------------------------------------------
def test_waited_pass_unsorted_walk(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd):
    forced, _ = _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, dict(WAITED, HFPF_STREAM_REPLAY="0"), "waited, unsorted walk")
    _all_waited(forced.passes)
    for p in forced.passes:
        assert _forms(p) == {"waited"} and p["walked"] >= SORT_MIN, p  # (only the limit keeps this walk unsorted)


# ---- 2: ... in slot order (sort_keys_u32 over touched_list with slot_bits) --------------------------------------------------------
def test_waited_pass_sorted_walk(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd):
    forced, _ = _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, dict(WAITED, **SORT, HFPF_STREAM_REPLAY="0"), "waited, sorted walk")
    _all_waited(forced.passes)
    for p in forced.passes:
        assert _forms(p) == {"waited", "sorted"} and p["walked"] >= SORT_MIN, p


def _mixed(passes):
    """Passes in which single-run bricks streamed and the chain walk took other cells (k_replay with skip_single = 1)."""
    return [p for p in passes if p["single"] > 0 and p["walked"] > 0]


# ---- 3: the streaming replay beside the chain walk, in the four instantiations launch_update_cells<true> can take ---------------------
@pytest.mark.parametrize("shape", [0, 1], ids=["dense", "wide"])
@pytest.mark.parametrize("color", [False, True], ids=["plain", "colour"])
def test_streaming_replay_beside_the_chain_walk(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd, color, shape):
    forced, _ = _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, dict(WAITED, **STREAM, HFPF_UPD_SHAPE=str(shape)),
                            "streaming beside the walk, colour %r, shape %d" % (color, shape), color=color)
    _all_waited(forced.passes)
    for p in forced.passes:
        assert "sorted" not in _forms(p), p
        assert p["single"] == 0 or p["single"] >= STREAM_MIN, p
    assert _mixed(forced.passes), "no pass streamed some cells and walked others: %r" % (forced.passes,)
    if color:
        assert len(np.unique(forced.rows["rgb"])) > 1000


# ---- 4: streaming and the sorted walk together -----------------------------------------------------------------------------------
def test_streaming_replay_beside_the_sorted_walk(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd):
    forced, _ = _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, dict(WAITED, **STREAM, **SORT), "streaming beside the sorted walk")
    _all_waited(forced.passes)
    both = [p for p in _mixed(forced.passes) if p["sorted"]]
    assert both, "no pass streamed some cells and walked others in slot order: %r" % (forced.passes,)
    for p in forced.passes:
        assert p["sorted"] == (p["walked"] >= SORT_MIN), p


# ---- 5: k_gate<4> and k_register<kRegTilesLarge> ----------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap,K", [(True, 3), (False, 3), (True, 1), (True, 5)], ids=["beside", "alone", "K1", "K5"])
def test_gate4_and_register_large(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd, overlap, K):
    """No-wait passes: from the second batch on their front half -- gate and registration -- runs on front_stream beside the update
    kernel (or, with HFPF_CLEAN_OVERLAP=0, on the engine's stream).  Register blocks are tiles x (2K + 1): K = 1 and K = 5 as well."""
    env = dict(LARGE) if overlap else dict(LARGE, HFPF_CLEAN_OVERLAP="0")
    forced, ref = _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, env, "gate<4>, register large, overlap %r, K %d" % (overlap, K), K=K)
    for p in forced.passes:
        assert _forms(p) == {"gate4", "register large"}, p
        assert p["candidates"] >= GATE4_MIN and p["candidates"] == p["pending"] + p["new"], p
    assert [p["beside"] for p in forced.passes] == ([False, True, True] if overlap else [False] * 3), forced.passes
    assert [p["beside"] for p in ref.passes] == [False, True, True], ref.passes
    for p in forced.passes[1:]:
        assert p["pending"] > 0 and p["new"] > 0, "pass %d has no pending or no new list: %r" % (p["pass"], p)
        assert p["candidates"] % 1024 != 0 and p["candidates"] % 2048 != 0, p


# ---- 6: a planned compacting pass under the waited, sorted walk -------------------------------------------------------------------
def test_planned_compacting_pass(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd):
    """max_normals = 1.3 x the rows + 64, as in test_gpu_parity.py's compacting case -- of the scene's FIRST epoch, at K = 1.

    plan_clean compacts when dep + 2 (reg + prereg) + 2 (2K + 1) n_in + n_new exceeds max_dep = 2 (2K + 1) max_normals.  In the
    three-epoch schedule at K = 3 no capacity that holds the 122922 rows does that: measured at the head of pass 3, dep = 230703
    and reg = 175884 against 2 x 7 x 35681 + 26406 = 525940 for the pass itself and max_dep = 14 x 123000 = 1722000 at the least
    (no pass compacted for max_normals from 123000 to 159862, the 1.3 x of that schedule).  A first pass has dep = reg = prereg = 0
    and compacts when n_in (1 + 1 / (2 (2K + 1))) > max_normals: with its 71159 candidates and 59373 rows, 1.3 x 59373 + 64 = 77248
    lies above 76241 (K = 3) and below 83018 (K = 1).  So: one epoch, K = 1.  The planned rebuild leaves no notes (use_marks 0),
    never streams, and its replay walks every cell with a registrant, sorted here."""
    exact, _ = _oracle(oracle_mod, K=1, epochs=1)
    max_normals = int(len(exact) * 1.3) + 64
    forced, ref = _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, dict(WAITED, **SORT, **STREAM), "planned compacting, sorted walk",
                              default_forms=frozenset(("waited", "compacting")), K=1, epochs=1, max_normals=max_normals)
    (p,), (d,) = forced.passes, ref.passes
    assert p["compacting"] == "planned" and d["compacting"] == "planned", "max_normals %d made the pass no compacting one: %r, by default %r" % (max_normals, p, d)
    assert p["waited"] and p["use_marks"] == 0 and p["single"] == 0 and p["sorted"] and p["walked"] >= SORT_MIN, p
    assert d["waited"] and d["use_marks"] == 0 and d["single"] == 0 and not d["sorted"] and d["walked"] == p["walked"], d


# ---- 7: the direct-update handle never streams ------------------------------------------------------------------------------------
def test_direct_update_handle_never_streams(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd):
    """plan_replay needs `binned`: with cases 2 and 3's variables set, a handle of the direct forms walks (and sorts) everything.  The
    default run it is held against is the binned one."""
    ref = _default(hfpf_mod, monkeypatch, capfd)
    forced = _engine(hfpf_mod, monkeypatch, capfd, dict(WAITED, **STREAM, **SORT), "direct-update handle", binned_update=False)
    assert len(forced.passes) == 3
    for p in forced.passes:
        assert _forms(p) == {"waited", "sorted"} and p["single"] == 0 and p["walked"] >= SORT_MIN and not p["beside"], p
    assert all(not _forms(p) for p in ref.passes)
    _same(forced, ref, _oracle(oracle_mod), "direct-update handle")


# ---- 8: restore, then stream ------------------------------------------------------------------------------------------------------
def test_restore_then_stream(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd):
    """The streaming replay reads run_start, run_len and run_cnt from a restore: the snapshot is dirty (epoch 2 buffered, not yet
    replayed), the restored handle's first pass streams it.

    The source reads its counters behind the first pass.  Without that read-back the restored pass reported single 0, with it the
    4613 cells a session whose first pass waited reports.  (Read from the code, not measured: the host of a no-wait pass does not
    learn of the bricks the pass's registrations allocate, so the second call's spare bin regions go to those, the bricks that call
    discovers take the direct forms -- run_cnt bit 0x100 -- and no brick of the second epoch is single-run.)"""
    sc, clouds = _scene()
    plan = _plan(sc)
    ref = _default(hfpf_mod, monkeypatch, capfd)
    _set_env(monkeypatch, {})
    _stderr(capfd)
    with hfpf_mod.OccupancyGrid(resolution=sc.resolution, bbox=sc.bbox, **SMALL_CAPS) as src:
        st = DeviceFrames(src, sc, clouds)
        _drive(src, st, plan[:2] + [("counters",)] + plan[2:3])  # epoch 1, clean, (read-back,) epoch 2
        blob = src.snapshot()
        info = hfpf_mod.snapshot_info(blob)
        assert (info["frames_integrated"], info["clean_passes"]) == (2 * EPOCH, 1), "the snapshot was to hold an epoch that no pass has replayed: %r" % (info,)
        _set_env(monkeypatch, dict(WAITED, **STREAM))
        with hfpf_mod.OccupancyGrid(resolution=sc.resolution, bbox=sc.bbox, **SMALL_CAPS) as dst:
            dst.restore(blob)
            assert contract_counters(src) == contract_counters(dst)
            src_passes = _trace(capfd, "source, up to the snapshot")
            st2 = DeviceFrames(dst, sc, clouds)
            _drive(dst, st2, plan[3:])
            restored = _read(dst, _trace(capfd, "restored handle"))
            st2.free()
        _drive(src, st, plan[3:])
        source = _read(src, src_passes + _trace(capfd, "source, behind the snapshot"))
        st.free()
    assert len(restored.passes) == 2 and len(source.passes) == 3
    assert all(not _forms(p) for p in source.passes), source.passes
    first = restored.passes[0]
    assert first["waited"] and first["single"] >= STREAM_MIN and first["compacting"] == "no", "the pass behind the restore did not stream: %r" % (first,)
    assert (first["candidates"], first["pending"], first["new"]) == tuple(source.passes[1][k] for k in ("candidates", "pending", "new"))
    _same(restored, source, _oracle(oracle_mod), "restored against its source")
    _same(source, ref, _oracle(oracle_mod), "source against the uninterrupted run")


# ---- 9: the documented switches -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("var,value", [("HFPF_MAILBOX", "0"), ("HFPF_BIN_SPARE", "0"), ("HFPF_BIN_SLACK", "1"), ("HFPF_BIN_SLACK", "4")])
def test_documented_switches(oracle_mod, hfpf_mod, synth_mod, monkeypatch, capfd, var, value):
    """tuning and A/B switches change how the work is scheduled, never what is fused."""
    forced, ref = _three_ways(oracle_mod, hfpf_mod, monkeypatch, capfd, {var: value}, "%s=%s" % (var, value))
    assert all(not _forms(p) for p in forced.passes), forced.passes
    assert [p["beside"] for p in ref.passes] == [False, True, True], ref.passes
    if var == "HFPF_MAILBOX":
        assert not any(p["beside"] or p["fed"] for p in forced.passes), "clean_starts_early needs the mailbox: %r" % (forced.passes,)
    else:
        assert [p["beside"] for p in forced.passes] == [False, True, True], forced.passes
    if var == "HFPF_BIN_SPARE":
        print("points_direct: %d without spare regions, %d by default" % (forced.counters["points_direct"], ref.counters["points_direct"]))
        assert forced.counters["points_direct"] >= ref.counters["points_direct"]
