"""GPU: the internal limits of the integrate call and the replay -- round capacity, cell record and descriptor fields, the descriptor
array, a full record table, pre-dependant lists, a streamed replay of several rounds, kBufLdsMin, the wave grouping of k_integrate,
its occupancy stage and the largest frame id -- with the crafted clouds of tests/crafted.py against the oracle with exact moments.
test_crafted_models.py asserts on the CPU that every cloud reaches its limit; here every case also asserts, from the engine's own
counters, that the limit WAS reached: the exact growth of update_extra_rounds, table_misses > 0, points_direct unchanged, or the
clean trace.

The session recipe.  A parked point needs a bin plan, and the plan of a launch is the demand of the one before (x scale x slack
+ 64 a region): base surface, clean, the crafted frame once (the demand launch), sync, the identical frame again (the measured
launch).  One hfpf_integrate_device call is one launch.  Where a brick holds more than CAP points its fill is 1 (mod CAP), so a
single point that missed the bin changes the rounds."""
import sys

import numpy as np
import pytest

import crafted as X
import gpu_support as G
import scenes

pytestmark = pytest.mark.gpu

CAPS = dict(max_bricks=4096, max_log_points=1 << 20, max_normals=1 << 15, max_frames=64)   # the log has 64 regions: 16384 entries for a brick's runs
ORACLE_COUNTERS = (("presented", "points_presented"), ("zclip_pass", "points_zclip_pass"), ("inserted", "points_in_bbox"),
                   ("occupied", "voxels_occupied"), ("normals", "voxels_with_normal"), ("buffered", "points_buffered"))

# name -> (the shape the figures are computed for, colour, environment, engine keywords, k_update_cells counts its rounds)
FORMS = {
    "dense": ("dense", False, {"HFPF_UPD_SHAPE": "0"}, {}, True),
    "wide": ("wide", False, {"HFPF_UPD_SHAPE": "1"}, {}, True),
    "colour": ("dense_colour", True, {"HFPF_UPD_SHAPE": "0"}, {}, True),
    "wide_colour": ("wide_colour", True, {"HFPF_UPD_SHAPE": "1"}, {}, True),
    "per_point": ("dense", False, {"HFPF_UPDATE_FORM": "p"}, {}, False),
    "unbinned": ("dense", False, {}, dict(binned_update=False), False),
}
_engine_rows = {}   # (case, colour) -> (form, rows): all forms of one cloud give the same bytes


def _set_env(monkeypatch, env, trace=False):
    """Exactly `env` of the variables that pick a form; the clean trace where a case reads it."""
    for v in G.FORM_VARIABLES:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        assert k in G.FORM_VARIABLES, k
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("HFPF_TRACE_CLEAN", "1" if trace else "0")


def _stderr(capfd):
    cap = capfd.readouterr()
    sys.stdout.write(cap.out)
    return cap.err


def _launch(g, op):
    """One hfpf_integrate_device call, waited for."""
    buf = np.concatenate([np.ascontiguousarray(f).view(np.uint8).reshape(-1) for f in op.frames])
    stride = op.n_points * 16
    with G.uploaded(g, buf) as (dev,):
        g.integrate_device(dev, len(op.frames), stride, op.n_points, np.stack([np.asarray(p, np.float64).reshape(12) for p in op.poses]),
                           frame_ids=None if op.ids is None else np.array(op.ids, np.uint32))
        g.sync()


def _drive(g, case, between=None):
    """The case's schedule; returns (counters behind every op, occupied lists behind the ops of case.snaps)."""
    ctr, occ = [], {}
    for i, op in enumerate(case.ops):
        if between:
            between(g, i)
        if op is X.CLEAN:
            g.clean()
        else:
            _launch(g, op)
        ctr.append(g.counters())
        if i in case.snaps:
            occ[i] = g.occupied().copy()
    return ctr, occ


def _engine(hfpf_mod, monkeypatch, case, form, between=None, trace=False):
    _, colour, env, kw, _ = FORMS[form]
    _set_env(monkeypatch, env, trace)
    with hfpf_mod.OccupancyGrid(resolution=X.RES, bbox=X.BBOX, fuse_color=colour, **case.config, **dict(CAPS, **case.caps), **kw) as g:
        assert g.dims[0] == X.DIMS
        ctr, occ = _drive(g, case, between)
        rows, occ_end, contract = g.extract().copy(), g.occupied().copy(), G.contract_counters(g)
    return dict(counters=ctr, occupied=occ, rows=rows, occ=occ_end, contract=contract)


def _growth(ctr, i, name):
    return ctr[i][name] - (ctr[i - 1][name] if i else 0)


def _against_the_oracle(case, form, run, ref, what):
    """Rows (fourteen columns byte for byte, mean_dist and sd_dist within the derived bounds), the occupied list as a set, the oracle's
    six counters behind every op, members = the rows' counts, and the bytes of every other form of the same cloud."""
    colour = FORMS[form][1]
    rep = scenes.compare_rows_exact(ref["rows"], run["rows"])
    assert rep["exact_bytes_differing"] == 0
    assert np.array_equal(X.occupied_keys(run["occ"]), X.occupied_keys(ref["occ"])), "%s: occupied sets differ" % what
    for i, (c_ref, c) in enumerate(zip(ref["counters"], run["counters"])):
        for a, b in ORACLE_COUNTERS:
            assert c_ref[a] == c[b], "%s: behind op %d: %s %d, the oracle's %s %d" % (what, i, b, c[b], a, c_ref[a])
    members = int(ref["rows"]["count"].astype(np.int64).sum())
    assert run["contract"]["dep_pairs_member"] + run["contract"]["replay_members"] == members, "%s: %d + %d members, the oracle's rows count %d" % (
        what, run["contract"]["dep_pairs_member"], run["contract"]["replay_members"], members)
    if colour:
        assert len(np.unique(run["rows"]["rgb"])) > 100
    first = _engine_rows.setdefault((case.name, colour), (form, run["rows"], run["contract"]))
    assert first[1].tobytes() == run["rows"].tobytes(), "%s: rows differ from those of the form %s" % (what, first[0])
    assert first[2] == run["contract"], "%s: contract counters %r, the form %s has %r" % (what, run["contract"], first[0], first[2])


# ---- k_update_cells ------------------------------------------------------------------------------------------------------------------

def _update_case(oracle_mod, hfpf_mod, monkeypatch, case, form, table_full=False):
    shape, colour, _, kw, counts_rounds = FORMS[form]
    ref = X.oracle_run(oracle_mod, case, shape, colour)
    fg = ref["figures"]
    run = _engine(hfpf_mod, monkeypatch, case, form)
    m = case.measured
    ctr = run["counters"]
    what = "%s, %s" % (case.name, form)
    print("%s: fill %r, expected extra rounds %d; over the measured launch: points_direct +%d, update_extra_rounds +%d, table_misses +%d, dep_pairs_tested +%d" % (
        what, fg["fill"], fg["rounds"], _growth(ctr, m, "points_direct"), _growth(ctr, m, "update_extra_rounds"), _growth(ctr, m, "table_misses"),
        _growth(ctr, m, "dep_pairs_tested")))
    if not kw:   # a binned engine: every point of the measured launch was parked
        assert _growth(ctr, m, "points_direct") == 0, "%s: %d points of the measured launch took the direct forms" % (what, _growth(ctr, m, "points_direct"))
    if counts_rounds:
        assert _growth(ctr, m, "update_extra_rounds") == fg["rounds"], "%s: update_extra_rounds grew by %d, the fill %r makes it %d" % (
            what, _growth(ctr, m, "update_extra_rounds"), fg["fill"], fg["rounds"])
        if table_full and ref["records"] > X.ENGINE[shape]["slots"]:
            assert _growth(ctr, m, "table_misses") > 0, "%s: %d records with members and no table miss" % (what, ref["records"])
    # every (point, dependant) pair of the launch is tested once, whatever the form
    pairs = int((fg["n"] * fg["deps"]).sum())
    assert _growth(ctr, m, "dep_pairs_tested") == pairs, "%s: %d pairs tested, the cloud holds %d" % (what, _growth(ctr, m, "dep_pairs_tested"), pairs)
    _against_the_oracle(case, form, run, ref, what)
    return run, ref


@pytest.mark.parametrize("where", ["first", "last", "odd"])
@pytest.mark.parametrize("form", list(FORMS))
def test_one_cell_fills_a_round(oracle_mod, hfpf_mod, monkeypatch, form, where):
    """Case 1: n_c = CAP in round 0 (the 12-bit count at 2048, chunk index 255), one point in round 1; the cell at local index 0, at 511,
    and at 7 behind a cell with one point (a first position that is not zero)."""
    _update_case(oracle_mod, hfpf_mod, monkeypatch, X.one_cell_fills_a_round(FORMS[form][0], where), form)


@pytest.mark.parametrize("k", range(4), ids=["cap", "cap_plus_1", "two_caps", "two_caps_plus_1"])
@pytest.mark.parametrize("form", list(FORMS))
def test_round_boundaries(oracle_mod, hfpf_mod, monkeypatch, form, k):
    """Case 2: extra rounds 0, 1, 1, 2.  The fills CAP and 2 CAP are not 1 (mod CAP): a point that missed the bin would leave their
    rounds as they are, so for them points_direct and the plan (demand + 64 a region) carry the evidence that all were parked."""
    _update_case(oracle_mod, hfpf_mod, monkeypatch, X.round_boundaries(FORMS[form][0], k), form)


@pytest.mark.parametrize("form", list(FORMS))
def test_more_items_than_descriptors(oracle_mod, hfpf_mod, monkeypatch, form):
    """Case 3: the 9-step search over s_items, with cells that have no items in the middle of it."""
    _update_case(oracle_mod, hfpf_mod, monkeypatch, X.more_items_than_descriptors(FORMS[form][0]), form)


@pytest.mark.parametrize("form", list(FORMS))
def test_full_table(oracle_mod, hfpf_mod, monkeypatch, form):
    """Case 4: 640 records with members against 352 or 512 slots, the shape forced; no HFPF_TEST_TABLE_SKIP."""
    _update_case(oracle_mod, hfpf_mod, monkeypatch, X.full_table(FORMS[form][0]), form, table_full=True)


@pytest.mark.parametrize("form", list(FORMS))
def test_largest_item_sums(oracle_mod, hfpf_mod, monkeypatch, form):
    """Case 5: full chunks of members at the far end of the segment, just inside the radius."""
    _update_case(oracle_mod, hfpf_mod, monkeypatch, X.largest_item_sums(FORMS[form][0]), form)


@pytest.mark.parametrize("form", list(FORMS))
def test_pre_dependant_lists(oracle_mod, hfpf_mod, monkeypatch, form):
    """Case 6: more than CAP points in cells occupied in the running epoch whose list is their pre-dependant (nv_line entries)."""
    _update_case(oracle_mod, hfpf_mod, monkeypatch, X.pre_dependant_lists(FORMS[form][0]), form)


# ---- the streamed replay ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["dense", "wide", "colour", "wide_colour"])
def test_streamed_replay_of_several_rounds(oracle_mod, hfpf_mod, monkeypatch, capfd, form):
    """Case 7: T's REPLAY_M x CAP + 1 buffered points are one run; the waited, streaming pass replays them in REPLAY_M + 1 rounds, and the
    second pass again with the lists cut down to its own registrants."""
    shape, colour, env, _, _ = FORMS[form]
    case = X.streamed_replay(shape)
    ref = X.oracle_run(oracle_mod, case, shape, colour)
    monkeypatch.setitem(FORMS, form, (shape, colour, dict(env, **G.WAITED, **G.STREAM), {}, True))
    _stderr(capfd)
    run = _engine(hfpf_mod, monkeypatch, case, form, trace=True)
    lines, passes = G.clean_trace(_stderr(capfd))
    for ln in lines:
        print("    " + ln)
    ctr = run["counters"]
    what = "%s, %s" % (case.name, form)
    assert _growth(ctr, 0, "points_direct") == 0, "%s: %d points of the first call were not parked" % (what, ctr[0]["points_direct"])
    assert ctr[0]["update_extra_rounds"] == 0
    assert len(passes) == 2 and all(p["waited"] and p["single"] >= 1 for p in passes), "a pass did not stream: %r" % (passes,)
    for i in (1, 3):
        assert _growth(ctr, i, "update_extra_rounds") == X.REPLAY_M, "%s: pass behind op %d: update_extra_rounds grew by %d" % (what, i, _growth(ctr, i, "update_extra_rounds"))
    assert _growth(ctr, 3, "replay_members") > X.REPLAY_M * X.ENGINE[shape]["cap"] // 4, "the second pass's registrants found few members in T's run"
    _against_the_oracle(case, form, run, ref, what)


# ---- k_buffer ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("colour", [False, True], ids=["plain", "colour"])
@pytest.mark.parametrize("spread", [False, True], ids=["single_cell", "spread"])
def test_buffer_runs_at_kBufLdsMin(oracle_mod, hfpf_mod, monkeypatch, spread, colour):
    """Case 8: runs of 255, 256 and 257 points, ids out of order with the smallest id's camera on the other side; then 10 points more."""
    form = "colour" if colour else "dense"
    case = X.buffer_runs(spread)
    ref = X.oracle_run(oracle_mod, case, "dense", colour)
    run = _engine(hfpf_mod, monkeypatch, case, form)
    ctr, m = run["counters"], case.measured
    what = "%s, %s" % (case.name, form)
    for i in (m, m + 1):
        assert _growth(ctr, i, "points_direct") == 0, "%s: op %d: %d points were not parked" % (what, i, _growth(ctr, i, "points_direct"))
    assert _growth(ctr, m, "points_buffered") == sum(X.BUF_COUNTS) and _growth(ctr, m + 1, "points_buffered") == 30
    _against_the_oracle(case, form, run, ref, what)
    rows = run["rows"]
    new = rows[rows["iz"] == X.BUF_LAYER]
    assert len(new) >= 3 and (new["count"] > 0).all()
    if not spread:   # every frame touched the cell: the smallest id's camera, above the sheets, decides
        assert (new["nz"] > 0).all(), "the cells of layer %d look at the camera above" % X.BUF_LAYER
    else:            # a cell the smallest id did not touch looks down
        assert (new["nz"] > 0).sum() > 50 and (new["nz"] < 0).sum() > 10


# ---- k_integrate ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["dense", "colour", "unbinned"])
def test_wave_grouping_extremes(oracle_mod, hfpf_mod, monkeypatch, form):
    """Case 9: all 64 lanes lead (three identical frames race for the same directory entries), a whole frame in one cell, two bricks
    alternating with four groups a wave.  Compared behind every launch, before any clean."""
    colour = FORMS[form][1]
    case = X.wave_grouping()
    ref = X.oracle_run(oracle_mod, case, "dense", colour)
    run = _engine(hfpf_mod, monkeypatch, case, form)
    ctr = run["counters"]
    a, b, c = case.snaps
    assert _growth(ctr, a, "bricks_allocated") == 1024 and _growth(ctr, b, "bricks_allocated") == 0 and _growth(ctr, c, "bricks_allocated") == 0
    for i in case.snaps:
        assert np.array_equal(X.occupied_keys(run["occupied"][i]), X.occupied_keys(ref["occupied"][i])), "occupied sets differ behind op %d" % i
    _against_the_oracle(case, form, run, ref, "%s, %s" % (case.name, form))


def test_occupancy_staging(oracle_mod, hfpf_mod, monkeypatch):
    """Case 10: every point the first touch of its cell, five tiles and more for each of the k_integrate workgroups (sized for
    INTEGRATE_GRID = 2048 of them; a device with more takes fewer tiles a workgroup and the case reaches the flush less often).  A wave
    stages 64 cells a tile: four tiles fill s_occ to exactly kOccStage, the fifth flushes.  Counters and the occupied set behind the
    launch; no clean pass."""
    _set_env(monkeypatch, {})
    rec, pose, n = X.occupancy_staging()
    og = oracle_mod.OracleGrid(resolution=X.OCC_RES, bbox=X.OCC_BBOX)
    og.capture(rec, pose)
    c_ref, occ_ref = og.counters(), X.occupied_keys(og.occupied())
    og.close()
    assert c_ref["occupied"] == n
    with hfpf_mod.OccupancyGrid(resolution=X.OCC_RES, bbox=X.OCC_BBOX, max_bricks=1 << 15, max_log_points=1 << 23, max_normals=1 << 20, max_frames=16) as g:
        _launch(g, X.single(rec, pose))
        c = g.counters()
        occ = X.occupied_keys(g.occupied())
    for a, b in ORACLE_COUNTERS:
        assert c_ref[a] == c[b], "counter %s: %d, the oracle's %s %d" % (b, c[b], a, c_ref[a])
    assert np.array_equal(occ, occ_ref), "occupied sets differ"


def test_largest_frame_id(oracle_mod, hfpf_mod, monkeypatch):
    """Case 11: ids 2^23 - 1, 0 and 2^23 - 2 through the direct forms and through the parked word; 2^23 is refused and the handle goes on."""
    case = X.largest_frame_id()
    ref = X.oracle_run(oracle_mod, case, "dense", False)
    refused = []

    def between(g, i):
        if i != 1:
            return
        op = case.ops[1]
        with pytest.raises(hfpf_mod.HfpfError) as e:
            _launch(g, X.Launch(op.frames, op.poses, [0, X.MAX_FRAMES, 1]))
        refused.append(e.value.code)

    run = _engine(hfpf_mod, monkeypatch, case, "dense", between)
    assert refused == [-3], "HFPF_ERR_CAPACITY"
    ctr = run["counters"]
    assert ctr[0]["points_direct"] == 3 * case.ops[0].n_points, "a session's first small call takes the direct forms"
    assert _growth(ctr, 1, "points_direct") == 0, "%d points of the planned call were not parked" % _growth(ctr, 1, "points_direct")
    assert ctr[1]["frames_integrated"] == 6
    _against_the_oracle(case, "dense", run, ref, case.name)
    rows = run["rows"]
    assert ((rows["nz"] > 0) == (rows["ix"] % 2 == 1)).all()
