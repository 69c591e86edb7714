"""GPU: the sharded session's epoch exchange on crafted clouds (tests/shards.py drives tests/crafted.py schedules over 2 to 4 handles).

Every case asserts (a) the merged rows byte for byte against the oracle's exact rows (and scenes.compare_rows), (b) against one handle
running the same schedule, (c) every rank's occupied set against the single handle's and one voxels_with_normal on all ranks, (d) the
points_presented counters summing to the points of the schedule, and (e) its own precondition -- from the oracle or from the log of
exported records alone -- without which it could pass and never reach what it is named for.  The log itself is checked on the way:
every export is cells first, then two records a frame; the cells of all exports are the single handle's occupied set; and, where
the log is small enough to fold in Python, exchange_ref over it ends with that set and one latch a cell on every rank.

A count of ONE record cannot be exported by a rank that has occupied a cell (a frame adds two): that import is
test_gpu_exchange_records.py::test_import_distinct_cells_at_tile_and_workgroup_boundaries[1], on a hand-built array."""
import numpy as np
import pytest

import crafted as X
import exchange_ref as E
import faces
import gpu_support as G
import scenes
import shards as S

pytestmark = pytest.mark.gpu

SHAPE0 = {"HFPF_UPD_SHAPE": "0"}
# test_gpu_crafted.FORMS: name -> (the shape the figures are computed for, colour, environment)
FORMS = {"dense": ("dense", False, SHAPE0), "colour": ("dense_colour", True, SHAPE0)}


def _env(monkeypatch, env=None):
    """Exactly `env` of the variables that pick a form (none: a run with defaults)."""
    for v in G.FORM_VARIABLES:
        monkeypatch.delenv(v, raising=False)
    for k, v in (env or {}).items():
        assert k in G.FORM_VARIABLES, k
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("HFPF_TRACE_CLEAN", "0")


def _keys_of_log(log, dims):
    """Every cell record of the log as X.occupied_keys would key it, sorted and unique."""
    recs = [r[~E.is_frame(r)] for sink in log for r in sink]
    cells = E.key_cells(dims, np.concatenate(recs)["key"]).astype(np.int64) if recs else np.zeros((0, 3), np.int64)
    return np.unique(X.occupied_keys(cells))


def _check(oracle_mod, hfpf_mod, ops, deal, world, mode, colour=False, config=None, caps=None, bbox=X.BBOX, res=X.RES, dims=X.DIMS,
           extract_on=(0,), poison=None, what=""):
    """(a) to (d) and the log; returns (sharded run, single run, oracle run)."""
    kw = dict(colour=colour, config=config)
    ref = S.run_oracle(oracle_mod, ops, bbox=bbox, res=res, **kw)
    one = S.run_single(hfpf_mod, ops, caps=caps, bbox=bbox, res=res, **kw)
    run = S.run_sharded(hfpf_mod, ops, deal, world, mode, caps=caps, bbox=bbox, res=res, extract_on=extract_on, poison=poison, **kw)
    assert len(ref["exact"]) > 0, "%s: the oracle has no rows" % what
    for r, rows in run["rows"].items():
        rep = scenes.compare_rows_exact(ref["exact"], rows)
        assert rep["exact_bytes_differing"] == 0
        scenes.compare_rows(ref["rows"], rows)
        assert rows.tobytes() == one["rows"].tobytes(), "%s: the rows merged on rank %d differ from one handle's" % (what, r)
    want = X.occupied_keys(one["occ"])
    assert np.array_equal(want, X.occupied_keys(ref["occ"])), "%s: the single handle's occupied set is not the oracle's" % what
    for r, occ in enumerate(run["occ"]):
        assert np.array_equal(X.occupied_keys(occ), want), "%s: rank %d's occupied set differs from one handle's" % (what, r)
    normals = {c["voxels_with_normal"] for c in run["counters"]}
    assert normals == {one["counters"]["voxels_with_normal"]}, "%s: voxels_with_normal %r, one handle %d" % (what, normals, one["counters"]["voxels_with_normal"])
    presented = sum(c["points_presented"] for c in run["counters"])
    assert presented == run["points"] == one["counters"]["points_presented"], "%s: %d points presented of %d" % (what, presented, run["points"])
    for x, sink in enumerate(run["log"]):
        for r, rec in enumerate(sink):
            S.check_export_shape(rec, "%s: exchange %d, rank %d" % (what, x, r))
    assert np.array_equal(_keys_of_log(run["log"], dims), want), "%s: the exported cells are not the occupied set" % what
    if sum(len(r) for sink in run["log"] for r in sink) <= 30000:
        mf = dict(S.CAPS, **(caps or {}))["max_frames"]
        model = S.replay_log(run["log"], world, dims, mf)[0]
        assert np.array_equal(X.occupied_keys(np.array(sorted(model.occupied), np.int64)), want), "%s: exchange_ref over the log" % what
    return run, one, ref


def _growth(run, i, rank, name):
    return run["per_op"][i][rank][name] - (run["per_op"][i - 1][rank][name] if i else 0)


# ---- import tile boundaries -----------------------------------------------------------------------------------------------------------

BIG_X, BIG_Y = (8, 100), (8, 68)   # a sheet of 92 x 60 cells: up to 4095 cells in one layer


def _tile_ops(n_cells, receiver_has_half):
    """Epoch 1: rank 1 integrates a frame (id 0, from above) on a small sheet of its own or on every second one of the cells to come;
    then rank 0 occupies exactly n_cells cells of layer 40 with one frame (id 1).  Epoch 2: rank 1 looks at all of them again.  (The
    oracle captures launch by launch: ids rise from one launch to the next.)"""
    cells = X.sheet((40,), BIG_X, BIG_Y)[:n_cells]
    other = cells[::2] if receiver_has_half else X.sheet((60,), (8, 18), (8, 18))
    ops = [X.single(*X.points(other, 0x5A01, spread=0.3, flip=True), fid=0), X.single(*X.points(cells, 0x5A00 + n_cells, spread=0.3), fid=1), X.CLEAN,
           X.single(*X.points(cells, 0x5A02), fid=2), X.CLEAN]
    return cells, other, ops, (lambda li, fi, fid: {0: 1, 1: 0, 3: 1}[li])


@pytest.mark.parametrize("total", [255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097])
def test_import_tile_boundaries(oracle_mod, hfpf_mod, monkeypatch, total):
    """Ranks 1 and 2 import `total` = n_cells + 2 records from rank 0 in one launch ("lists"): at, one below and one above a tile of
    256 and a workgroup of 2048 records."""
    _env(monkeypatch)
    cells, _, ops, deal = _tile_ops(total - 2, False)
    run, _, _ = _check(oracle_mod, hfpf_mod, ops, deal, 3, "lists", what="tile boundary %d" % total)
    first = run["log"][0]
    assert len(first[0]) == total, "rank 0 exported %d records, the case is built for %d" % (len(first[0]), total)
    assert len(first[2]) == 0 and len(run["log"][1][0]) == 0, "a rank without a frame exported records"


@pytest.mark.parametrize("total", [2049, 4096])
def test_import_where_the_receiver_holds_every_second_cell(oracle_mod, hfpf_mod, monkeypatch, total):
    """Rank 1 has occupied every second one of rank 0's cells itself: its import finds half the records' cells there (f_first is
    sparse within every tile, the occ_list reservation smaller than the tile), and the latch of those cells is rank 1's own id 0."""
    _env(monkeypatch)
    cells, other, ops, deal = _tile_ops(total - 2, True)
    run, _, _ = _check(oracle_mod, hfpf_mod, ops, deal, 3, "lists", what="tile boundary %d, half held" % total)
    first = run["log"][0]
    assert len(first[0]) == total and len(first[1]) == len(other) + 2 == (total - 1) // 2 + 2
    k0, k1 = first[0]["key"][:total - 2], first[1]["key"][:len(other)]
    assert np.isin(k1, k0).all() and np.array_equal(np.isin(k0, k1), np.isin(k0, E.make_key(X.DIMS, other)))
    rows = run["rows"][0]
    mine = rows[np.isin(E.make_key(X.DIMS, np.stack([rows["ix"], rows["iy"], rows["iz"]], 1)), k1)]
    assert len(mine) > 0.3 * len(other) and (mine["nz"] > 0).all(), "the cells rank 1 saw first, from above, look up"


# ---- shared cells ---------------------------------------------------------------------------------------------------------------------

def _shared_ops(world, low, swap=False, layers=X.LAYERS_A):
    """Every rank's frame covers the same sheets.  Rank r's frame has the id (r - low) mod world -- rank `low` holds the smallest --
    and ids alternate between the camera below and above.  swap: the ids 0 and 1 change places (the poses stay with the frames).  The
    second epoch repeats it with the ids world .. 2 world - 1."""
    cells = X.sheet(layers)
    ops = []
    for epoch in range(2):
        order = [(r - low) % world for r in range(world)]
        made = [X.points(cells, 0x5B00 + 16 * epoch + r, flip=order[r] % 2 == 1) for r in range(world)]
        ids = [({0: 1, 1: 0}.get(k, k) if swap else k) + epoch * world for k in order]
        ops += [X.Launch([m[0] for m in made], [m[1] for m in made], ids, "shared cells, epoch %d" % epoch), X.CLEAN]
    return ops, (lambda li, fi, fid: fi)


def _sign_changes(oracle_mod, ops, swapped):
    a, b = S.run_oracle(oracle_mod, ops)["exact"], S.run_oracle(oracle_mod, swapped)["exact"]
    assert len(a) == len(b) and all(np.array_equal(a[k], b[k]) for k in ("ix", "iy", "iz"))
    return int(((a["nz"] > 0) != (b["nz"] > 0)).sum())


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("world,low", [(w, low) for w in (3, 4) for low in range(w)])
def test_shared_cells(oracle_mod, hfpf_mod, monkeypatch, world, low, mode):
    """The same cells newly occupied by every rank in one epoch, the smallest id on the rank imported first (0), last (world - 1) and
    on each importing rank in turn.  In "concat" mode the same key sits in two and three foreign arrays of one launch."""
    _env(monkeypatch)
    ops, deal = _shared_ops(world, low)
    changed = _sign_changes(oracle_mod, ops, _shared_ops(world, low, swap=True)[0])
    assert changed >= 500, "%d rows whose normal depends on which of the two smallest ids is latched" % changed
    run, _, _ = _check(oracle_mod, hfpf_mod, ops, deal, world, mode, what="shared cells, world %d, low %d, %s" % (world, low, mode))
    first = run["log"][0]
    for r in range(world):   # what each rank exported: its own id on every cell
        cells_r, ff = S.log_cells(first[r])
        assert len(cells_r) == len(X.sheet(X.LAYERS_A)) and (ff == (r - low) % world).all()
    for i in range(world):
        foreign = np.concatenate([first[j]["key"][~E.is_frame(first[j])] for j in range(world) if j != i])
        _, n = np.unique(foreign, return_counts=True)
        assert (n >= 2).sum() >= 500, "importer %d: %d keys in two foreign arrays" % (i, (n >= 2).sum())


def test_gathered_padding_and_own_slice_are_never_read(oracle_mod, hfpf_mod, monkeypatch):
    """The padded buffer built by hand: stride 2048 records and more beyond the largest count; all padding and the importer's own
    slice hold well-formed poison -- cells of layer 70, which no rank occupies, with first_frame 0, and frame records that would
    overwrite every real frame's viewpoint with NaN.  Byte-equal to the oracle and to one handle (as the unpoisoned runs of
    test_shared_cells are), and no poison cell is occupied."""
    _env(monkeypatch)
    world = 3
    ops, deal = _shared_ops(world, 1)
    bad_cells = X.sheet((70,))
    poison = np.concatenate([E.cell_records(X.DIMS, bad_cells, 0), E.frame_records(np.arange(2 * world), np.full((2 * world, 3), np.nan))])
    poison = poison[np.random.default_rng(0x5C00).permutation(len(poison))]
    run, one, _ = _check(oracle_mod, hfpf_mod, ops, deal, world, "gathered", poison=poison, what="poisoned gathered buffer")
    clean_run = S.run_sharded(hfpf_mod, ops, deal, world, "gathered")
    assert run["rows"][0].tobytes() == clean_run["rows"][0].tobytes(), "the poisoned run differs from the unpoisoned one"
    bad = X.occupied_keys(bad_cells)
    for r, occ in enumerate(run["occ"]):
        assert not np.isin(X.occupied_keys(occ), bad).any(), "rank %d occupies a poison cell" % r
    buf, stride, counts = S.poisoned_buffer(run["log"][0], 0, poison)
    assert stride // 16 >= int(counts.max()) + 2048 and len(buf) == world * (stride // 16) and (counts == len(X.sheet(X.LAYERS_A)) + 2).all()
    own = buf[:stride // 16]
    assert np.isin(own["key"], poison["key"]).all() and np.isnan(E.record_floats(own[E.is_frame(own)])).any(), "the importer's own slice is not poison"


# ---- frame ids ------------------------------------------------------------------------------------------------------------------------

def _non_monotone_ops(swap=False):
    """One launch of four frames with the ids 5, 2, 9, 0 on windows of three sheets that overlap, the second from above; then a frame
    over everything.  swap: the ids 0 and 2 change places."""
    ids = [5, 0, 9, 2] if swap else [5, 2, 9, 0]
    made = [X.points(X.sheet((40, 43, 46), (32 + 2 * k, 48 + 2 * k)), 0x5D00 + k, flip=k == 1) for k in range(4)]
    ops = [X.Launch([m[0] for m in made], [m[1] for m in made], ids, "non-monotone ids"), X.CLEAN,
           X.single(*X.points(X.sheet((40, 43, 46), (32, 54)), 0x5D10), fid=10), X.CLEAN]
    owner = [0, 1, 2, 1]
    return ops, (lambda li, fi, fid: owner[fi] if li == 0 else 0)


@pytest.mark.parametrize("mode", S.MODES)
def test_non_monotone_ids_within_an_epoch(oracle_mod, hfpf_mod, monkeypatch, mode):
    _env(monkeypatch)
    ops, deal = _non_monotone_ops()
    changed = _sign_changes(oracle_mod, ops, _non_monotone_ops(swap=True)[0])
    assert changed >= 300, "%d rows whose normal depends on the ids 0 and 2" % changed
    run, _, _ = _check(oracle_mod, hfpf_mod, ops, deal, 3, mode, what="non-monotone ids, %s" % mode)
    first = run["log"][0]
    per_rank = [dict(zip(r["key"][~E.is_frame(r)].tolist(), r["first_frame"][~E.is_frame(r)].tolist())) for r in first]
    differing = sum(1 for k, v in per_rank[1].items() if k in per_rank[0] and per_rank[0][k] != v)
    assert differing >= 100 and set(per_rank[1].values()) == {0, 2} and set(per_rank[0].values()) == {5}, "the ranks' latches before the exchange"


@pytest.mark.parametrize("mode", ["lists", "concat"])
def test_largest_frame_id_sharded(oracle_mod, hfpf_mod, monkeypatch, mode):
    """crafted.largest_frame_id with max_frames = 2^23: the frame with the id 2^23 - 1 on rank 0, the ids 0 and 2^23 - 2, which latch
    every cell, on ranks 1 and 2.  Rank 0 exports every cell with 2^23 - 1 and ends with none of them latched by it."""
    _env(monkeypatch)
    case = X.largest_frame_id()
    run, _, _ = _check(oracle_mod, hfpf_mod, case.ops, lambda li, fi, fid: fi, 3, mode, caps=case.caps, what="largest frame id, %s" % mode)
    first = run["log"][0]
    cells0, ff0 = S.log_cells(first[0])
    assert len(cells0) == len(case.cells) and (ff0 == X.MAX_FRAMES - 1).all()
    assert sorted(set((first[0]["key"][E.is_frame(first[0])] & np.uint64(0xFFFFFFFF)).tolist())) == [X.MAX_FRAMES - 1]
    assert set(S.log_cells(first[2])[1].tolist()) == {X.MAX_FRAMES - 2} and set(S.log_cells(first[1])[1].tolist()) == {0}
    rows = run["rows"][0]
    assert len(rows) > 300 and ((rows["nz"] > 0) == (rows["ix"] % 2 == 1)).all()


# ---- bricks a rank has only through an import -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", S.MODES)
def test_import_made_bricks(oracle_mod, hfpf_mod, monkeypatch, mode):
    """Rank 0 alone sees region A (layer 40 of the sheets: nine bricks, the points in random order), rank 1 alone region B (layer 60,
    further along x).  Behind the clean rank 1 integrates a frame into A, into bricks it holds through the import alone and cells that
    have normals on it through the replicated clean alone."""
    _env(monkeypatch)
    a, b = X.sheet((40,)), X.sheet((60,), (64, 88))
    a = a[np.random.default_rng(0x5E00).permutation(len(a))]
    ops = [X.Launch([X.points(a, 0x5E01)[0], X.points(b, 0x5E02)[0]], [X.pose_of()] * 2, [0, 1], "A and B"), X.CLEAN,
           X.single(*X.points(a, 0x5E03), fid=2), X.CLEAN]
    deal = lambda li, fi, fid: fi if li == 0 else 1
    before = {}

    def each(og, i):
        if i == 2:
            rows = X.rows_now(og)
            before["count"] = rows[rows["iz"] == 40]["count"].astype(np.int64)

    og_rows = S.run_oracle(oracle_mod, ops, each=each)["exact"]
    after = og_rows[og_rows["iz"] == 40]["count"].astype(np.int64)
    assert len(after) == len(before["count"]) >= 400 and (after > before["count"]).sum() >= 300, "the oracle's rows in A gain no members from rank 1's frame"
    run, _, _ = _check(oracle_mod, hfpf_mod, ops, deal, 2, mode, what="import-made bricks, %s" % mode)
    cells0, _ = S.log_cells(run["log"][0][0])
    assert len(cells0) == len(a) and (S.log_cells(run["log"][0][1])[0][:, 2] == 60).all()
    runs = [len(np.unique(X.brick_of(cells0[j:j + 64]), axis=0)) for j in range(0, len(cells0) - 63, 64)]
    assert max(runs) >= 3, "no 64-record run of rank 0's export spans three bricks: %r" % runs
    assert _growth(run, 2, 1, "points_in_bbox") == len(a) and _growth(run, 2, 1, "bricks_allocated") == 0


# ---- ranks with nothing -------------------------------------------------------------------------------------------------------------------

def _idle_ops():
    return X.base_ops() + [X.single(*X.points(X.sheet((40, 43, 46)), 0x5F00)), X.single(*X.points(X.sheet((41, 44, 47)), 0x5F01, flip=True)), X.CLEAN]


def test_a_rank_that_never_integrates(oracle_mod, hfpf_mod, monkeypatch):
    """World 3, rank 2 without a frame in the whole session; extract taken on it and on rank 0."""
    _env(monkeypatch)
    run, _, _ = _check(oracle_mod, hfpf_mod, _idle_ops(), lambda li, fi, fid: fid % 2, 3, "lists", extract_on=(0, 2), what="rank 2 idle")
    assert run["rows"][0].tobytes() == run["rows"][2].tobytes()
    assert all(len(sink[2]) == 0 for sink in run["log"]) and run["counters"][2]["points_presented"] == 0 and run["counters"][2]["frames_integrated"] == 0
    assert all(len(sink[0]) > 0 for sink in run["log"]) and all(run["counters"][r]["points_presented"] > 0 for r in (0, 1))


@pytest.mark.parametrize("mode", ["gathered", "concat"])
def test_a_rank_idle_in_the_first_epoch(oracle_mod, hfpf_mod, monkeypatch, mode):
    _env(monkeypatch)
    run, _, _ = _check(oracle_mod, hfpf_mod, _idle_ops(), lambda li, fi, fid: 0 if li < 2 else (fid + 1) % 2, 2, mode, extract_on=(0, 1), what="rank 1 idle at first")
    assert run["rows"][0].tobytes() == run["rows"][1].tobytes()
    assert len(run["log"][0][1]) == 0 and all(len(sink[1]) > 0 for sink in run["log"][1:]), "rank 1's exports: %r" % [len(s[1]) for s in run["log"]]


def test_a_frame_wholly_outside_the_box(oracle_mod, hfpf_mod, monkeypatch):
    """Rank 1's only frame of the first epoch lies beyond the box's +x face: its export is that frame's two records and no cell."""
    _env(monkeypatch)
    outside = X.sheet((40,), (X.DIMS[0] + 3, X.DIMS[0] + 27))
    ops = _idle_ops()
    ops.insert(1, X.single(*X.points(outside, 0x5F10)))
    run, _, _ = _check(oracle_mod, hfpf_mod, ops, lambda li, fi, fid: 1 if li == 1 else (0 if li < 4 else fid % 2), 2, "lists", what="a frame outside the box")
    rec = run["log"][0][1]
    assert len(rec) == 2 and E.is_frame(rec).all() and (rec["key"] & np.uint64(0xFFFFFFFF)).tolist() == [1, 1], "rank 1's first export: %r" % (rec,)
    assert run["per_op"][1][1]["points_presented"] == len(outside) and run["per_op"][1][1]["points_in_bbox"] == 0


# ---- the hot path's limit cases, sharded --------------------------------------------------------------------------------------------------

def _shard_case(oracle_mod, case, world=2):
    """The case's schedule for `world` ranks: the base surface stays as it is (rank 0 takes it); a launch of several frames is split
    over the ranks frame by frame; a launch of one frame without an id becomes a launch of `world` frames -- the original and twins
    with the same number of points in every cell, other positions and colours -- one a rank.  The demand and the measured launch of
    a case share their frame, and so their twins."""
    og = X.oracle_grid(oracle_mod, case)
    twins, ops = {}, []
    try:
        for i, op in enumerate(case.ops):
            if op is X.CLEAN or op.tag == "base" or len(op.frames) > 1 or op.ids is not None:
                ops.append(op)
                continue
            key = id(op.frames[0])
            if key not in twins:
                idx, valid = X.cells_of(og, op.frames[0], op.poses[0])
                assert valid.all() and np.array_equal(op.poses[0], X.pose_of())
                twins[key] = [X.points(idx, 0x7100 + 16 * i + r)[0] for r in range(1, world)]
            ops.append(X.Launch([op.frames[0]] + twins[key], [op.poses[0]] * world, None, op.tag))
    finally:
        og.close()
    return ops, (lambda li, fi, fid: 0 if ops[li].tag == "base" else fi % world)


def _limit_case(oracle_mod, hfpf_mod, monkeypatch, case, form, env=None, mode="lists"):
    shape, colour, form_env = FORMS[form]
    _env(monkeypatch, dict(form_env, **(env or {})))
    ops, deal = _shard_case(oracle_mod, case)
    run, _, _ = _check(oracle_mod, hfpf_mod, ops, deal, 2, mode, colour=colour, config=case.config, caps=case.caps, what="%s, sharded, %s" % (case.name, form))
    if colour:
        assert len(np.unique(run["rows"][0]["rgb"])) > 100
    return run


def _parked(run, i, rank):
    return _growth(run, i, rank, "points_in_bbox") - _growth(run, i, rank, "points_direct")


@pytest.mark.parametrize("k", range(4), ids=["cap", "cap_plus_1", "two_caps", "two_caps_plus_1"])
@pytest.mark.parametrize("form", list(FORMS))
def test_round_boundaries_sharded(oracle_mod, hfpf_mod, monkeypatch, form, k):
    """Each rank parks a fill of CAP, CAP + 1, 2 CAP, 2 CAP + 1 of its own in T and updates records that everybody's cells registered."""
    case = X.round_boundaries(FORMS[form][0], k)
    run = _limit_case(oracle_mod, hfpf_mod, monkeypatch, case, form)
    m, cap = case.measured, X.ENGINE[FORMS[form][0]]["cap"]
    for r in (0, 1):
        assert _parked(run, m, r) == (cap, cap + 1, 2 * cap, 2 * cap + 1)[k], "rank %d parked %d points of the measured launch" % (r, _parked(run, m, r))
        assert _growth(run, m, r, "update_extra_rounds") == (0, 1, 1, 2)[k], "rank %d: update_extra_rounds +%d" % (r, _growth(run, m, r, "update_extra_rounds"))


@pytest.mark.parametrize("form", list(FORMS))
def test_more_items_than_descriptors_sharded(oracle_mod, hfpf_mod, monkeypatch, form):
    case = X.more_items_than_descriptors(FORMS[form][0])
    run = _limit_case(oracle_mod, hfpf_mod, monkeypatch, case, form)
    m = case.measured
    for r in (0, 1):
        assert _parked(run, m, r) == case.ops[m].n_points and _growth(run, m, r, "dep_pairs_tested") > 4 * case.ops[m].n_points - 1, "rank %d" % r


@pytest.mark.parametrize("form", list(FORMS))
def test_pre_dependant_lists_sharded(oracle_mod, hfpf_mod, monkeypatch, form):
    case = X.pre_dependant_lists(FORMS[form][0])
    run = _limit_case(oracle_mod, hfpf_mod, monkeypatch, case, form)
    m = case.measured
    for r in (0, 1):
        assert _parked(run, m, r) == case.ops[m].n_points and _growth(run, m, r, "update_extra_rounds") == 1, "rank %d" % r


@pytest.mark.parametrize("form", list(FORMS))
def test_streamed_replay_sharded(oracle_mod, hfpf_mod, monkeypatch, form):
    """The nine frames of the first call dealt 5 : 4: each rank buffers its share of T's points and replays them, at both cleans, against
    registrations made from everybody's cells."""
    case = X.streamed_replay(FORMS[form][0])
    run = _limit_case(oracle_mod, hfpf_mod, monkeypatch, case, form, env=dict(G.WAITED, **G.STREAM))
    for r in (0, 1):
        assert _growth(run, 0, r, "points_buffered") > X.ENGINE[FORMS[form][0]]["cap"] // 2, "rank %d buffered %d points" % (r, _growth(run, 0, r, "points_buffered"))
        for i in (1, 3):
            assert _growth(run, i, r, "replay_members") > 0, "rank %d: the clean behind op %d replayed no member" % (r, i)


@pytest.mark.parametrize("colour", [False, True], ids=["plain", "colour"])
@pytest.mark.parametrize("spread", [False, True], ids=["single_cell", "spread"])
def test_buffer_runs_sharded(oracle_mod, hfpf_mod, monkeypatch, spread, colour):
    case = X.buffer_runs(spread)
    run = _limit_case(oracle_mod, hfpf_mod, monkeypatch, case, "colour" if colour else "dense", mode="concat")
    m = case.measured
    got = [_growth(run, m, r, "points_buffered") for r in (0, 1)]
    assert min(got) > 100 and sum(got) == sum(X.BUF_COUNTS), "points buffered over the measured launch: %r" % got
    new = run["rows"][0][run["rows"][0]["iz"] == X.BUF_LAYER]
    assert len(new) >= 3 and (new["count"] > 0).all()
    if not spread:
        assert (new["nz"] > 0).all(), "the smallest id's camera, above the sheets and on rank 1, decides"


@pytest.mark.parametrize("form", list(FORMS))
def test_wave_grouping_sharded(oracle_mod, hfpf_mod, monkeypatch, form):
    case = X.wave_grouping()
    run = _limit_case(oracle_mod, hfpf_mod, monkeypatch, case, form, mode="gathered")
    a = case.snaps[0]
    for r in (0, 1):
        assert _growth(run, a, r, "bricks_allocated") == 1024, "rank %d claimed %d bricks" % (r, _growth(run, a, r, "bricks_allocated"))


# ---- faces and the largest indices ----------------------------------------------------------------------------------------------------------

def _scene_ops(sc):
    ops = []
    for ev in sc.schedule():
        ops.append(X.single(np.ascontiguousarray(sc.frame(ev[1])).view(np.uint8).reshape(-1, 16), sc.poses[ev[1]]) if ev[0] == "integrate" else X.CLEAN)
    return ops


@pytest.mark.parametrize("name", ["cut", "deepx"])
def test_faces_and_largest_indices_gathered(oracle_mod, hfpf_mod, synth_mod, monkeypatch, name):
    """faces.FaceScene "cut" (all six faces cut the model; occupied cells at index == dim on every axis) and "deepx" (x indices up to
    2^21 - 2: every bit of the key's x field), frames dealt round robin over two ranks, the padded-buffer import."""
    _env(monkeypatch)
    sc = faces.FaceScene(name)
    run, one, ref = _check(oracle_mod, hfpf_mod, _scene_ops(sc), lambda li, fi, fid: fid % 2, 2, "gathered", config=sc.config, caps=G.SMALL_CAPS,
                           bbox=sc.bbox, res=sc.resolution, dims=sc.dims, what=name)
    faces.check_conditions(name, run["rows"][0], run["occ"][1], sc.dims)
    occ = np.asarray(ref["occ"], np.int64)
    assert all(len(S.log_cells(r, sc.dims)[0]) > 1000 for r in run["log"][0]), "a rank exported few cells: %r" % [len(r) for r in run["log"][0]]
    cells = np.vstack([S.log_cells(r, sc.dims)[0] for sink in run["log"] for r in sink])
    for a in range(3):
        lo, hi = int(occ[:, a].min()), int(occ[:, a].max())
        assert hi == sc.dims[a], "the oracle indexes no cell at dim on axis %d" % a
        assert (cells[:, a] == hi).any() and (cells[:, a] == lo).any(), "axis %d: no exported record at %d or at %d" % (a, lo, hi)
        if name == "cut" or a > 0:
            assert lo == 0
    if name == "deepx":
        assert hi_bit(cells[:, 0].max()) == faces.KEY_FIELD_BITS


def hi_bit(v):
    return int(v).bit_length()


# ---- three processes over the host-staged transport -----------------------------------------------------------------------------------------

def _three_proc_worker(rank, world, port, q):
    """One OS process = one rank (all on GPU 0): its own frame of the shared-cells schedule, hfpf_dist.HostStagedTransport over gloo."""
    try:
        import os
        import sys
        here = os.path.dirname(os.path.abspath(__file__))
        root = os.path.dirname(here)
        for p in (os.path.join(root, "high-fidelity-pointcloud-fusion_amd", "python"), here):
            if p not in sys.path:
                sys.path.insert(0, p)
        import torch.distributed as dist
        import hfpf
        import hfpf_dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        ops, deal = _shared_ops(world, 1, layers=(40, 43))
        ids = S.frame_ids(ops)
        g = hfpf.OccupancyGrid(resolution=X.RES, bbox=X.BBOX, **S.CAPS)
        g.attach_transport(hfpf_dist.HostStagedTransport(dist))
        for i, op in enumerate(ops):
            if op is X.CLEAN:
                g.clean()   # collective: the foreign ranks' records joined and imported in one launch
                continue
            mine = [f for f in range(len(op.frames)) if deal(i, f, ids[i][f]) == rank]
            S.integrate(g, [op.frames[f] for f in mine], [op.poses[f] for f in mine], [ids[i][f] for f in mine], op.n_points)
        rows = g.extract()   # collective
        q.put((rank, rows.tobytes()))
        g.close()
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "FAIL: %s\n%s" % (e, traceback.format_exc())))


def test_three_processes_host_staged_transport(oracle_mod, hfpf_mod, monkeypatch):
    """HostStagedTransport.exchange at world 3, where its one import launch holds every shared key twice: three processes on GPU 0,
    each with the rows of one handle and of the oracle."""
    import multiprocessing as mp
    import socket
    _env(monkeypatch)
    world = 3
    ops, _ = _shared_ops(world, 1, layers=(40, 43))
    ref = S.run_oracle(oracle_mod, ops)
    one = S.run_single(hfpf_mod, ops)
    assert scenes.compare_rows_exact(ref["exact"], one["rows"])["exact_bytes_differing"] == 0 and len(one["rows"]) >= 800
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_three_proc_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for r in range(world):
        assert not isinstance(res[r], str), res[r]
        assert res[r] == one["rows"].tobytes(), "rank %d's merged rows differ from one handle's" % r
