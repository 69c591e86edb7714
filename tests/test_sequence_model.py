"""CPU: the model and the scripts of the sequence tests (tests/sequence_support.py), without an engine.  The model must itself be
right where it is the reference -- a rollback by replay, the hidden set across clean passes -- and the scripts of the default seeds
must reach what the GPU test is for: every read-out, behind every kind of predecessor, mostly on a model that has something to show.
These are conditions on the scripts, counted on the oracle's rows; the GPU test holds the engine's rows to the same floors."""
import collections

import numpy as np
import pytest

import hide_ref as HR
import sequence_support as S

N_DEFAULT = 12


@pytest.fixture(scope="module")
def x(synth_mod):
    return S.inputs()


def _model(oracle_mod, x, ops, **cfg):
    m = S.Model(oracle_mod, x, **cfg)
    for op in ops:
        S.apply(op, m)
    return m


def _same(a, b, what):
    assert a.rows().tobytes() == b.rows().tobytes(), "%s: rows, %d vs %d" % (what, len(a.rows()), len(b.rows()))
    assert a.occupied().tobytes() == b.occupied().tobytes(), "%s: occupied list" % what
    assert a.hidden().tobytes() == b.hidden().tobytes() and a.dirty() == b.dirty(), "%s: hidden set, dirtiness" % what


# ---- the model ------------------------------------------------------------------------------------------------------------------------

def test_rollback_by_replay_is_the_straight_run(oracle_mod, x):
    head = [("integrate", "pageable", 0, 4), ("clean",)]
    tail = [("integrate", "device_cloud", 4, 5), ("clean",), ("hide_box", "hide", "middle"), ("integrate", "depth", 9, 1)]
    m = _model(oracle_mod, x, head + [("mark",)] + tail)
    straight = _model(oracle_mod, x, head)
    assert len(m.rows()) < len(m.full_rows()) and len(m.full_rows()) > len(straight.rows()) > 1000 and m.dirty()
    m.rollback(0)
    _same(m, straight, "back to the mark behind the first pass")
    assert len(m.hidden()) == 0 and not m.dirty() and m.log == straight.log
    # a mark on a dirty model with something hidden; clear, show_all and further passes lie between it and the rollback
    S.apply(("hide_list", "hide", 12, "third"), m)
    S.apply(("integrate", "pinned", 4, 1), m)
    tag = m.mark()
    at_mark = m.frozen()
    for op in [("clean",), ("show_all",), ("clear",), ("integrate", "pageable", 5, 1), ("clean",)]:
        S.apply(op, m)
    assert len(m.hidden()) == 0 and m.rows().tobytes() != at_mark.rows().tobytes()
    m.rollback(tag)
    _same(m, at_mark, "back to the dirty mark")
    assert m.dirty() and len(m.hidden()) == (len(straight.rows()) + 2) // 3
    again = _model(oracle_mod, x, head + [("hide_list", "hide", 12, "third"), ("integrate", "pageable", 4, 1)])
    _same(m, again, "the dirty mark against its own straight run")
    for g in (m, straight, again):
        g.close()


def test_hidden_set_follows_the_op_algebra_across_passes(oracle_mod, x):
    m = _model(oracle_mod, x, [("integrate", "pageable", 0, 3), ("clean",)])
    F1 = HR.full_set(m.full_rows())
    counts = m.hide_box(*S.hide_box_of(m, "middle"), "hide")
    H1 = m.H.copy()
    assert 0 < counts["n_hidden"] == len(H1) < len(F1) and np.isin(H1, F1).all(), "H is a subset of F: %r" % (counts,)
    assert len(m.rows()) == len(F1) - len(H1)
    for op in [("integrate", "pageable", 3, 4), ("clean",)]:
        S.apply(op, m)
    F2 = HR.full_set(m.full_rows())
    later = np.setdiff1d(F2, F1)
    assert len(later) > 1000 and np.isin(F1, F2).all(), "the second pass adds rows and takes none away"
    assert np.array_equal(m.H, H1) and np.isin(m.H, F2).all(), "H lasts through integrate and clean"
    seen = HR.keys(HR.row_voxels(m.rows()))
    assert np.isin(later, seen).all() and not np.isin(H1, seen).any(), "a voxel that got its row later is visible, a hidden one is not"
    # SHOW of a part, HIDE_OTHERS of the rest: the counts and the set are hide_ref's, call by call
    v = S.hide_voxels_of(m, "third")
    c = m.hide_voxels(v, "show")
    assert c["n_hidden"] == len(m.H) == len(np.setdiff1d(H1, HR.keys(v[:-2]))) and c["n_full"] == len(F2)
    c = m.hide_voxels(S.hide_voxels_of(m, "most"), "hide_others")
    assert c["n_hidden"] == len(m.H) and len(m.rows()) == len(F2) - len(m.H) and np.isin(m.H, F2).all()
    m.clear()
    assert len(m.H) == 0 and len(m.rows()) == 0 and len(m.occupied()) == 0 and m.dirty(), "clear empties H"
    assert m.hide_voxels(v, "hide") == dict.fromkeys(HR.COUNTS, 0), "a handle without rows hides nothing"
    m.close()


def test_icosphere_and_the_two_invalid_triangles(x):
    v, t = S.icosphere((0.0, 0.0, 0.0), 1.0)
    assert len(t) == 320 and len(v) == 162 and np.allclose(np.linalg.norm(v, axis=1), 1.0, atol=1e-6)
    assert len(np.unique(np.sort(t, axis=1), axis=0)) == 320
    edges = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all(), "closed: every edge is used twice"
    assert len(x.tris) == 322 and x.tris[-2].max() >= len(x.verts) and np.isnan(x.verts[x.tris[-1]]).any()


def test_predecessors_of_a_hand_written_script():
    ops = [("integrate", "device_cloud", 0, 4), ("clean",), ("mark",), ("integrate", "depth", 4, 1), ("check", 0), ("check", 1), ("clean",), ("check", 2),
           ("integrate", "device_depth", 5, 5), ("clean",), ("clean",), ("check", 3), ("clear",), ("check", 4), ("restore", 0), ("check", 5),
           ("hide_box", "hide", "middle"), ("check", 6), ("show_all",), ("check", 7), ("integrate", "device_cloud", 0, 3), ("clean",), ("check", 8)]
    got = [sorted(S.predecessors(ops, j)) for j, op in enumerate(ops) if op[0] == "check"]
    assert got == [["integrate"], ["check"], ["clean"], ["batch_clean", "clean"], ["clear"], ["restore"], ["hide"], ["hide"], ["clean"]]
    with pytest.raises(AssertionError):
        S.predecessors([("mark",), ("check", 0)], 1)


def test_scripts_are_a_function_of_the_seed_alone():
    for seed in range(N_DEFAULT):
        ops = S.script(seed)
        assert ops == S.script(seed) and [op[1] for op in ops if op[0] == "check"] == [(seed * S.N_CHECKS + i) % len(S.READ_OUTS) for i in range(S.N_CHECKS)]
        marks = 0
        for j, op in enumerate(ops):
            if op[0] == "mark":
                marks += 1
            if op[0] == "restore":
                assert 0 <= op[1] < marks, "a restore goes to an earlier mark"
            if op[0] == "integrate":
                assert 0 <= op[2] and op[2] + op[3] <= S.N_FRAMES and (op[3] == 1 or op[1] in S.BATCH_KINDS) and 1 <= op[3] <= 6, op
            if op[0] == "check":
                S.predecessors(ops, j)


# ---- the scripts of the default seeds ------------------------------------------------------------------------------------------------

def test_default_seeds_meet_the_coverage_conditions(oracle_mod, x):
    checks = collections.defaultdict(list)      # read-out -> figures
    before = collections.Counter()              # predecessor -> checks directly behind it
    ops_seen = collections.Counter()
    slowest = 0.0
    for seed in range(N_DEFAULT):
        ops = S.script(seed)
        ops_seen.update((op[0], op[1]) if op[0] in ("integrate", "hide_list", "hide_box") else (op[0],) for op in ops)
        ran, seconds = S.model_run(oracle_mod, seed)
        slowest = max(slowest, seconds)
        print("seed %2d: model-only %.2f s, %s" % (seed, seconds, ", ".join("%s %d" % (S.NAMES[k], fig) for k, fig, _ in ran)))
        assert len(ran) == sum(op[0] == "check" for op in ops) == S.N_CHECKS, "no check is ever skipped"
        for k, fig, pred in ran:
            checks[k].append(fig)
            before.update(pred)
    print("slowest model-only seed: %.2f s; predecessors: %r" % (slowest, dict(before)))
    for k, ro in enumerate(S.READ_OUTS):
        figs = checks[k]
        assert len(figs) >= 3, "%s is checked %d times" % (ro.name, len(figs))
        if ro.floor is not None:
            good = sum(S.nontrivial(ro, f) for f in figs)
            assert 2 * good >= len(figs), "%s: %d of %d checks see more than %d %s: %r" % (ro.name, good, len(figs), ro.floor, ro.unit, figs)
    for kind in S.PREDECESSORS:
        assert before[kind] >= 3, "%s stands directly before a check %d times" % (kind, before[kind])
    # every form of every operation is drawn somewhere
    for kind in S.HOST_KINDS + S.BATCH_KINDS:
        assert ops_seen[("integrate", kind)] >= 1, kind
    for need in (("clear",), ("show_all",), ("mark",), ("restore",), ("handoff",), ("hide_list", "hide"), ("hide_list", "show"), ("hide_list", "hide_others"),
                 ("hide_box", "hide"), ("hide_box", "show"), ("hide_box", "hide_others")):
        assert ops_seen[need] >= 1, need


def test_every_state_of_the_matrix_has_something_to_show(oracle_mod, x):
    """The states the GPU matrix builds, on the model: a read-out's figure is above its floor in every state, and only the last state
    has a hidden set at the read-out.  (The mesh and the rays, the two slow restatements, are left to the GPU test, which asserts the
    same floor in every case.)"""
    for state in S.STATES:
        assert S.model_key(S.state_ops(state, 0)) == S.model_key(S.state_ops(state, 1)), "the forms of a state's calls do not change its model"
        m = _model(oracle_mod, x, S.state_ops(state, 0))
        figs = {ro.name: S.model_figure(ro, m, x) for ro in S.READ_OUTS if ro.name not in ("extract_mesh", "raycast_view")}
        print("%s: %d rows, %r" % (state, len(m.rows()), figs))
        for ro in S.READ_OUTS:
            assert ro.floor is None or ro.name not in figs or figs[ro.name] > ro.floor, "%s, %s: %d %s" % (state, ro.name, figs[ro.name], ro.unit)
        assert (figs["get_hidden"] > 1000) == (state == "rollback_to_hidden") and len(m.rows()) > 1000, "%s: %d hidden, %d rows" % (state, figs["get_hidden"], len(m.rows()))
        m.close()
