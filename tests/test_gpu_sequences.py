"""GPU: every read-out against its restatement in the middle of a session (tests/sequence_support.py).  include/hfpf.h says of every
read-out that it sees "exactly the rows hfpf_extract would return at that point of the call sequence"; the tests of one read-out ask
it on a settled handle.  Here the read-out is the first call to meet what the sequence left behind: host frames waiting for their
launch, a device batch in flight, a clean pass that did not wait or whose front half ran beside the update kernel, a clear, a restore
to an earlier snapshot, the row set of another read-out.

A. The matrix: every read-out of the table in each of eight states built call by call.
B. Random sequences: one script per seed on the model, on a handle that takes the read-outs and on a twin that takes none; at the end
   the twin is the handle ("read-outs change nothing", over whole sequences).

A check is: the read-out; hfpf_extract and hfpf_get_occupied against the model (scenes.compare_rows, as the random-schedule tests);
the restatement on the engine's own rows, byte for byte.  160 x 120 frames, SMALL capacities, colour on."""
import os

import pytest

import gpu_support as G
import scenes
import sequence_support as S

pytestmark = pytest.mark.gpu

N_DEFAULT = 12
N_SEEDS = int(os.environ.get("HFPF_SOAK_SEEDS", str(N_DEFAULT)))  # raise for a soak run


@pytest.fixture(scope="module")
def x(synth_mod):
    return S.inputs()


# ---- A. state x read-out ---------------------------------------------------------------------------------------------------------------

_states = {}


def _state(oracle_mod, x, state, index):
    """(resolved operations, frozen model) of a state: the model is built once for all the read-outs that share it."""
    ops = S.state_ops(state, index)
    key = S.model_key(ops)
    if key not in _states:
        m = S.Model(oracle_mod, x)
        try:
            resolved = [S.resolve(op, m) for op in ops]
            frozen = m.frozen()
        finally:
            m.close()
        for a in (frozen.rows_, frozen.occupied_, frozen.hidden_):
            a.setflags(write=False)
        _states[key] = (resolved, frozen)
    resolved, frozen = _states[key]
    # the forms of this index's integrate calls on the shared model's operations
    return [mine if op[0] == "integrate" else (op[:2] + (mine[2],) + op[3:] if op[0] == "hide_list" else op) for op, mine in zip(resolved, ops)], frozen


@pytest.mark.parametrize("state", S.STATES)
@pytest.mark.parametrize("name", S.NAMES)
def test_state_x_read_out(oracle_mod, hfpf_mod, x, monkeypatch, capfd, state, name):
    k = S.NAMES.index(name)
    index = k + S.STATES.index(state)   # host and device forms, cloud and depth frames alternate over read-outs and states
    ro = S.READ_OUTS[k]
    ops, m = _state(oracle_mod, x, state, index)
    for v in G.FORM_VARIABLES:          # the forms a session takes by default
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("HFPF_TRACE_CLEAN", "1")
    capfd.readouterr()
    with S.Engine(hfpf_mod, x) as e:
        assert e.g.dims == (x.dims, x.res), "engine and oracle lay out one grid"
        for op in ops:
            S.engine_apply(op, e)
        if state == "after_previous_readout":  # another read-out, gated at 0: its row set is the larger one
            other = S.RESTATED[(k + 5) % len(S.RESTATED)]
            assert other.name != ro.name, "the read-out that runs first is another one"
            other.call(e, x, 0.0, not index & 1)
        figure, rows = S.check(ro, e, m, index, state)
        n_rows = len(rows)
        del rows
    cap = capfd.readouterr()
    print(cap.out, end="")
    lines, passes = G.clean_trace(cap.err)
    print("%s, %s (%s form): %d rows, %d %s; %s" % (state, name, "device" if index & 1 else "host", n_rows, figure, ro.unit, "; ".join(lines)))
    assert n_rows > 1000 and (ro.floor is None or figure > ro.floor), "%s, %s: %d rows, %d %s" % (state, name, n_rows, figure, ro.unit)
    assert (len(m.hidden()) > 1000) == (state == "rollback_to_hidden"), "%s: %d voxels hidden at the read-out" % (state, len(m.hidden()))
    if state in ("nowait_clean", "overlapped_clean"):
        assert len(passes) == sum(op[0] == "clean" for op in ops) == 2, "both passes of the state launched kernels: %r" % (lines,)
    if state == "nowait_clean":
        assert not passes[-1]["waited"] and passes[-1]["compacting"] == "no", "the pass before the read-out was to be a no-wait one: %r" % (passes[-1],)
    if state == "overlapped_clean":
        assert passes[-1]["beside"], "the front half of the pass before the read-out was to run beside the update kernel: %r" % (passes[-1],)


# ---- B. random sequences -----------------------------------------------------------------------------------------------------------------

_figures = {}   # seed -> [(read-out index, figure)]


def _run_seed(oracle_mod, hfpf_mod, x, seed):
    cfg, binned, fw = S.config_of(seed)
    ops = S.script(seed)
    print("seed %d: %r, binned %r, frame_width %d\n  %s" % (seed, cfg, binned, fw, "\n  ".join(repr(op) for op in ops)))
    m = S.Model(oracle_mod, x, **cfg)
    try:
        with S.Engine(hfpf_mod, x, binned, fw, **cfg) as a, S.Engine(hfpf_mod, x, binned, fw, **cfg) as b:
            def on_check(k, i):
                figure, rows = S.check(S.READ_OUTS[k], a, m, i, "seed %d, check %d" % (seed, i))
                print("seed %d, check %d: %s (%s form), %d rows, %d %s" % (seed, i, S.NAMES[k], "device" if i & 1 else "host", len(rows), figure, S.READ_OUTS[k].unit))
                return k, figure
            figs = S.run_script(ops, m, a, b, on_check)
            assert len(figs) == S.N_CHECKS, "no check is ever skipped"
            # the twin took every mutating operation and no read-out (nor a handoff): it is the handle
            ra, rb = a.g.extract(), b.g.extract()
            scenes.compare_rows(m.rows(), rb)
            assert ra.tobytes() == rb.tobytes(), "rows: the handle that was read and its twin differ"
            assert a.g.occupied().tobytes() == b.g.occupied().tobytes(), "occupied lists differ"
            assert a.g.hidden().tobytes() == b.g.hidden().tobytes() == m.hidden().tobytes(), "hidden sets differ"
            assert a.g.state_changed == b.g.state_changed == m.dirty(), "dirtiness differs"
            ca, cb = G.contract_counters(a.g), G.contract_counters(b.g)
            assert ca == cb, "contract counters: %r vs %r" % (ca, cb)
            # (a blob's size is a function of the session's counts, not of how the buffered points spread over the log's append regions)
            assert len(a.g.snapshot()) == len(b.g.snapshot()), "snapshot lengths differ"
    finally:
        m.close()
    return figs


@pytest.mark.parametrize("seed", list(range(N_SEEDS)))
def test_random_sequence(oracle_mod, hfpf_mod, x, seed):
    _figures[seed] = _run_seed(oracle_mod, hfpf_mod, x, seed)


def test_default_seeds_meet_the_floors(oracle_mod, hfpf_mod, x):
    """The floors test_sequence_model.py holds the scripts to on the oracle's rows, on the engine's: every read-out is checked at least
    three times over the default seeds, and at least half of its checks see more than its floor.  (Seeds that did not run in this
    session are run here.)"""
    per = {}
    for seed in range(N_DEFAULT):
        if seed not in _figures:
            _figures[seed] = _run_seed(oracle_mod, hfpf_mod, x, seed)
        for k, figure in _figures[seed]:
            per.setdefault(k, []).append(figure)
    for k, ro in enumerate(S.READ_OUTS):
        figs = per.get(k, [])
        print("%s: %r" % (ro.name, figs))
        assert len(figs) >= 3, "%s is checked %d times" % (ro.name, len(figs))
        if ro.floor is not None:
            good = sum(S.nontrivial(ro, f) for f in figs)
            assert 2 * good >= len(figs), "%s: %d of %d checks see more than %d %s: %r" % (ro.name, good, len(figs), ro.floor, ro.unit, figs)
