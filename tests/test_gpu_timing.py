"""GPU: what hfpf_kernel_timing / hfpf_get_kernel_time count (include/hfpf.h): which calls each id brackets, that enabling zeroes
every sum and count, that a read settles the pending event pairs first, and that nothing is filed while timing is off.  The scene
is the synthetic depth stream of the render tests, 4 frames of 160 x 120 with one clean pass: the counts do not depend on its size.
An id outside 0..7 is HFPF_ERR_BAD_ARG, which include/hfpf.h numbers -2."""
import numpy as np
import pytest

from gpu_support import IDENT, grid, run
from scenes import DepthScene

pytestmark = pytest.mark.gpu
W, H = 160, 120
QUAD = np.array([[-3, -3, 0], [3, -3, 0], [3, 3, 0], [-3, 3, 0]], np.float32)
QUAD_TRIS = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


def _free(g, *ptrs):
    for p in ptrs:
        if p:
            g.device_free(p)


def _components_device(g, **kw):
    r, l, nr, c, nc = g.extract_components(device=True, **kw)
    _free(g, r, l, c)
    return nr, nc


def _compare(g, rows):
    """One hfpf_compare_mesh call: a quad through the middle of the model."""
    c = np.array([np.median(rows[k]) for k in ("x", "y", "z")], np.float64)
    return g.compare_mesh(QUAD, QUAD_TRIS, np.hstack([np.eye(3), c.reshape(3, 1)]), max_distance=4 * g.dims[1])


def _rays(rows, n=64):
    """n rays along -normal towards the first n live rows, from 5 cm in front of them."""
    live = rows[rows["count"] > 0][:n]
    c = np.stack([live["x"], live["y"], live["z"]], axis=1).astype(np.float64)
    d = np.stack([live["nx"], live["ny"], live["nz"]], axis=1).astype(np.float64)
    return np.hstack([c + 0.05 * d, -d]).astype(np.float32)


@pytest.fixture(scope="module")
def session(hfpf_mod, synth_mod):
    sc = DepthScene(4, W, H, clean_every=4)
    g = grid(hfpf_mod)
    run(g, sc)
    rows = g.extract().copy()
    assert len(rows) > 0
    # two more frames of the same stream as packed clouds in HBM, for hfpf_integrate_device
    poses = np.stack([synth_mod.pose(0x5E3, 4 + f) for f in range(2)])
    clouds = np.concatenate([synth_mod.frame(0xD3F7, 4 + f, W, H, poses[f]) for f in range(2)])
    dev = g.device_alloc(clouds.nbytes)
    g.device_upload(dev, clouds)
    yield g, rows, dev, poses
    g.device_free(dev)
    g.close()


def _integrate(g, dev, poses):
    g.integrate_device(dev, 2, W * H * 16, W * H, poses.reshape(2, 12))


def test_each_id_counts_its_calls(hfpf_mod, session):
    g, rows, dev, poses = session
    assert len(g.extract()) > 0
    g.kernel_timing(1)
    try:
        for _ in range(3):
            g.clean()
        g.extract_components(reach=1)
        _components_device(g, rows=False)
        g.extract_components(rows=False, reach=2)
        _components_device(g, reach=1)
        for _ in range(2):
            _compare(g, rows)
        for _ in range(3):
            assert len(g.raycast(_rays(rows), IDENT)) == 64
        _integrate(g, dev, poses)
        times = {k: g.kernel_time(k) for k in range(8)}
        print("kernel times:", times)
        assert times[1][1] == 3 and times[6][1] == 4 and times[7][1] == 2 and times[5][1] == 3
        assert times[0][1] >= 1
        assert all(n == 0 for k, (ms, n) in times.items() if k in (2, 3, 4)), "detail ids are off at level 1"
        assert all(ms > 0.0 for ms, n in times.values() if n > 0)
        assert all(ms == 0.0 for ms, n in times.values() if n == 0)
        # a second read finds nothing pending and reports the same
        assert {k: g.kernel_time(k) for k in range(8)} == times
        # enabling again zeroes every sum and count
        g.kernel_timing(1)
        assert all(g.kernel_time(k) == (0.0, 0) for k in range(8))
    finally:
        g.kernel_timing(0)
        g.clean()


def test_detail_ids_of_an_integrate_call(hfpf_mod, session):
    g, rows, dev, poses = session
    g.kernel_timing(2)
    try:
        _integrate(g, dev, poses)
        t = {k: g.kernel_time(k) for k in range(5)}
        print("kernel times:", t)
        assert t[0][1] >= 1 and t[2][1] >= 1
        assert t[3][1] <= t[2][1] and t[4][1] <= t[2][1]
        assert all(ms > 0.0 for ms, n in t.values() if n > 0)
        g.kernel_timing(2)
        assert all(g.kernel_time(k) == (0.0, 0) for k in range(8))
    finally:
        g.kernel_timing(0)
        g.clean()


def test_bad_ids_leave_the_handle_usable(hfpf_mod, session):
    g, rows, dev, poses = session
    want = g.extract().tobytes()
    g.kernel_timing(1)
    try:
        for bad in (8, -1):
            with pytest.raises(hfpf_mod.HfpfError) as e:
                g.kernel_time(bad)
            assert e.value.code == -2  # HFPF_ERR_BAD_ARG
        g.extract_components(reach=1)
        assert g.kernel_time(6)[1] == 1
        assert g.extract().tobytes() == want
    finally:
        g.kernel_timing(0)


def test_nothing_is_filed_while_timing_is_off(hfpf_mod, session):
    g, rows, dev, poses = session
    g.kernel_timing(0)
    g.extract_components(reach=1)
    _compare(g, rows)
    g.kernel_timing(1)
    try:
        assert g.kernel_time(6) == (0.0, 0) and g.kernel_time(7) == (0.0, 0)
    finally:
        g.kernel_timing(0)


def test_early_exits_count_only_the_calls_that_reached_the_bracket(hfpf_mod, synth_mod):
    """hfpf_extract_components that keeps nothing leaves through its nk == 0 exit, behind the bracket's start: it counts.  On a cleared
    handle the call returns with no rows, in front of the bracket: it does not."""
    sc = DepthScene(4, W, H, clean_every=4)
    with grid(hfpf_mod) as g:
        run(g, sc)
        assert len(g.extract()) > 0
        g.kernel_timing(1)
        for form in (False, True):
            if form:
                assert _components_device(g, min_rows=1 << 30) == (0, 0)
            else:
                out, labels, comps = g.extract_components(min_rows=1 << 30)
                assert len(out) == len(labels) == len(comps) == 0
        assert len(g.extract_components(reach=1)[2]) > 0
        ms, n = g.kernel_time(6)
        assert n == 3 and ms > 0.0
        g.clear()
        for form in (False, True):
            if form:
                assert _components_device(g) == (0, 0)
            else:
                assert len(g.extract_components()[2]) == 0
        assert g.kernel_time(6) == (ms, 3)
