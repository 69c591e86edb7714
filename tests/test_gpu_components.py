"""GPU: connected components of the fused model and the speck filter (hfpf_extract_components, hfpf_extract_components_device).
The call is defined on the rows hfpf_extract_filtered returns, so rows, labels and component records are compared byte for byte with
tests/components_ref.py run on those.  The shared session is the synthetic depth stream of the query tests plus two flat patches
integrated as clouds well clear of the surface: the specks."""
import ctypes as C

import numpy as np
import pytest

import components_ref as CR
import scenes
from gpu_support import PATCH_CELLS, add_patches, components_device, counters, grid, in_boxes, run, same_components, two_handles, unchanged
from scenes import DepthScene

pytestmark = pytest.mark.gpu
# (reach, min_count, min_normal_dot, min_rows, min_points, keep_largest); min_rows "specks" = between the patches and the surface
OPTION_SETS = [(1, 0.0, -2.0, 0, 0, 0), (2, 0.0, 0.0, 0, 0, 0), (3, 3.0, 0.9, 0, 0, 0), (4, 0.0, -2.0, 0, 0, 0), (1, 0.0, -2.0, "specks", 0, 0),
               (1, 0.0, 0.9, 0, 500, 3), (2, 2.0, -2.0, 0, 0, 1), (1, 0.0, 0.0, 2, 40, 0)]


def _opts(opt, specks):
    reach, min_count, dot, min_rows, min_points, keep = opt
    return dict(reach=reach, min_count=min_count, min_normal_dot=dot, min_rows=specks if min_rows == "specks" else min_rows,
                min_points=min_points, keep_largest=keep)


@pytest.fixture(scope="module")
def session(hfpf_mod, synth_mod):
    sc = DepthScene(12, 640, 480, clean_every=4)
    g = grid(hfpf_mod)
    run(g, sc)
    boxes = add_patches(g)
    rows = g.extract().copy()
    # the scene as the reference sees it: the patches are components of their own, the surface has one at least 100 times larger
    ref = CR.components(rows, reach=1)
    patch = in_boxes(rows, boxes)
    patch_comps = np.unique(ref[1][patch])
    sizes = ref[2]["n_rows"]
    print("session: %d rows, %d of them on the patches; reach 1: %d components, largest %d, patch components %s" % (
        len(rows), patch.sum(), len(sizes), sizes.max(), sizes[patch_comps]))
    assert patch.sum() >= 2 * (PATCH_CELLS - 4) ** 2, "the patches' interiors should hold rows"
    assert not np.isin(ref[1][~patch], patch_comps).any(), "a patch shares a component with the surface"
    assert len(patch_comps) >= 2 and sizes.max() >= 100 * sizes[patch_comps].max()
    specks = int(sizes[patch_comps].max()) + 1  # min_rows between the patches' size and the main component's
    assert specks < sizes.max()
    yield sc, g, rows, boxes, specks
    g.close()


# ---- 1. byte-exact against the numpy contract ------------------------------------------------------------------------

@pytest.mark.parametrize("opt", OPTION_SETS, ids=["r%d_mc%g_dot%g_rows%s_pts%d_keep%d" % o for o in OPTION_SETS])
def test_byte_exact_against_components_ref(hfpf_mod, session, opt):
    sc, g, rows, boxes, specks = session
    kw = _opts(opt, specks)
    gated = g.extract_filtered(kw["min_count"])
    assert gated.tobytes() == rows[CR.count_gate(rows, kw["min_count"])].tobytes()
    ref = CR.components(gated, **dict(kw, min_count=0.0))
    got = g.extract_components(**kw)
    print("%s: %d rows in, %d rows / %d components out, largest %d" % (kw, len(gated), len(got[0]), len(got[2]),
                                                                    got[2]["n_rows"].max() if len(got[2]) else 0))
    same_components(got, ref, str(kw))
    assert len(got[2]) >= 1 and not got[2]["reserved"].any()
    if kw["keep_largest"]:
        assert len(got[2]) <= kw["keep_largest"]


# ---- 2. forms --------------------------------------------------------------------------------------------------------

def test_host_and_device_forms_agree_and_rows_are_optional(hfpf_mod, session):
    sc, g, rows, boxes, specks = session
    for kw in (dict(reach=1), dict(reach=2, min_normal_dot=0.9, min_rows=specks), dict(reach=1, min_count=2.0, keep_largest=3)):
        host = g.extract_components(**kw)
        same_components(components_device(g, hfpf_mod, **kw), host, "device form %s" % kw)
        no_rows = g.extract_components(rows=False, **kw)
        assert no_rows[0] is None
        same_components(no_rows, (None,) + host[1:], "rows = NULL %s" % kw)
        r, l, nr, c, nc = g.extract_components(device=True, rows=False, **kw)
        try:
            assert r == 0 and nr == len(host[1]) and nc == len(host[2])
            assert g.device_download(l, nr * 4).tobytes() == host[1].tobytes() and g.device_download(c, nc * 48).tobytes() == host[2].tobytes()
        finally:
            g.device_free(l), g.device_free(c)
    full = g.extract_components()
    assert full[0].tobytes() == rows.tobytes(), "with every filter off the rows are hfpf_extract's"


# ---- 3. the speck filter ---------------------------------------------------------------------------------------------

def test_min_rows_removes_exactly_the_patches(hfpf_mod, session):
    """min_rows between the patches' size and the main component's, both as the reference reports them.  At reach 1 the synthetic
    surface itself sheds a few pieces smaller than a patch (a property of the scene), and they go with the patches; the test also
    runs at the smallest reach at which the reference finds nothing that small but the patches, where the kept rows are exactly the
    unfiltered rows minus the patch rows."""
    sc, g, rows, boxes, specks = session
    patch = in_boxes(rows, boxes)
    exact_at = None
    for reach in (1, 2, 3, 4):
        ref = CR.components(rows, reach=reach)
        sizes = ref[2]["n_rows"]
        main, patch_size = int(sizes.max()), int(sizes[np.unique(ref[1][patch])].max())
        assert patch_size < main
        min_rows = patch_size + 1
        small = np.isin(ref[1], np.flatnonzero(sizes < min_rows))
        assert small[patch].all()
        print("reach %d: main %d, patches %d, %d other rows in components below min_rows" % (reach, main, patch_size, (small & ~patch).sum()))
        kept, labels, comps = g.extract_components(reach=reach, min_rows=min_rows)
        assert kept.tobytes() == rows[~small].tobytes()
        assert not in_boxes(kept, boxes).any() and comps["n_rows"].min() >= min_rows and comps["n_rows"].max() == main
        if exact_at is None and (small == patch).all():
            exact_at = reach
            assert kept.tobytes() == rows[~patch].tobytes(), "the kept rows are the unfiltered rows minus the patch rows"
    assert exact_at is not None, "at no reach are the patches the only small components of this scene"


# ---- 4. no side effects ----------------------------------------------------------------------------------------------

def test_components_change_nothing(hfpf_mod, synth_mod):
    sc = DepthScene(10, 320, 240, clean_every=3)

    def look(g, i):
        g.extract_components(reach=1 + i % 4, min_normal_dot=(-2.0, 0.5)[i % 2], min_rows=i % 3, keep_largest=i % 2)

    with two_handles(hfpf_mod, sc, look, lambda b: b.extract_components()) as (a, b, rb):
        before = counters(b)
        one = b.extract_components(reach=2, min_normal_dot=0.5)
        two = b.extract_components(reach=2, min_normal_dot=0.5)
        same_components(one, two, "second call")
        same_components(one, CR.components(rb, reach=2, min_normal_dot=0.5), "components_ref")
        assert counters(b) == before
        unchanged(a, b, rb)
        # the same continuation on both handles
        for g in (a, b):
            sc.integrate(g, 0)
            g.clean()
        assert a.extract().tobytes() == b.extract().tobytes() and counters(a) == counters(b)


# ---- 5. scheduling independence --------------------------------------------------------------------------------------

def test_direct_update_and_restored_handles_give_the_same_components(hfpf_mod, session):
    sc, g, rows, boxes, specks = session
    cases = (dict(reach=1), dict(reach=2, min_normal_dot=0.9, min_rows=specks), dict(reach=3, min_count=2.0, keep_largest=2))
    want = [g.extract_components(**kw) for kw in cases]
    with grid(hfpf_mod, binned_update=False) as d:
        run(d, sc)
        add_patches(d)
        assert d.extract().tobytes() == rows.tobytes()
        for kw, w in zip(cases, want):
            same_components(d.extract_components(**kw), w, "HFPF_FLAG_DIRECT_UPDATE %s" % kw)
    blob = g.snapshot()
    with grid(hfpf_mod) as r:
        r.restore(blob)
        for kw, w in zip(cases, want):
            same_components(r.extract_components(**kw), w, "restored %s" % kw)
            same_components(components_device(r, hfpf_mod, **kw), w, "restored, device form %s" % kw)


# ---- 6. edges --------------------------------------------------------------------------------------------------------

def test_empty_and_uncleaned_handles_hold_no_components(hfpf_mod, synth_mod):
    sc = DepthScene(3, 320, 240, clean_every=0)
    with grid(hfpf_mod) as g:
        for form in (dict(), dict(rows=False)):
            out = g.extract_components(reach=4, **form)
            assert len(out[1]) == 0 and len(out[2]) == 0 and (out[0] is None or len(out[0]) == 0)
        assert g.extract_components(device=True) == (0, 0, 0, 0, 0)
        for f in range(sc.n_frames):  # integrated, never cleaned: cells are occupied, no row exists
            sc.integrate(g, f)
        out = g.extract_components(reach=2)
        assert len(out[0]) == 0 and len(out[1]) == 0 and len(out[2]) == 0
        assert g.extract_components(device=True, reach=2) == (0, 0, 0, 0, 0)
        g.clean()
        out = g.extract_components(min_count=1e9)  # a gate no row passes
        assert len(out[0]) == 0 and len(out[2]) == 0
        assert len(g.extract_components(min_rows=1 << 30)[2]) == 0  # rows, but no component is kept
        same_components(g.extract_components(reach=2), CR.components(g.extract(), reach=2), "after the first clean")


def test_bad_arguments_are_refused_and_the_handle_stays_usable(hfpf_mod, synth_mod):
    H_ = hfpf_mod
    L = H_.lib()
    sc = DepthScene(6, 160, 120, clean_every=3)
    nan, inf = float("nan"), float("inf")
    bad = [("struct_size", C.sizeof(H_.ComponentOpts) - 8), ("flags", 1), ("reserved0", 1), ("reserved", 1), ("reach", 0), ("reach", 5),
           ("min_count", nan), ("min_normal_dot", nan), ("min_normal_dot", inf), ("min_normal_dot", -2.5), ("min_normal_dot", 1.25)]
    with grid(hfpf_mod) as g:
        run(g, sc)
        want = g.extract().copy()
        ref = g.extract_components(reach=2)
        r, l, c = C.c_void_p(1), C.c_void_p(2), C.c_void_p(3)
        nr, nc = C.c_uint64(7), C.c_uint64(8)

        def calls(o, rp=C.byref(r), lp=C.byref(l), nrp=C.byref(nr), cp=C.byref(c), ncp=C.byref(nc)):
            return [L.hfpf_extract_components(g._h, o, rp, lp, nrp, cp, ncp), L.hfpf_extract_components_device(g._h, o, rp, lp, nrp, cp, ncp)]

        for field, val in bad:
            o = H_.component_opts()
            setattr(o, field, val)
            assert calls(C.byref(o)) == [-2, -2], (field, val)
        o = H_.component_opts()
        assert calls(None) == [-2, -2], "NULL opts"
        assert calls(C.byref(o), lp=None) == [-2, -2], "NULL labels"
        assert calls(C.byref(o), nrp=None) == [-2, -2], "NULL n_rows"
        assert calls(C.byref(o), cp=None) == [-2, -2], "NULL comps"
        assert calls(C.byref(o), ncp=None) == [-2, -2], "NULL n_comps"
        assert (r.value, l.value, c.value, nr.value, nc.value) == (1, 2, 3, 7, 8), "a refused call wrote its outputs"
        assert g.extract().tobytes() == want.tobytes()
        same_components(g.extract_components(reach=2), ref, "after the refusals")
        same_components(ref, CR.components(want, reach=2), "components_ref")


def test_rccl_and_failed_handles_are_refused(hfpf_mod, synth_mod):
    sc = scenes.Scene(2, 160, 120, 0.001, fx=615.0)
    with hfpf_mod.OccupancyGrid(resolution=sc.resolution, bbox=sc.bbox, max_bricks=60000, max_log_points=1 << 20, max_normals=1 << 16,
                                max_frames=8) as g:
        g.dist_init_rccl(0, 1, hfpf_mod.dist_unique_id())
        g.integrate(sc.frame(0), sc.poses[0])
        g.clean()
        for form in (dict(), dict(device=True)):
            with pytest.raises(hfpf_mod.HfpfError) as e:
                g.extract_components(**form)
            assert e.value.code == -5
        g.dist_disable()
        assert len(g.extract_components()[0]) == len(g.extract()) > 0
    with hfpf_mod.OccupancyGrid(resolution=sc.resolution, bbox=sc.bbox, max_bricks=60000, max_log_points=1 << 20, max_normals=64,
                                max_frames=8) as g:
        g.integrate(sc.frame(0), sc.poses[0])
        with pytest.raises(hfpf_mod.HfpfError) as e:
            g.clean()
        assert e.value.code == -3
        for form in (dict(), dict(device=True)):
            with pytest.raises(hfpf_mod.HfpfError) as e:
                g.extract_components(**form)
            assert e.value.code == -5
        g.clear()
        assert len(g.extract_components()[2]) == 0


def test_kernel_time_id_6_counts_the_calls(hfpf_mod, session):
    sc, g, rows, boxes, specks = session
    g.kernel_timing(1)
    try:
        g.extract_components(reach=1)
        g.extract_components(device=True, rows=False, min_rows=1 << 30)
        ms, n = g.kernel_time(6)
        assert n == 2 and ms > 0.0
    finally:
        g.kernel_timing(0)
