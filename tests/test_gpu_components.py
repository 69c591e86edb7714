"""GPU: connected components of the fused model and the speck filter (hfpf_extract_components, hfpf_extract_components_device).
The call is defined on the rows hfpf_extract_filtered returns, so rows, labels and component records are compared byte for byte with
tests/components_ref.py run on those.  The shared session is the synthetic depth stream of the query tests plus two flat patches
integrated as clouds well clear of the surface: the specks."""
import ctypes as C

import numpy as np
import pytest

import components_ref as CR
import scenes
from test_gpu_render import BBOX, RES, DepthScene, _counters, _grid, _run

pytestmark = pytest.mark.gpu
PATCH_CELLS = 15         # a patch is PATCH_CELLS x PATCH_CELLS voxels, one voxel thick; its interior passes the gate of 20 neighbours
PATCH_CLEAR = 0.08       # metres between a patch's centre and the nearest occupied voxel (Chebyshev): 0.05 clear of its rim
PATCH_DEPTH = 0.4        # camera-frame z of a patch's points (inside the default z-clip 0.28 .. 0.6)
# (reach, min_count, min_normal_dot, min_rows, min_points, keep_largest); min_rows "specks" = between the patches and the surface
OPTION_SETS = [(1, 0.0, -2.0, 0, 0, 0), (2, 0.0, 0.0, 0, 0, 0), (3, 3.0, 0.9, 0, 0, 0), (4, 0.0, -2.0, 0, 0, 0), (1, 0.0, -2.0, "specks", 0, 0),
               (1, 0.0, 0.9, 0, 500, 3), (2, 2.0, -2.0, 0, 0, 1), (1, 0.0, 0.0, 2, 40, 0)]


def free_spots(occ, bbox=BBOX, res=RES, clear=PATCH_CLEAR, cell=0.01):
    """Centres (fusion frame, voxel-centred in z) of two places at least `clear` (Chebyshev) from every occupied voxel and 0.1 m from
    the bounding box: the first and the last free cell of a 1 cm grid in lexicographic order."""
    lo = np.asarray(bbox, np.float64)[0::2]
    hi = np.asarray(bbox, np.float64)[1::2]
    n = np.round((hi - lo) / cell).astype(int)
    coarse = np.zeros(n, bool)
    c = np.clip(np.floor((np.asarray(occ, np.float64) + 0.5) * res / cell).astype(int), 0, n - 1)
    coarse[c[:, 0], c[:, 1], c[:, 2]] = True
    r = int(np.ceil(clear / cell)) + 1  # + 1: an occupied voxel may sit anywhere inside its coarse cell
    for axis in range(3):
        grown = coarse.copy()
        for s in range(1, r + 1):
            for sign in (1, -1):
                sh = np.roll(coarse, sign * s, axis=axis)
                idx = [slice(None)] * 3
                idx[axis] = slice(0, s) if sign == 1 else slice(n[axis] - s, None)
                sh[tuple(idx)] = False
                grown |= sh
        coarse = grown
    m = int(round(0.1 / cell))
    free = ~coarse
    inner = np.zeros_like(free)
    inner[m:n[0] - m, m:n[1] - m, m:n[2] - m] = True
    cells = np.argwhere(free & inner)
    assert len(cells) >= 2, "no room for the patches"
    spots = []
    for cc in (cells[0], cells[-1]):
        p = lo + (cc + 0.5) * cell
        p[2] = lo[2] + (np.floor((p[2] - lo[2]) / res) + 0.5) * res
        spots.append(p)
    assert np.abs(spots[0] - spots[1]).max() >= 0.1, "the two patches must be apart"
    return spots


def patch_cloud(centre, bbox=BBOX, res=RES, cells=PATCH_CELLS, per_cell=3):
    """(records, pose, voxel box) of one flat patch: per_cell^2 points in every voxel of a cells x cells square of the z-plane through
    `centre`, as packed 16-byte x, y, z, rgb records in the frame of a camera looking along +z from PATCH_DEPTH in front of it."""
    lo = np.asarray(bbox, np.float64)[0::2]
    v0 = np.floor((np.asarray(centre) - lo) / res).astype(int) - np.array([cells // 2, cells // 2, 0])
    t = (np.arange(cells * per_cell) + 0.5) / per_cell  # voxel units: no point on a voxel boundary
    u, v = np.meshgrid(t, t, indexing="ij")
    origin = lo + v0 * res  # the patch's low corner; z: the voxel's low face
    cam_t = np.array([origin[0], origin[1], origin[2] + 0.5 * res - PATCH_DEPTH])
    rec = np.zeros((u.size, 4), np.float32)
    rec[:, 0], rec[:, 1], rec[:, 2] = (u * res).ravel(), (v * res).ravel(), PATCH_DEPTH
    rec[:, 3] = np.array([0x00FF00FF], np.uint32).view(np.float32)[0]
    pose = np.hstack([np.eye(3), cam_t.reshape(3, 1)])
    box = (v0, v0 + np.array([cells - 1, cells - 1, 0]))
    return np.ascontiguousarray(rec), pose, box


def add_patches(g):
    """Integrates the two patches on top of what g holds and cleans; returns their voxel boxes."""
    boxes = []
    for centre in free_spots(g.occupied()):
        rec, pose, box = patch_cloud(centre)
        g.integrate(rec, pose)
        boxes.append(box)
    g.clean()
    return boxes


def in_boxes(rows, boxes):
    m = np.zeros(len(rows), bool)
    for lo, hi in boxes:
        m |= ((rows["ix"] >= lo[0]) & (rows["ix"] <= hi[0]) & (rows["iy"] >= lo[1]) & (rows["iy"] <= hi[1]) & (rows["iz"] >= lo[2]) &
              (rows["iz"] <= hi[2]))
    return m


def _same(got, ref, what):
    for x, y, name in zip(got, ref, ("rows", "labels", "comps")):
        if x is None and y is None:
            continue
        assert len(x) == len(y), "%s: %s: %d vs %d" % (what, name, len(x), len(y))
        a, b = np.ascontiguousarray(x).view(np.uint8).reshape(len(x), -1), np.ascontiguousarray(y).view(np.uint8).reshape(len(y), -1)
        bad = np.flatnonzero((a != b).any(axis=1))
        assert bad.size == 0, "%s: %s differ at %d of %d, first %d: %r vs %r" % (what, name, bad.size, len(x), bad[0], x[bad[0]], y[bad[0]])


def _device(g, H, **kw):
    """The device form, downloaded: (rows, labels, comps)."""
    r, l, nr, c, nc = g.extract_components(device=True, **kw)
    try:
        rows = g.device_download(r, nr * 64).view(H.ROW_DTYPE) if nr else np.zeros(0, H.ROW_DTYPE)
        labels = g.device_download(l, nr * 4).view(np.uint32) if nr else np.zeros(0, np.uint32)
        comps = g.device_download(c, nc * 48).view(H.COMPONENT_DTYPE) if nc else np.zeros(0, H.COMPONENT_DTYPE)
    finally:
        for p in (r, l, c):
            if p:
                g.device_free(p)
    return rows, labels, comps


def _opts(opt, specks):
    reach, min_count, dot, min_rows, min_points, keep = opt
    return dict(reach=reach, min_count=min_count, min_normal_dot=dot, min_rows=specks if min_rows == "specks" else min_rows,
                min_points=min_points, keep_largest=keep)


@pytest.fixture(scope="module")
def session(hfpf_mod, synth_mod):
    sc = DepthScene(12, 640, 480, clean_every=4)
    g = _grid(hfpf_mod)
    _run(g, sc)
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
    _same(got, ref, str(kw))
    assert len(got[2]) >= 1 and not got[2]["reserved"].any()
    if kw["keep_largest"]:
        assert len(got[2]) <= kw["keep_largest"]


# ---- 2. forms --------------------------------------------------------------------------------------------------------

def test_host_and_device_forms_agree_and_rows_are_optional(hfpf_mod, session):
    sc, g, rows, boxes, specks = session
    for kw in (dict(reach=1), dict(reach=2, min_normal_dot=0.9, min_rows=specks), dict(reach=1, min_count=2.0, keep_largest=3)):
        host = g.extract_components(**kw)
        _same(_device(g, hfpf_mod, **kw), host, "device form %s" % kw)
        no_rows = g.extract_components(rows=False, **kw)
        assert no_rows[0] is None
        _same(no_rows, (None,) + host[1:], "rows = NULL %s" % kw)
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

    with _grid(hfpf_mod) as a, _grid(hfpf_mod) as b:
        _run(a, sc)
        b.extract_components()  # on the empty handle
        _run(b, sc, between=look)
        ra, rb = a.extract(), b.extract()
        assert len(ra) > 0 and ra.tobytes() == rb.tobytes()
        assert _counters(a) == _counters(b)
        before = _counters(b)
        one = b.extract_components(reach=2, min_normal_dot=0.5)
        two = b.extract_components(reach=2, min_normal_dot=0.5)
        _same(one, two, "second call")
        _same(one, CR.components(rb, reach=2, min_normal_dot=0.5), "components_ref")
        assert _counters(b) == before and b.extract().tobytes() == ra.tobytes()
        # the same continuation on both handles
        for g in (a, b):
            sc.integrate(g, 0)
            g.clean()
        assert a.extract().tobytes() == b.extract().tobytes() and _counters(a) == _counters(b)


# ---- 5. scheduling independence --------------------------------------------------------------------------------------

def test_direct_update_and_restored_handles_give_the_same_components(hfpf_mod, session):
    sc, g, rows, boxes, specks = session
    cases = (dict(reach=1), dict(reach=2, min_normal_dot=0.9, min_rows=specks), dict(reach=3, min_count=2.0, keep_largest=2))
    want = [g.extract_components(**kw) for kw in cases]
    with _grid(hfpf_mod, binned_update=False) as d:
        _run(d, sc)
        add_patches(d)
        assert d.extract().tobytes() == rows.tobytes()
        for kw, w in zip(cases, want):
            _same(d.extract_components(**kw), w, "HFPF_FLAG_DIRECT_UPDATE %s" % kw)
    blob = g.snapshot()
    with _grid(hfpf_mod) as r:
        r.restore(blob)
        for kw, w in zip(cases, want):
            _same(r.extract_components(**kw), w, "restored %s" % kw)
            _same(_device(r, hfpf_mod, **kw), w, "restored, device form %s" % kw)


# ---- 6. edges --------------------------------------------------------------------------------------------------------

def test_empty_and_uncleaned_handles_hold_no_components(hfpf_mod, synth_mod):
    sc = DepthScene(3, 320, 240, clean_every=0)
    with _grid(hfpf_mod) as g:
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
        _same(g.extract_components(reach=2), CR.components(g.extract(), reach=2), "after the first clean")


def test_bad_arguments_are_refused_and_the_handle_stays_usable(hfpf_mod, synth_mod):
    H_ = hfpf_mod
    L = H_.lib()
    sc = DepthScene(6, 160, 120, clean_every=3)
    nan, inf = float("nan"), float("inf")
    bad = [("struct_size", C.sizeof(H_.ComponentOpts) - 8), ("flags", 1), ("reserved0", 1), ("reserved", 1), ("reach", 0), ("reach", 5),
           ("min_count", nan), ("min_normal_dot", nan), ("min_normal_dot", inf), ("min_normal_dot", -2.5), ("min_normal_dot", 1.25)]
    with _grid(hfpf_mod) as g:
        _run(g, sc)
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
        _same(g.extract_components(reach=2), ref, "after the refusals")
        _same(ref, CR.components(want, reach=2), "components_ref")


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
