"""GPU: querying the fused model at given points (hfpf_query, hfpf_query_device, hfpf_query_depth).  A query is defined on the rows
hfpf_extract returns and the cells hfpf_get_occupied lists, so every hit and row is compared byte for byte with tests/query_ref.py
run on those."""
import ctypes as C

import numpy as np
import pytest

import depth_ref
import query_ref as Q
from gpu_support import IDENT, Z_CLIP, grid, held_out, run, same_planes, same_query, two_handles, unchanged, uploaded
from scenes import DepthScene

pytestmark = pytest.mark.gpu
INF = float("inf")
# (radius, min_count, max_distance, zclip): every radius, a count gate, a distance gate, both z-clip settings
OPTION_SETS = [(0, 0.0, INF, False), (1, 0.0, INF, True), (2, 3.0, 0.003, False), (4, 0.0, INF, True), (1, 2.0, 0.0015, False)]


def _bbox(g):
    return tuple(g.cfg.bbox)


def _ref(g, rows, occ, pts, pose, radius, min_count, max_distance, zclip):
    return Q.query(rows, occ, pts, pose, _bbox(g), g.dims[1], Z_CLIP, radius=radius, min_count=min_count, max_distance=max_distance,
                   zclip=zclip)


def _point_sets(synth_mod, g, rows):
    """(label, points (N, 3) f32, pose, depth image or None) of the three sets."""
    depth, K, pose = held_out(synth_mod)
    rng = np.random.default_rng(0x9E7)
    b = np.asarray(_bbox(g))
    span = b[1::2] - b[0::2]
    rand = rng.uniform(b[0::2] - 0.05 * span, b[1::2] + 0.05 * span, (100000, 3)).astype(np.float32)
    live = rows[rows["count"] > 0]
    xyz = np.stack([live["x"], live["y"], live["z"]], axis=1).astype(np.float32)
    jit = (xyz + rng.normal(0.0, 0.002, xyz.shape)).astype(np.float32)
    return [("held-out depth frame", Q.depth_points(depth, K), pose, (depth, K)), ("random in and around the bbox", rand, IDENT, None),
            ("jittered row centroids", jit, IDENT, None)]


@pytest.fixture(scope="module")
def session(hfpf_mod, synth_mod):
    sc = DepthScene(12, 640, 480, clean_every=4)
    g = grid(hfpf_mod)
    run(g, sc)
    rows = g.extract().copy()
    occ = g.occupied()
    yield sc, g, rows, occ
    g.close()


# ---- 1. bit-exact against the numpy contract -------------------------------------------------------------------------

@pytest.mark.parametrize("opt", OPTION_SETS, ids=["r%d_mc%g_md%g_z%d" % (o[0], o[1], o[2], o[3]) for o in OPTION_SETS])
def test_bit_exact_against_query_ref(hfpf_mod, synth_mod, session, opt):
    sc, g, rows, occ = session
    radius, min_count, max_distance, zclip = opt
    kw = dict(radius=radius, min_count=min_count, max_distance=max_distance, zclip=zclip)
    for label, pts, pose, img in _point_sets(synth_mod, g, rows):
        got = g.query_depth(img[0], pose, img[1], **kw) if img is not None else g.query(pts, pose, **kw)
        ref = _ref(g, rows, occ, pts, pose, **kw)
        flags = got[0]["flags"]
        print("%s, %s: %d points, %d used, %d in bbox, %d occupied, %d has_row, %d found" % (
            label, opt, len(pts), (flags & Q.USED != 0).sum(), (flags & Q.IN_BBOX != 0).sum(), (flags & Q.OCCUPIED != 0).sum(),
            (flags & Q.HAS_ROW != 0).sum(), (flags & Q.FOUND != 0).sum()))
        same_query(got, ref, "%s, %s" % (label, opt))
        assert (flags & Q.FOUND != 0).sum() > (20 if img is None and label.startswith("random") else 10000)


# ---- 2. agreement with integrate ------------------------------------------------------------------------------------

def test_a_frame_queried_after_its_integrate_lands_in_occupied_cells(hfpf_mod, synth_mod):
    sc = DepthScene(6, 640, 480, clean_every=3)
    depth, K, pose = held_out(synth_mod)
    with grid(hfpf_mod) as g:
        run(g, sc)
        g.integrate_depth(depth, pose, K)  # a host frame: the query launches it first
        hits, _ = g.query_depth(depth, pose, K, radius=1, zclip=True, rows=False)
        f = hits["flags"]
        inside = (f & Q.USED != 0) & (f & Q.IN_BBOX != 0)
        assert inside.sum() > 100000
        assert (f[inside] & Q.OCCUPIED != 0).all()
        pts = Q.depth_points(depth, K)
        q, idx, pflags = g.probe_points(pose, pts)
        used = f & Q.USED != 0
        assert np.array_equal(used, (pflags & 1) != 0)
        assert np.array_equal(inside, (pflags & 3) == 3)
        assert hits["voxel"][used].tobytes() == idx[used].tobytes()
        assert hits["p"][used].tobytes() == q[used].tobytes()
        same_query((hits, None), (_ref(g, g.extract(), g.occupied(), pts, pose, 1, 0.0, INF, True)[0], None), "after integrate")


# ---- 3. equivalent inputs -------------------------------------------------------------------------------------------

def test_host_cloud_device_cloud_and_depth_forms_agree(hfpf_mod, synth_mod, session):
    sc, g, rows, occ = session
    depth, K, pose = held_out(synth_mod)
    kw = dict(radius=2, min_count=2.0, zclip=True)
    a = g.query_depth(depth, pose, K, **kw)
    cloud = depth_ref.packed_cloud(depth, K)  # 16-byte records: the packed form
    layout16 = dict(point_step=16, off_x=0, off_y=4, off_z=8)
    b = g.query(cloud, pose, layout=layout16, **kw)
    c = g.query(Q.depth_points(depth, K), pose, **kw)  # 12-byte records: the strided form
    with uploaded(g, cloud) as (dev,):
        d = g.query_device(dev, len(cloud) // 16, pose, layout=layout16, **kw)
        e = g.query_device(dev, len(cloud) // 16 - 1, pose, layout=dict(point_step=16, off_x=8, off_y=4, off_z=0), **kw)  # strided
    for what, x in (("host packed cloud", b), ("host strided cloud", c), ("device packed cloud", d)):
        same_query(x, a, what)
    assert (a[0]["flags"] & Q.FOUND != 0).sum() > 100000
    # x and z swapped: the same as a host cloud with that layout
    same_query(e, g.query(cloud[:len(cloud) - 16], pose, layout=dict(point_step=16, off_x=8, off_y=4, off_z=0), **kw), "swapped axes")
    # without rows, the hits are those of a call with rows
    h, r = g.query_depth(depth, pose, K, rows=False, **kw)
    assert r is None and h.tobytes() == a[0].tobytes()
    h, r = g.query(cloud, pose, layout=layout16, rows=False, **kw)
    assert r is None and h.tobytes() == a[0].tobytes()


# ---- 4. no side effects ---------------------------------------------------------------------------------------------

def test_queries_change_nothing(hfpf_mod, synth_mod):
    sc = DepthScene(10, 320, 240, clean_every=3)
    K = sc.K
    rng = np.random.default_rng(5)
    pts = rng.uniform(-0.3, 0.3, (5000, 3)).astype(np.float32)
    pts[:, 2] += np.float32(0.45)

    def look(g, i):
        if i % 2 == 0:
            g.query(pts, sc.poses[i % sc.n_frames], radius=i % 5)
        else:
            g.query_depth(sc.frames[i % sc.n_frames][0], sc.poses[0], K, radius=1, zclip=True)

    with two_handles(hfpf_mod, sc, look, lambda b: b.query(pts, sc.poses[0])) as (a, b, rb):
        ia = a.render(sc.poses[2], K, sc.W, sc.H, z_range=(0.05, 3.0), splat_radius=2)
        same_planes(ia, b.render(sc.poses[2], K, sc.W, sc.H, z_range=(0.05, 3.0), splat_radius=2), "a render of both handles")
        one = b.query(pts, sc.poses[1], radius=2)
        two = b.query(pts, sc.poses[1], radius=2)
        same_query(one, two, "second query")
        same_query(one, _ref(b, rb, b.occupied(), pts, sc.poses[1], 2, 0.0, INF, False), "query_ref")
        unchanged(a, b, rb)


# ---- 5. edges -------------------------------------------------------------------------------------------------------

def test_empty_and_uncleaned_handles_find_nothing(hfpf_mod, synth_mod):
    sc = DepthScene(3, 320, 240, clean_every=0)
    depth, K = sc.frames[0][0], sc.K
    with grid(hfpf_mod) as g:
        hits, rows = g.query_depth(depth, sc.poses[0], K, radius=4)
        assert not (hits["flags"] & (Q.OCCUPIED | Q.HAS_ROW | Q.FOUND)).any() and (hits["flags"] & Q.IN_BBOX).any()
        assert (rows["ix"] == -1).all() and not rows["count"].any()
        for f in range(sc.n_frames):  # integrated, never cleaned: cells are occupied, no row exists
            sc.integrate(g, f)
        assert len(g.extract()) == 0
        pts = Q.depth_points(depth, K)
        got = g.query_depth(depth, sc.poses[0], K, radius=4, zclip=True)
        assert not (got[0]["flags"] & Q.FOUND).any() and (got[0]["flags"] & Q.OCCUPIED != 0).sum() > 10000
        same_query(got, _ref(g, g.extract(), g.occupied(), pts, sc.poses[0], 4, 0.0, INF, True), "before the first clean")


def test_bad_arguments_are_refused_and_the_handle_stays_usable(hfpf_mod, synth_mod):
    H_ = hfpf_mod
    sc = DepthScene(6, 160, 120, clean_every=3)
    with grid(hfpf_mod) as ref:
        run(ref, sc)
        want = ref.extract().copy()
    L = H_.lib()
    bad = {"struct_size": ("struct_size", C.sizeof(H_.QueryOpts) - 8), "flags": ("flags", 2), "reserved0": ("reserved0", 1),
           "reserved": ("reserved", 1), "radius -1": ("radius", -1), "radius 5": ("radius", 5), "min_count nan": ("min_count", float("nan")),
           "max_distance 0": ("max_distance", 0.0), "max_distance -1": ("max_distance", -1.0), "max_distance nan": ("max_distance", float("nan"))}
    pts = np.random.default_rng(1).uniform(-0.2, 0.2, (100, 3)).astype(np.float32)
    pts[:, 2] += np.float32(0.45)
    depth, K = sc.frames[0][0], sc.K
    d = H_._image_desc(depth, K, None, None, 0.001)
    n_px = sc.W * sc.H
    with grid(hfpf_mod) as g:
        for i, ev in enumerate(sc.schedule()):
            if ev[0] == "integrate":
                sc.integrate(g, ev[1])
            else:
                g.clean()
            if i != 2:
                continue
            pose = np.ascontiguousarray(sc.poses[0], np.float64).reshape(12)
            hits = np.zeros(n_px, H_.QUERY_HIT_DTYPE)
            rows = np.zeros(n_px, H_.ROW_DTYPE)
            hp, rp, pp, dp = hits.ctypes.data, rows.ctypes.data, pts.ctypes.data, depth.ctypes.data
            dev = g.device_alloc(n_px * 64 * 2 + 4096)
            try:
                g.device_upload(dev, np.zeros(2 * n_px * 64, np.uint8))
                g.device_upload(dev + 2 * n_px * 64, pts)
                dpts = dev + 2 * n_px * 64

                def calls(o, pose_p, hits_p=hp, desc=d):
                    return [L.hfpf_query(g._h, o, pp, 100, 12, 0, 4, 8, pose_p, hits_p, rp),
                            L.hfpf_query_device(g._h, o, dpts, 100, 12, 0, 4, 8, pose_p, dev if hits_p else None, dev + n_px * 64),
                            L.hfpf_query_depth(g._h, o, C.byref(desc), dp, pose_p, hits_p, rp)]

                for what, (field, val) in bad.items():
                    o = H_.query_opts()
                    setattr(o, field, val)
                    assert calls(C.byref(o), pose.ctypes.data) == [-2, -2, -2], what
                o = H_.query_opts()
                assert calls(None, pose.ctypes.data) == [-2, -2, -2], "NULL opts"
                assert calls(C.byref(o), None) == [-2, -2, -2], "NULL pose"
                for k, v in ((0, float("nan")), (5, float("inf"))):
                    p2 = pose.copy()
                    p2[k] = v
                    assert calls(C.byref(o), p2.ctypes.data) == [-2, -2, -2], "non-finite pose"
                assert calls(C.byref(o), pose.ctypes.data, hits_p=None) == [-2, -2, -2], "NULL hits"
                lay = [(12, 0, 4, 10), (14, 0, 4, 8), (12, 0, 4, 12), (8, 0, 4, 8)]  # unaligned offset / step, offsets beyond the step
                for step, ox, oy, oz in lay:
                    assert L.hfpf_query(g._h, C.byref(o), pp, 10, step, ox, oy, oz, pose.ctypes.data, hp, rp) == -2, (step, ox, oy, oz)
                    assert L.hfpf_query_device(g._h, C.byref(o), dpts, 10, step, ox, oy, oz, pose.ctypes.data, dev, None) == -2
                assert L.hfpf_query(g._h, C.byref(o), None, 10, 12, 0, 4, 8, pose.ctypes.data, hp, rp) == -2, "NULL cloud"
                assert L.hfpf_query_device(g._h, C.byref(o), dpts + 2, 10, 12, 0, 4, 8, pose.ctypes.data, dev, None) == -2, "unaligned cloud"
                assert L.hfpf_query_device(g._h, C.byref(o), dpts, 10, 12, 0, 4, 8, pose.ctypes.data, dev + 4, None) == -2, "unaligned hits"
                assert L.hfpf_query_device(g._h, C.byref(o), dpts, 10, 12, 0, 4, 8, pose.ctypes.data, dev, dev + 8) == -2, "unaligned rows"
                for field, val in (("struct_size", 8), ("width", 0), ("depth_format", 7), ("fx", 0.0), ("depth_step", 2), ("reserved", 1),
                                   ("color_format", H_.COLOR_RGB8)):
                    d2 = H_._image_desc(depth, K, None, None, 0.001)
                    setattr(d2, field, val)
                    assert L.hfpf_query_depth(g._h, C.byref(o), C.byref(d2), dp, pose.ctypes.data, hp, rp) == -2, field
                assert L.hfpf_query_depth(g._h, C.byref(o), C.byref(d), None, pose.ctypes.data, hp, rp) == -2, "NULL depth"
                assert not hits.view(np.uint8).any() and not rows.view(np.uint8).any(), "a refused call wrote its output"
                assert not g.device_download(dev, 2 * n_px * 64).any(), "a refused call wrote its device output"
                # n_points = 0: nothing is read or written
                assert L.hfpf_query(g._h, C.byref(o), None, 0, 12, 0, 4, 8, pose.ctypes.data, None, None) == 0
                assert L.hfpf_query_device(g._h, C.byref(o), None, 0, 12, 0, 4, 8, pose.ctypes.data, None, None) == 0
                assert L.hfpf_query(g._h, C.byref(o), pp, 0, 12, 0, 4, 8, pose.ctypes.data, hp, rp) == 0
                assert not hits.view(np.uint8).any() and not rows.view(np.uint8).any()
                h0, r0 = g.query(np.zeros((0, 3), np.float32), pose)
                assert len(h0) == 0 and len(r0) == 0
            finally:
                g.device_free(dev)
        assert g.extract().tobytes() == want.tobytes()
        occ = g.occupied()
        same_query(g.query(pts, sc.poses[0], radius=2), _ref(g, want, occ, pts, sc.poses[0], 2, 0.0, INF, False), "after the refusals")


def test_a_cloud_of_several_chunks_is_exact(hfpf_mod, synth_mod, session):
    sc, g, rows, occ = session
    rng = np.random.default_rng(0xC4)
    live = rows[rows["count"] > 0]
    xyz = np.stack([live["x"], live["y"], live["z"]], axis=1).astype(np.float32)
    n = (1 << 20) * 2 + 12345  # three chunks of the host forms
    pts = (xyz[rng.integers(0, len(xyz), n)] + rng.normal(0.0, 0.003, (n, 3))).astype(np.float32)
    got = g.query(pts, IDENT, radius=1, min_count=2.0)
    same_query(got, _ref(g, rows, occ, pts, IDENT, 1, 2.0, INF, False), "three chunks")
    assert (got[0]["flags"] & Q.FOUND != 0).sum() > n // 2
