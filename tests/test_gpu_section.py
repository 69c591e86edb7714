"""GPU: planar sections of a triangle mesh (hfpf_section_mesh, hfpf_section_mesh_device).  The call is defined on its arguments alone,
so every point, segment, contour, plane record and summary is compared byte for byte with tests/section_ref.py: the contract is
exact, no tolerance is involved.  The meshes are the cube, the closed sphere and box of the plan tests, a seeded soup, the model's own
mesh of the cover tests' session (three 160 x 120 synthetic depth frames at 2 mm) and a strip that reaches the per-plane cap."""
import ctypes as C

import numpy as np
import pytest

import plan_support as PS
import section_ref as X
import section_support as S
from gpu_support import RES, counters, grid, run, uploaded
from scenes import DepthScene

pytestmark = pytest.mark.gpu
TINY = dict(max_bricks=2000, max_log_points=1 << 18, max_normals=1 << 14, max_frames=16)  # a handle that fuses nothing
BAD_ARG, CAPACITY = -2, -3
CUBE_V, CUBE_T = S.cube()


@pytest.fixture(scope="module")
def empty(hfpf_mod):
    """An empty handle with the default box: a section needs no fused model."""
    g = hfpf_mod.OccupancyGrid(resolution=RES, bbox=S.BBOX, **TINY)
    yield g
    g.close()


@pytest.fixture(scope="module")
def shapes():
    return PS.sphere_and_box()


def both(g, verts, tris, pose, planes, what, bbox=S.BBOX):
    """The host form against the reference; returns (got, ref)."""
    got = g.section_mesh(verts, tris, pose, planes)
    ref = S.reference(verts, tris, pose, planes, bbox)
    S.same_section(got, ref, what)
    S.consistent(*got)
    return got, ref


def device_form(g, H, verts, tris, pose, planes, stride=None):
    verts = np.ascontiguousarray(verts)
    stride = stride if stride is not None else (verts.dtype.itemsize if verts.dtype.names else 12)
    with uploaded(g, verts, tris) as (dv, dt):
        return S.section_device(g, H, dv, len(verts), stride, dt, len(tris), pose, planes)


# ---- 1. the cube --------------------------------------------------------------------------------------------------------------------

def test_cube_axis_plane_is_one_closed_unit_square(hfpf_mod, empty):
    (points, segments, contours, recs, s), _ = both(empty, CUBE_V, CUBE_T, S.IDENT, [[0, 0, 1, 0.25]], "cube, z = 0.25")
    assert (len(points), len(segments), len(contours)) == (8, 8, 1)
    assert contours[0]["flags"] == X.CLOSED and contours[0]["area_q28"] == S.Q28 and contours[0]["length_q32"] == 4 * S.Q32
    assert recs[0]["area_q28"] == S.Q28 and s["n_closed"] == 1 and s["n_tris_valid"] == 12


def test_cube_same_area_for_the_flipped_and_scaled_normal(hfpf_mod, empty):
    (_, _, contours, _, _), _ = both(empty, CUBE_V, CUBE_T, S.IDENT, [[0, 0, 1, 0.25], [0, 0, -2, -0.5]], "cube, n and -2n")
    assert len(contours) == 2 and (contours["area_q28"] == S.Q28).all() and (contours["flags"] == X.CLOSED).all()


def test_cube_diagonal_planes_and_a_plane_on_a_face(hfpf_mod, empty):
    planes = [[1, 1, 1, 0.5], [1, 1, 1, 1.0], [0, 0, 1, 0.0]]  # the hexagon, three corners exactly, the bottom face
    (points, segments, contours, recs, s), _ = both(empty, CUBE_V, CUBE_T, S.IDENT, planes, "cube, diagonal planes")
    assert recs["n_points"].tolist()[0] == 12 and recs["n_segments"].tolist()[0] == 12 and recs["n_contours"].tolist() == [1, 1, 0]
    assert (contours["flags"] == X.CLOSED).all() and recs[2].tobytes()[4:8] == bytes(4) and recs[2]["n_points"] == 0
    P = np.stack([points[k] for k in "xyz"], axis=1)
    on_corners = segments[points["plane"][segments["p0"]] == 1]
    assert (P[on_corners["p0"]] == P[on_corners["p1"]]).all(axis=1).any(), "zero-length segments are kept"


# ---- 2. the sphere and the box: chunks of 64 planes ---------------------------------------------------------------------------------

@pytest.mark.parametrize("planes", [S.parallel_planes(1), S.parallel_planes(64), S.parallel_planes(65), S.mixed_planes(65)], ids=["1", "64", "65", "mixed"])
def test_sphere_and_box_across_the_chunk_boundary(hfpf_mod, empty, shapes, planes):
    verts, tris = shapes
    (points, segments, contours, recs, s), _ = both(empty, verts, tris, S.IDENT, planes, "sphere and box, %d planes" % len(planes))
    print("%d planes: %d segments, %d points, %d contours" % (len(planes), len(segments), len(points), len(contours)))
    assert (contours["flags"] == X.CLOSED).all() and s["n_tris_invalid"] == 96
    if len(planes) > 1:
        assert (recs["n_segments"] == 0).any() and (recs["n_contours"] == 2).any(), "a plane that misses everything, one that meets both shapes"
    if len(planes) == 65:
        assert recs[64]["n_segments"] > 0, "the plane behind the chunk boundary cuts something"


@pytest.mark.parametrize("make", [S.parallel_planes, S.mixed_planes], ids=["parallel", "mixed"])
def test_sixty_five_planes_cut_down_to_sixty_four(hfpf_mod, empty, shapes, make):
    verts, tris = shapes
    a = empty.section_mesh(verts, tris, S.IDENT, make(65))
    b = empty.section_mesh(verts, tris, S.IDENT, make(65)[:64])
    for name, x, y in zip(S.NAMES, S.cut_to_planes(a, 64), b[:4]):
        assert x.tobytes() == y.tobytes(), name


# ---- 3. a soup with invalid and far triangles ---------------------------------------------------------------------------------------

def test_soup_with_invalid_and_far_triangles_host_and_device(hfpf_mod, empty):
    verts, tris = S.soup()
    planes = S.soup_planes()
    (points, segments, contours, recs, s), ref = both(empty, verts, tris, S.IDENT, planes, "soup, host form")
    print("soup: %r, segments per plane %r" % (s, recs["n_segments"].tolist()))
    assert s["n_tris_invalid"] == 78 and s["n_tris_far"] == 20 and s["n_tris_valid"] == len(tris) - 78
    assert (recs["n_segments"] > 0).all() and s["n_contours"] == s["n_segments"] and (contours["n_ends"] == 2).all()
    assert len(set((segments["tri"] % 64).tolist())) == 64, "crossing triangles at every lane position of a wave"
    assert len(set((segments["tri"] // 64).tolist())) > 8, "and in more than one workgroup"
    dev = device_form(empty, hfpf_mod, verts, tris, S.IDENT, planes)
    S.same_section(dev, ref, "soup, device form")


# ---- 4. non-manifold and mixed winding ----------------------------------------------------------------------------------------------

def test_non_manifold_edge_and_mixed_winding(hfpf_mod, empty):
    (points, _, contours, _, _), _ = both(empty, *S.fan(3), S.IDENT, [[0, 0, 1, 0.5]], "three triangles on one edge")
    assert contours["flags"].tolist() == [X.BRANCHED] and contours[0]["n_ends"] == 3
    (points, _, contours, _, _), _ = both(empty, *S.bow(), S.IDENT, [[0, 0, 1, 0.5]], "two triangles of opposite winding")
    assert contours["flags"].tolist() == [X.BRANCHED] and points[(points["va"] == 0) & (points["vb"] == 1)][0]["ends"] == 2 << 16
    (_, _, contours, _, s), _ = both(empty, *S.unweld(CUBE_V, CUBE_T), S.IDENT, [[0, 0, 1, 0.25]], "the cube as a soup")
    assert len(contours) == 8 and (contours["n_ends"] == 2).all() and s["n_closed"] == 0


# ---- 5. the model's own mesh, without leaving HBM -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def session(hfpf_mod, synth_mod):
    sc = DepthScene(3, 160, 120, clean_every=2)
    g = grid(hfpf_mod)
    run(g, sc)
    yield sc, g
    g.close()


OWN_PLANES = np.array([[0, 1.0, 0, -0.04], [0, 1.0, 0, 0.0], [0, 1.0, 0, 0.04], [1.0, 0, 0, -0.14], [1.0, 0, 0, 0.05], [2.0, 0, 0, 0.2],
                       [0.6, 0.3, 1.0, 0.48]])  # three orientations through the sphere and the box of the scene


def test_own_mesh_device_and_host_forms(hfpf_mod, session):
    sc, g = session
    before, rows_before, bytes_before = counters(g), g.extract().tobytes(), g.counters()["device_bytes"]
    dv, nv, dt, nt = g.extract_mesh_device()
    try:
        assert nt > 1000
        dev = S.section_device(g, hfpf_mod, dv, nv, 32, dt, nt, S.IDENT, OWN_PLANES)
        verts = g.device_download(dv, nv * 32).view(hfpf_mod.MESH_VERTEX_DTYPE)
        tris = g.device_download(dt, nt * 12).view(np.uint32).reshape(-1, 3)
    finally:
        g.device_free(dv), g.device_free(dt)
    ref = S.reference(verts, tris, S.IDENT, OWN_PLANES, stride=32)
    S.same_section(dev, ref, "own mesh, device form")
    S.consistent(*dev)
    host = g.section_mesh(verts, tris, S.IDENT, OWN_PLANES)
    S.same_section(host, ref, "own mesh, host form")
    for name, a, b in zip(S.NAMES, host[:4], dev[:4]):
        assert a.tobytes() == b.tobytes(), name
    points, segments, contours, recs, s = dev
    print("own mesh of %d triangles: segments per plane %r, %d contours, %d closed" % (nt, recs["n_segments"].tolist(), len(contours), s["n_closed"]))
    assert recs["n_segments"].max() > 100 and (contours["flags"] & X.CLOSED == 0).any(), "a real profile, open where the scan is"
    assert counters(g) == before and g.extract().tobytes() == rows_before, "a section changes nothing on the handle"
    assert g.counters()["device_bytes"] >= bytes_before


# ---- 6. a rotated mesh frame --------------------------------------------------------------------------------------------------------

def test_rotated_mesh_frame_brought_back_by_the_pose(hfpf_mod, empty, shapes):
    verts, tris = shapes
    pose = S.rigid(0.7, (0.3, -1.0, 0.5), (0.02, -0.03, 0.04))
    R, t = pose[:, :3], pose[:, 3]
    moved = ((verts.astype(np.float64) - t) @ R).astype(np.float32)  # the mesh frame: pose maps it back (up to f32 rounding)
    got, ref = both(empty, moved, tris, pose, S.parallel_planes(9), "rotated mesh frame")
    assert (got[2]["flags"] == X.CLOSED).all() and len(got[2]) >= 9
    dev = device_form(empty, hfpf_mod, moved, tris, pose, S.parallel_planes(9))
    S.same_section(dev, ref, "rotated mesh frame, device form")


# ---- 7. far from the origin ---------------------------------------------------------------------------------------------------------

def test_cube_in_a_box_far_from_the_origin(hfpf_mod):
    bbox = (1023.5, 1024.5, -512.5, -511.5, 256.0, 257.0)
    verts, tris = S.cube(lo=(1023.5, -512.5, 256.0))
    planes = [[0, 0, 1, 256.25], [0, 0, -2, -512.5], [1, 1, 1, 768.5]]
    with hfpf_mod.OccupancyGrid(resolution=RES, bbox=bbox, **TINY) as g:
        (_, _, contours, _, s), _ = both(g, verts, tris, S.IDENT, planes, "far cube", bbox=bbox)
    assert s["n_tris_far"] == 0 and (contours["flags"] == X.CLOSED).all()
    assert contours["area_q28"].tolist()[:2] == [S.Q28, S.Q28] and contours["length_q32"].tolist()[:2] == [4 * S.Q32, 4 * S.Q32]


def test_cube_far_from_the_box_is_counted_as_far(hfpf_mod, empty):
    verts, tris = S.cube(lo=(1023.5, -512.5, 256.0))
    (points, _, _, _, s), _ = both(empty, verts, tris, S.IDENT, [[0, 0, 1, 256.25]], "far from the box")
    assert s["n_tris_far"] == 12 and s["n_tris_valid"] == 12 and len(points) == 0


# ---- 8. the cap, reached for real ---------------------------------------------------------------------------------------------------

def test_the_per_plane_cap_is_reached_and_one_more_fails(hfpf_mod, empty):
    n = hfpf_mod.SECTION_MAX_PLANE_SEGMENTS
    verts, tris = S.strip(n + 1)
    planes = [[0, 0, 1, 9.0], [0, 1, 0, 0.0]]  # plane 0 misses the strip, plane 1 crosses every triangle
    points, segments, contours, recs, s = empty.section_mesh(verts[:3 * n], tris[:n], S.IDENT, planes)
    assert s["n_segments"] == n == recs[1]["n_segments"] and recs[0]["n_segments"] == 0 and s["n_points"] == 2 * n and s["n_contours"] == n
    assert recs[1]["length_q32"] == n * (S.Q32 >> 23) and int(contours["length_q32"].sum()) == n * (S.Q32 >> 23), "2^20 segments of 2^-23 m"
    assert (segments["tri"] == np.arange(n)).all() and (contours["n_ends"] == 2).all()
    with pytest.raises(hfpf_mod.HfpfError) as e:
        empty.section_mesh(verts, tris, S.IDENT, planes)
    assert e.value.code == CAPACITY and "plane 1 " in str(e.value) and str(n + 1) in str(e.value), str(e.value)
    got, _ = both(empty, CUBE_V, CUBE_T, S.IDENT, [[0, 0, 1, 0.25]], "the next call on the handle")
    assert got[4]["n_closed"] == 1


# ---- 9. arguments and state ---------------------------------------------------------------------------------------------------------

SENTINEL = 0x5A


class Call:
    """One raw call of either form with every output preset to a sentinel: run() returns the status, untouched() says whether any
    output byte changed."""

    def __init__(self, H, g, device, d_mesh=None):
        self.H, self.g, self.device = H, g, device
        self.verts, self.tris = np.ascontiguousarray(CUBE_V), np.ascontiguousarray(CUBE_T)
        self.pose = np.ascontiguousarray(S.IDENT, np.float64).reshape(12).copy()
        self.planes = np.array([[0, 0, 1, 0.25], [1, 1, 1, 0.5]], np.float64)
        self.opts = H.section_opts()
        vp, tp = d_mesh if device else (self.verts.ctypes.data, self.tris.ctypes.data)
        self.a = dict(opts=C.byref(self.opts), verts=C.c_void_p(vp), n_verts=8, stride=12, tris=C.c_void_p(tp), n_tris=12,
                      pose=C.c_void_p(self.pose.ctypes.data), planes=C.c_void_p(self.planes.ctypes.data), n_planes=2)
        self.ptrs = [C.c_void_p(SENTINEL) for _ in range(3)]
        self.counts = [C.c_uint64(SENTINEL) for _ in range(3)]
        self.recs = np.full(2 * 64, SENTINEL, np.uint8)
        self.summary = np.full(64, SENTINEL, np.uint8)
        self.outs = dict(points=C.byref(self.ptrs[0]), n_points=C.byref(self.counts[0]), segments=C.byref(self.ptrs[1]), n_segments=C.byref(self.counts[1]),
                         contours=C.byref(self.ptrs[2]), n_contours=C.byref(self.counts[2]), recs=C.c_void_p(self.recs.ctypes.data),
                         summary=C.c_void_p(self.summary.ctypes.data))

    def run(self):
        a, o = self.a, self.outs
        raw = C.CDLL(self.H.lib()._name)  # the library again, without the binding's argument types: every argument is given its C type here
        fn = raw.hfpf_section_mesh_device if self.device else raw.hfpf_section_mesh
        return fn(self.g._h, a["opts"], a["verts"], C.c_uint64(a["n_verts"]), C.c_uint32(a["stride"]), a["tris"], C.c_uint64(a["n_tris"]),
                  a["pose"], a["planes"], C.c_uint32(a["n_planes"]), o["points"], o["n_points"], o["segments"], o["n_segments"], o["contours"],
                  o["n_contours"], o["recs"], o["summary"])

    def untouched(self):
        return (all(p.value == SENTINEL for p in self.ptrs) and all(c.value == SENTINEL for c in self.counts) and (self.recs == SENTINEL).all() and
                (self.summary == SENTINEL).all())


def _rejections(device):
    nan, inf = float("nan"), float("inf")
    def plane(j, k, v):
        def f(c):
            c.planes[j, k] = v
        return f
    def arg(**kw):
        return lambda c: c.a.update(kw)
    def out(name):
        return lambda c: c.outs.update({name: None})
    def opts(field, v):
        return lambda c: setattr(c.opts, field, v)
    def pose(i, v):
        def f(c):
            c.pose[i] = v
        return f
    cases = [("struct_size", opts("struct_size", 8)), ("flags", opts("flags", 1)), ("reserved", opts("reserved", 1)), ("NULL opts", arg(opts=None)),
             ("stride 8", arg(stride=8)), ("stride 14", arg(stride=14)), ("NULL verts", arg(verts=None)), ("NULL tris", arg(tris=None)),
             ("n_verts 2^32", arg(n_verts=1 << 32)), ("n_tris 2^32 - 1", arg(n_tris=0xFFFFFFFF)), ("NULL pose", arg(pose=None)),
             ("NaN pose", pose(5, nan)), ("inf pose", pose(11, inf)), ("NaN normal", plane(0, 1, nan)), ("inf d", plane(1, 3, inf)),
             ("zero normal", lambda c: c.planes.__setitem__((1, slice(0, 3)), 0.0)), ("overflowing normal", plane(0, 0, 1e200)),
             ("NULL planes", arg(planes=None)), ("4097 planes", arg(n_planes=4097)), ("n_verts 2^26 + 1", arg(n_verts=(1 << 26) + 1))]
    cases += [("NULL %s" % k, out(k)) for k in ("points", "n_points", "segments", "n_segments", "contours", "n_contours", "recs", "summary")]
    if device:
        cases += [("misaligned verts", lambda c: c.a.update(verts=C.c_void_p(c.a["verts"].value + 2))),
                  ("misaligned tris", lambda c: c.a.update(tris=C.c_void_p(c.a["tris"].value + 1)))]
    return cases


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_every_rejection_leaves_the_outputs_untouched(hfpf_mod, empty, device):
    with uploaded(empty, CUBE_V, CUBE_T) as d_mesh:
        for what, spoil in _rejections(device):
            c = Call(hfpf_mod, empty, device, d_mesh)
            spoil(c)
            rc = c.run()
            assert rc == BAD_ARG, "%s: status %d" % (what, rc)
            assert c.untouched(), "%s: an output was written" % what
        c = Call(hfpf_mod, empty, device, d_mesh)  # and the unspoiled call works on the same handle
        assert c.run() == 0 and c.counts[1].value == 8 + 12 and not c.untouched()
        if device:
            for p in c.ptrs:
                empty.device_free(p.value)
        else:
            hfpf_mod.lib().hfpf_free_section(*c.ptrs)


def test_no_planes_and_no_triangles_return_the_documented_empties(hfpf_mod, empty):
    verts, tris = S.soup()
    got, _ = both(empty, verts, tris, S.IDENT, np.zeros((0, 4)), "no planes")
    assert got[4]["n_tris_invalid"] == 78 and got[4]["n_tris_far"] == 20 and got[4]["n_segments"] == 0 and len(got[3]) == 0
    got, _ = both(empty, CUBE_V, np.zeros((0, 3), np.uint32), S.IDENT, S.soup_planes(), "no triangles")
    assert got[3].tobytes() == bytes(5 * 64) and all(v == 0 for v in got[4].values()) and len(got[0]) == len(got[1]) == len(got[2]) == 0
    got, _ = both(empty, np.zeros((0, 3), np.float32), CUBE_T, S.IDENT, S.soup_planes(), "no vertices")
    assert got[4]["n_tris_invalid"] == 12 and got[4]["n_segments"] == 0
    with uploaded(empty, CUBE_V, CUBE_T) as (dv, dt):
        (p, npt), (s, ns), (c, nc), recs, summ = empty.section_mesh_device(dv, 8, 12, dt, 12, S.IDENT, [[0, 0, 1, 5.0]])
    assert (p, npt, s, ns, c, nc) == (0, 0, 0, 0, 0, 0) and recs.tobytes() == bytes(64) and summ["n_tris_valid"] == 12


def test_the_device_form_returns_the_same_empties(hfpf_mod, empty):
    """No planes, no triangles and no vertices through hfpf_section_mesh_device: NULL arrays, and the records and the summary of the host form."""
    verts, tris = S.soup()
    for v, t, planes, what in ((verts, tris, np.zeros((0, 4)), "no planes"), (CUBE_V, np.zeros((0, 3), np.uint32), S.soup_planes(), "no triangles"),
                               (np.zeros((0, 3), np.float32), CUBE_T, S.soup_planes(), "no vertices")):
        host = empty.section_mesh(v, t, S.IDENT, planes)
        with uploaded(empty, v, t) as (dv, dt):
            (p, npt), (s, ns), (c, nc), recs, summ = empty.section_mesh_device(dv, len(v), 12, dt, len(t), S.IDENT, planes)
        assert (p, npt, s, ns, c, nc) == (0, 0, 0, 0, 0, 0) and len(host[0]) == len(host[1]) == len(host[2]) == 0, what
        assert recs.tobytes() == host[3].tobytes() == bytes(64 * len(planes)) and summ == host[4], what


def test_device_bytes_do_not_shrink(hfpf_mod, empty, shapes):
    verts, tris = shapes
    seen = [empty.counters()["device_bytes"]]
    for planes in (S.parallel_planes(64), S.parallel_planes(1), S.mixed_planes(65)):
        empty.section_mesh(verts, tris, S.IDENT, planes)
        seen.append(empty.counters()["device_bytes"])
    assert seen == sorted(seen), seen
