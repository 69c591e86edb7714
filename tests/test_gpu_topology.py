"""GPU: open edges of a triangle mesh (hfpf_mesh_topology, hfpf_mesh_topology_device).  The call is defined on its arguments alone and
every output is an integer reduction, a sort rank or a union-find label, so every edge, loop, shell, per-triangle word and the summary
are compared byte for byte with tests/topology_ref.py: no tolerance is involved.  The meshes are those of tests/test_topology_ref.py, a
seeded soup, fans that make one run of the sort longer than a wave and than a workgroup, a welded strip that sends 70,000 triangles
into one shell and 70,002 edges into one loop, and the model's own mesh of the section tests' session."""
import ctypes as C

import numpy as np
import pytest

import plan_support as PS
import section_support as S
import topology_ref as T
import topology_support as TS
from gpu_support import RES, counters, grid, run, uploaded
from scenes import DepthScene

pytestmark = pytest.mark.gpu
TINY = dict(max_bricks=2000, max_log_points=1 << 18, max_normals=1 << 14, max_frames=16)  # a handle that fuses nothing
BAD_ARG = -2
CUBE_V, CUBE_T = S.cube()


@pytest.fixture(scope="module")
def empty(hfpf_mod):
    """An empty handle with the default box: the call needs no fused model."""
    g = hfpf_mod.OccupancyGrid(resolution=RES, bbox=S.BBOX, **TINY)
    yield g
    g.close()


def device_form(g, H, verts, tris, pose=S.IDENT, stride=None, tri_shell=True):
    verts = np.ascontiguousarray(verts)
    stride = stride if stride is not None else (verts.dtype.itemsize if verts.dtype.names else 12)
    with uploaded(g, verts, tris) as (dv, dt):
        return TS.topology_device(g, H, dv, len(verts), stride, dt, len(tris), pose, tri_shell=tri_shell)


def both(g, H, verts, tris, what, pose=S.IDENT, bbox=S.BBOX):
    """The host form and the device form against the reference; returns the host form's result."""
    ref = TS.reference(verts, tris, pose, bbox)
    got = g.mesh_topology(verts, tris, pose)
    TS.same_topology(got, ref, what + ", host form")
    TS.consistent(*got)
    TS.same_topology(device_form(g, H, verts, tris, pose), ref, what + ", device form")
    return got


# ---- 1. the small meshes of the reference's own tests -------------------------------------------------------------------------------

def test_cube_and_cube_without_a_face(hfpf_mod, empty):
    _, _, shells, _, s = both(empty, hfpf_mod, CUBE_V, CUBE_T, "cube")
    assert s["n_watertight"] == 1 and shells[0]["area_q32"] == 6 * TS.Q32 and shells[0]["volume_q40"] == TS.Q40 + 2
    edges, loops, shells, _, s = both(empty, hfpf_mod, *TS.open_cube(), "cube without its top")
    assert s["n_boundary"] == 4 and loops[0]["flags"] == T.LOOP_CLOSED and loops[0]["area_q28"].tolist() == [0, 0, -TS.Q28]
    assert loops[0]["length_q32"] == 4 * TS.Q32 and shells[0]["flags"] == T.SHELL_OPEN


def test_non_manifold_miswound_soup_and_lone_triangle(hfpf_mod, empty):
    edges, loops, _, _, s = both(empty, hfpf_mod, *S.fan(3), "fan of three")
    assert s["n_nonmanifold"] == 1 and s["n_boundary"] == 6 and loops[0]["flags"] == T.LOOP_BRANCHED
    edges, loops, _, _, s = both(empty, hfpf_mod, *S.bow(), "bow")
    assert s["n_miswound"] == 1 and edges[edges["kind"] == T.MISWOUND][0]["uses"] == 2 and loops[0]["n_ends"] == 0
    _, loops, shells, _, s = both(empty, hfpf_mod, *S.unweld(CUBE_V, CUBE_T), "the cube as a soup")
    assert s["n_boundary"] == 36 and len(shells) == 12 and s["n_closed_loops"] == 12
    _, loops, _, _, _ = both(empty, hfpf_mod, *TS.lone_triangle(), "a lone triangle")
    assert len(loops) == 1 and loops[0]["flags"] == T.LOOP_CLOSED


def test_sphere_and_box(hfpf_mod, empty):
    verts, tris = PS.sphere_and_box()
    _, _, shells, _, s = both(empty, hfpf_mod, verts, tris, "sphere and box")
    assert (s["n_tris_invalid"], s["n_interior"], s["n_boundary"]) == (96, 3234, 192) and s["n_watertight"] >= 1


# ---- 2. a soup with invalid and far triangles ---------------------------------------------------------------------------------------

def test_soup_with_invalid_and_far_triangles(hfpf_mod, empty):
    verts, tris = S.soup()
    edges, loops, shells, tri_shell, s = both(empty, hfpf_mod, verts, tris, "soup")
    print("soup: %r" % (s,))
    assert (s["n_tris_invalid"], s["n_tris_far"], s["n_tris_valid"]) == (78, 20, len(tris) - 78)
    assert s["n_shells"] == s["n_loops"] == len(tris) - 98 and len(edges) == 3 * s["n_shells"]
    assert len(set((edges["tri"] % 64).tolist())) == 64, "listed edges from every lane position of a wave"
    assert len(set((edges["tri"] // 256).tolist())) > 2, "and from more than one workgroup"


# ---- 3. the run walk ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [63, 64, 65, 257, 300])
def test_one_edge_used_by_a_whole_fan(hfpf_mod, empty, n):
    edges, _, shells, _, s = both(empty, hfpf_mod, *S.fan(n), "fan of %d" % n)
    nm = edges[edges["kind"] == T.NONMANIFOLD]
    assert len(nm) == 1 and nm[0]["uses"] == n and nm[0]["tri"] == 0 and s["n_boundary"] == 2 * n and len(shells) == 1


def test_uses_saturate_and_the_classes_stay_exact(hfpf_mod, empty):
    n = 70000
    edges, _, _, _, s = both(empty, hfpf_mod, *S.fan(n), "fan of %d" % n)
    assert edges[0]["kind"] == T.NONMANIFOLD and edges[0]["uses"] == 65535 and (s["n_nonmanifold"], s["n_boundary"], s["n_interior"]) == (1, 2 * n, 0)


# ---- 4. same-address sums, chunk and grid edges -------------------------------------------------------------------------------------

def test_seventy_thousand_triangles_in_one_shell_and_one_loop(hfpf_mod, empty):
    n = 70000
    edges, loops, shells, tri_shell, s = both(empty, hfpf_mod, *TS.welded_strip(n), "welded strip of %d" % n)
    assert (s["n_shells"], s["n_loops"], s["n_closed_loops"], s["n_interior"], s["n_boundary"]) == (1, 1, 1, n - 1, n + 2)
    assert loops[0]["n_edges"] == n + 2 == loops[0]["n_verts"] and shells[0]["n_tris"] == n and (tri_shell == 0).all()
    assert loops[0]["length_q32"] == n * int(TS.STRIP_PITCH * TS.Q32) + 2 * int(2 * TS.STRIP_HALF * TS.Q32)
    assert shells[0]["area_q32"] == n * int(TS.STRIP_PITCH * TS.STRIP_HALF * TS.Q32)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_meshes_at_the_edges_of_a_workgroup(hfpf_mod, empty, n):
    _, loops, shells, _, s = both(empty, hfpf_mod, *TS.welded_strip(n), "welded strip of %d" % n)
    assert (s["n_shells"], s["n_closed_loops"], s["n_interior"], s["n_boundary"]) == (1, 1, n - 1, n + 2)


# ---- 5. the model's own mesh, without leaving HBM -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def session(hfpf_mod, synth_mod):
    sc = DepthScene(3, 160, 120, clean_every=2)
    g = grid(hfpf_mod)
    run(g, sc)
    yield sc, g
    g.close()


def test_own_mesh_device_and_host_forms(hfpf_mod, session):
    sc, g = session
    before, rows_before, hidden_before, bytes_before = counters(g), g.extract().tobytes(), g.hidden().tobytes(), g.counters()["device_bytes"]
    mesh_bytes = None
    dv, nv, dt, nt = g.extract_mesh_device()
    try:
        assert nt > 1000
        dev = TS.topology_device(g, hfpf_mod, dv, nv, 32, dt, nt)
        verts = g.device_download(dv, nv * 32).view(hfpf_mod.MESH_VERTEX_DTYPE)
        tris = g.device_download(dt, nt * 12).view(np.uint32).reshape(-1, 3)
        mesh_bytes = verts.tobytes() + tris.tobytes()
    finally:
        g.device_free(dv), g.device_free(dt)
    ref = TS.reference(verts, tris, stride=32)
    TS.same_topology(dev, ref, "own mesh, device form")
    TS.consistent(*dev)
    host = g.mesh_topology(verts, tris)
    TS.same_topology(host, ref, "own mesh, host form")
    for name, a, b in zip(TS.NAMES, host[:4], dev[:4]):
        assert a.tobytes() == b.tobytes(), name
    edges, loops, shells, _, s = dev
    print("own mesh of %d triangles: %r; the five longest loops have %r edges" % (nt, s, sorted(loops["n_edges"].tolist())[-5:]))
    assert s["n_boundary"] > 0 and s["n_closed_loops"] >= 1, "a scan has a rim, and a real hole or rim closes"
    assert counters(g) == before and g.extract().tobytes() == rows_before and g.hidden().tobytes() == hidden_before, "the call changes nothing on the handle"
    v2, t2 = g.extract_mesh()
    assert v2.tobytes() + t2.tobytes() == mesh_bytes, "the mesh extracts to the same bytes behind the call"
    assert g.counters()["device_bytes"] >= bytes_before


# ---- 6. poses and boxes -------------------------------------------------------------------------------------------------------------

def test_rotated_mesh_frame_brought_back_by_the_pose(hfpf_mod, empty):
    verts, tris = PS.sphere_and_box()
    pose = S.rigid(0.7, (0.3, -1.0, 0.5), (0.02, -0.03, 0.04))
    R, t = pose[:, :3], pose[:, 3]
    moved = ((verts.astype(np.float64) - t) @ R).astype(np.float32)  # the mesh frame: pose maps it back (up to f32 rounding)
    _, _, _, _, s = both(empty, hfpf_mod, moved, tris, "rotated mesh frame", pose=pose)
    assert (s["n_interior"], s["n_boundary"]) == (3234, 192)


def test_cube_in_a_box_far_from_the_origin(hfpf_mod):
    verts, tris = S.cube(lo=TS.FAR_LO)
    with hfpf_mod.OccupancyGrid(resolution=RES, bbox=TS.FAR_BBOX, **TINY) as g:
        _, _, shells, _, s = both(g, hfpf_mod, verts, tris, "far cube", bbox=TS.FAR_BBOX)
    assert s["n_tris_far"] == 0 and s["n_watertight"] == 1 and shells[0]["area_q32"] == 6 * TS.Q32 and abs(int(shells[0]["volume_q40"]) - TS.Q40) <= 12


def test_cube_far_from_the_box_is_counted_as_far(hfpf_mod, empty):
    verts, tris = S.cube(lo=TS.FAR_LO)
    edges, loops, shells, tri_shell, s = both(empty, hfpf_mod, verts, tris, "far from the box")
    assert s["n_tris_far"] == 12 == s["n_tris_valid"] and len(shells) == len(loops) == len(edges) == 0 and (tri_shell == T.NONE).all() and len(tri_shell) == 12


# ---- 7. tri_shell -------------------------------------------------------------------------------------------------------------------

def test_tri_shell_is_optional(hfpf_mod, empty):
    verts, tris = S.soup()
    ref = TS.reference(verts, tris)
    got = empty.mesh_topology(verts, tris)
    assert got[3].tobytes() == ref[3].tobytes() and (got[3] == T.NONE).sum() == 98
    without = empty.mesh_topology(verts, tris, tri_shell=False)
    assert without[3] is None
    TS.same_topology(without, ref, "without tri_shell, host form", tri_shell=False)
    dev = device_form(empty, hfpf_mod, verts, tris, tri_shell=False)
    assert dev[3] is None
    TS.same_topology(dev, ref, "without tri_shell, device form", tri_shell=False)


# ---- 8. arguments and state ---------------------------------------------------------------------------------------------------------

SENTINEL = 0x5A


class Call:
    """One raw call of either form with every output preset to a sentinel: run() returns the status, untouched() says whether any
    output byte changed."""

    def __init__(self, H, g, device, d_mesh=None):
        self.H, self.g, self.device = H, g, device
        self.verts, self.tris = np.ascontiguousarray(CUBE_V), np.ascontiguousarray(TS.open_cube()[1])
        self.pose = np.ascontiguousarray(S.IDENT, np.float64).reshape(12).copy()
        self.opts = H.topology_opts()
        vp, tp = d_mesh if device else (self.verts.ctypes.data, self.tris.ctypes.data)
        self.a = dict(opts=C.byref(self.opts), verts=C.c_void_p(vp), n_verts=8, stride=12, tris=C.c_void_p(tp), n_tris=10, pose=C.c_void_p(self.pose.ctypes.data))
        self.ptrs = [C.c_void_p(SENTINEL) for _ in range(4)]
        self.counts = [C.c_uint64(SENTINEL) for _ in range(3)]
        self.summary = np.full(128, SENTINEL, np.uint8)
        self.outs = dict(edges=C.byref(self.ptrs[0]), n_edges=C.byref(self.counts[0]), loops=C.byref(self.ptrs[1]), n_loops=C.byref(self.counts[1]),
                         shells=C.byref(self.ptrs[2]), n_shells=C.byref(self.counts[2]), tri_shell=C.byref(self.ptrs[3]),
                         summary=C.c_void_p(self.summary.ctypes.data))

    def run(self):
        a, o = self.a, self.outs
        raw = C.CDLL(self.H.lib()._name)  # the library again, without the binding's argument types: every argument is given its C type here
        fn = raw.hfpf_mesh_topology_device if self.device else raw.hfpf_mesh_topology
        return fn(self.g._h, a["opts"], a["verts"], C.c_uint64(a["n_verts"]), C.c_uint32(a["stride"]), a["tris"], C.c_uint64(a["n_tris"]), a["pose"],
                  o["edges"], o["n_edges"], o["loops"], o["n_loops"], o["shells"], o["n_shells"], o["tri_shell"], o["summary"])

    def untouched(self):
        return all(p.value == SENTINEL for p in self.ptrs) and all(c.value == SENTINEL for c in self.counts) and (self.summary == SENTINEL).all()


def _rejections(device):
    nan, inf = float("nan"), float("inf")
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
             ("NaN pose", pose(5, nan)), ("inf pose", pose(11, inf)),
             ("n_verts 2^26 + 1", arg(n_verts=(1 << 26) + 1)), ("3 n_tris = 2^32 + 2", arg(n_tris=((1 << 32) + 2) // 3))]
    cases += [("NULL %s" % k, out(k)) for k in ("edges", "n_edges", "loops", "n_loops", "shells", "n_shells", "summary")]
    if device:
        cases += [("misaligned verts", lambda c: c.a.update(verts=C.c_void_p(c.a["verts"].value + 2))),
                  ("misaligned tris", lambda c: c.a.update(tris=C.c_void_p(c.a["tris"].value + 1)))]
    return cases


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_every_rejection_leaves_the_outputs_untouched(hfpf_mod, empty, device):
    with uploaded(empty, CUBE_V, TS.open_cube()[1]) as d_mesh:
        for what, spoil in _rejections(device):
            c = Call(hfpf_mod, empty, device, d_mesh)
            spoil(c)
            rc = c.run()
            assert rc == BAD_ARG, "%s: status %d" % (what, rc)
            assert c.untouched(), "%s: an output was written" % what
        c = Call(hfpf_mod, empty, device, d_mesh)  # and the unspoiled call works on the same handle
        assert c.run() == 0 and [n.value for n in c.counts] == [4, 1, 1] and not c.untouched() and all(p.value for p in c.ptrs)
        if device:
            for p in c.ptrs:
                empty.device_free(p.value)
        else:
            hfpf_mod.lib().hfpf_free_topology(*c.ptrs)


def test_no_triangles_and_no_vertices_return_the_documented_empties(hfpf_mod, empty):
    none = np.zeros((0, 3), np.uint32)
    edges, loops, shells, tri_shell, s = both(empty, hfpf_mod, CUBE_V, none, "no triangles")
    assert len(edges) == len(loops) == len(shells) == len(tri_shell) == 0 and all(v == 0 for v in s.values())
    c = Call(hfpf_mod, empty, False)
    c.a.update(n_tris=0)
    assert c.run() == 0 and all(p.value is None for p in c.ptrs) and [n.value for n in c.counts] == [0, 0, 0] and (c.summary == 0).all()
    _, _, shells, tri_shell, s = both(empty, hfpf_mod, np.zeros((0, 3), np.float32), CUBE_T, "no vertices")
    assert s["n_tris_invalid"] == 12 and len(shells) == 0 and (tri_shell == T.NONE).all()


def test_device_bytes_do_not_shrink(hfpf_mod, empty):
    seen = [empty.counters()["device_bytes"]]
    for mesh in (PS.sphere_and_box(), TS.lone_triangle(), S.soup()):
        empty.mesh_topology(*mesh)
        seen.append(empty.counters()["device_bytes"])
    assert seen == sorted(seen), seen
