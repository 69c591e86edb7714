"""GPU: a triangle mesh of the fused model (hfpf_extract_mesh, hfpf_extract_mesh_device).  A mesh is defined on the rows hfpf_extract
returns and the cells hfpf_get_occupied lists, so both forms are compared byte for byte with tests/mesh_ref.py run on those."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_ref as M
from gpu_support import BBOX, DEPTH_CAPS, RES, grid, mesh_device, node_feed, node_grid, run, same_mesh, same_planes, two_handles, unchanged
from pcd_io import read_ply
from scenes import DepthScene

pytestmark = pytest.mark.gpu
INF = float("inf")
SPHERE_C, SPHERE_R = np.array([0.05, 0.0, 0.45]), 0.10  # synth/synth.cpp
# (radius, min_count, max_distance): every radius class, a count gate, a tight distance gate
OPTION_SETS = [(1, 0.0, INF), (2, 0.0, INF), (4, 0.0, INF), (2, 3.0, INF), (2, 0.0, 0.002)]


@pytest.fixture(scope="module")
def session(hfpf_mod, synth_mod):
    sc = DepthScene(12, 640, 480, clean_every=4)
    g = grid(hfpf_mod)
    run(g, sc)
    rows = g.extract().copy()
    occ = g.occupied()
    yield sc, g, rows, occ
    g.close()


def _ref(g, rows, occ, radius, min_count, max_distance):
    dims, res = g.dims
    v, t, _ = M.mesh(rows, occ, tuple(g.cfg.bbox), res, dims, radius=radius, min_count=min_count, max_distance=max_distance)
    return v, t


# ---- 1. byte-identical to the numpy contract -----------------------------------------------------------------------------

@pytest.mark.parametrize("opt", OPTION_SETS, ids=["r%d_mc%g_md%g" % o for o in OPTION_SETS])
def test_host_and_device_forms_are_byte_identical_to_mesh_ref(hfpf_mod, session, opt):
    sc, g, rows, occ = session
    radius, min_count, max_distance = opt
    kw = dict(radius=radius, min_count=min_count, max_distance=max_distance)
    host = g.extract_mesh(**kw)
    assert len(host[1]) > 1000
    ref = _ref(g, rows, occ, radius, min_count, max_distance)
    same_mesh(host, ref, "host form %r" % (opt,))
    same_mesh(mesh_device(g, **kw), ref, "device form %r" % (opt,))


# ---- 2. geometry ---------------------------------------------------------------------------------------------------------

def test_geometry(hfpf_mod, session):
    sc, g, rows, occ = session
    v, t = g.extract_mesh(radius=2)
    p = M.positions(v).astype(np.float64)
    # A vertex whose two edge endpoints both take their samples from rows on the sphere with outward normals lies on it.  (Rows
    # seen at grazing angles near the silhouette can be oriented inwards; an edge between such a row's sample and an outward one's
    # has a sign change that is not a surface crossing, and its vertex lies up to one lattice edge off the sphere: include/hfpf.h.)
    dims, res = g.dims
    rv, rt, _, (ea, eb) = M.mesh(rows, occ, tuple(g.cfg.bbox), res, dims, radius=2, with_ends=True)
    assert rv.tobytes() == v.tobytes() and rt.tobytes() == t.tobytes()

    def outward_on_sphere(r):
        rc = np.stack([r["x"], r["y"], r["z"]], axis=1).astype(np.float64) - SPHERE_C
        rd = np.linalg.norm(rc, axis=1)
        n = np.stack([r["nx"], r["ny"], r["nz"]], axis=1).astype(np.float64)
        return (np.abs(rd - SPHERE_R) < 0.0005) & (np.einsum("ij,ij->i", n, rc / rd[:, None]) > 0.9)

    on = outward_on_sphere(ea) & outward_on_sphere(eb)
    assert on.sum() > 10000
    err = np.abs(np.linalg.norm(p[on] - SPHERE_C, axis=1) - SPHERE_R)
    assert np.quantile(err, 0.99) < 0.0005 and err.max() < 0.001, np.quantile(err, [0.5, 0.9, 0.99, 1.0])
    nrm = np.stack([v["nx"], v["ny"], v["nz"]], axis=1).astype(np.float64)
    _, cnt, _ = M.edge_use(t)
    assert cnt.max() <= 2, "no edge is used by more than two triangles"
    n = M.face_normals(v, t)
    big = np.linalg.norm(n, axis=1) > 1e-14
    vn = nrm[t.astype(np.int64)].sum(axis=1)
    facing = np.einsum("ij,ij->i", n[big], vn[big]) > 0
    assert facing.mean() > 0.99, facing.mean()


def test_colour_is_the_rows_colour(hfpf_mod, session):
    sc, g, rows, occ = session
    v, t = g.extract_mesh(radius=2)
    assert v["rgb"].any()
    assert set(np.unique(v["rgb"])) <= set(np.unique(rows["rgb"]))


# ---- 3. no side effects, edges, refusals ---------------------------------------------------------------------------------

def test_a_mesh_changes_nothing(hfpf_mod, synth_mod):
    sc = DepthScene(10, 320, 240, clean_every=3)
    K = sc.K

    def look(g, i):
        g.extract_mesh(radius=1 + i % 4)

    def on_empty(b):  # before the first clean
        v0, t0 = b.extract_mesh()
        assert len(v0) == 0 and len(t0) == 0
        assert b.extract_mesh_device() == (0, 0, 0, 0)

    with two_handles(hfpf_mod, sc, look, on_empty) as (a, b, rb):
        ia = a.render(sc.poses[2], K, sc.W, sc.H, z_range=(0.05, 3.0), splat_radius=2)
        same_planes(ia, b.render(sc.poses[2], K, sc.W, sc.H, z_range=(0.05, 3.0), splat_radius=2), "a render of both handles")
        one, two = b.extract_mesh(), b.extract_mesh()
        same_mesh(one, two, "second mesh")
        same_mesh(one, _ref(b, rb, b.occupied(), 2, 0.0, INF), "mesh_ref")
        unchanged(a, b, rb)


def test_bad_arguments_are_refused_and_the_handle_stays_usable(hfpf_mod, synth_mod):
    H_ = hfpf_mod
    sc = DepthScene(6, 160, 120, clean_every=3)
    bad = {"struct_size": ("struct_size", 24), "flags": ("flags", 1), "reserved": ("reserved", 1), "radius 0": ("radius", 0),
           "radius 5": ("radius", 5), "min_count nan": ("min_count", float("nan")), "max_distance 0": ("max_distance", 0.0),
           "max_distance -1": ("max_distance", -1.0), "max_distance nan": ("max_distance", float("nan"))}
    L = H_.lib()
    with grid(hfpf_mod) as g:
        run(g, sc)
        want = g.extract().copy()
        ref = _ref(g, want, g.occupied(), 2, 0.0, INF)
        v, nv, t, nt = C.c_void_p(7), C.c_uint64(7), C.c_void_p(7), C.c_uint64(7)
        outs = (C.byref(v), C.byref(nv), C.byref(t), C.byref(nt))
        for fn in (L.hfpf_extract_mesh, L.hfpf_extract_mesh_device):
            for what, (field, val) in bad.items():
                o = H_.mesh_opts()
                setattr(o, field, val)
                assert fn(g._h, C.byref(o), *outs) == -2, what
            assert fn(g._h, None, *outs) == -2, "NULL opts"
            o = H_.mesh_opts()
            for k in range(4):
                args = list(outs)
                args[k] = None
                assert fn(g._h, C.byref(o), *args) == -2, "NULL output %d" % k
            assert (v.value, nv.value, t.value, nt.value) == (7, 7, 7, 7), "a refused call wrote its output"
        assert g.extract().tobytes() == want.tobytes()
        same_mesh(g.extract_mesh(), ref, "after the refusals")
        same_mesh(mesh_device(g), ref, "device form after the refusals")


# ---- 4. the node shell ---------------------------------------------------------------------------------------------------

def test_node_writes_mesh_ply(hfpf_mod, synth_mod, tmp_path):
    import hfpf_node
    sc = DepthScene(6, 320, 240, clean_every=0)
    opts = hfpf_mod.mesh_opts(radius=2)
    caps = dict(DEPTH_CAPS)
    with hfpf_node.FusionNode(BBOX, directory_name=str(tmp_path), resolution=RES, final_clean_on_process=True, **caps) as n:
        n.set_mesh_output(opts)
        node_feed(n, sc)
        # the mesh the node will write: the same model, meshed through the engine handle before ~process clears it
        g = node_grid(hfpf_mod, hfpf_node, n)
        g.clean()
        v, t = g.extract_mesh(opts=opts)
        g._h = None
        rc, ok, msg = n.process()
        assert rc == 0 and ok, msg
    path = os.path.join(tmp_path, "mesh.ply")
    ref = os.path.join(tmp_path, "ref.ply")
    hfpf_mod.write_ply(v, t, ref)
    assert len(t) > 1000
    assert open(path, "rb").read() == open(ref, "rb").read()
    pv, pf = read_ply(path)
    assert len(pv) == len(v) and len(pf) == len(t)
    with hfpf_node.FusionNode(BBOX, directory_name=str(tmp_path / "off"), resolution=RES, **caps) as n:
        os.makedirs(str(tmp_path / "off"))
        n.set_mesh_output(opts)
        n.set_mesh_output(None)
        n.start()
        rc, ok, msg = n.process()
        assert rc == 0 and ok, msg
        assert not os.path.exists(str(tmp_path / "off" / "mesh.ply"))
