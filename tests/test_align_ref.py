"""CPU: the align contract (tests/align_ref.py = deviation_ref + track_ref) on a synthetic patch, and the host-side pieces of the
library: the exports, the struct sizes and hfpf_check_align_opts.  The patch is a gently curved height field sampled by hand with
analytic normals; the mesh is a triangulated copy of the same surface, displaced by a known small rigid motion."""
import ctypes as C

import numpy as np

import align_ref as A
import deviation_ref as D

BBOX = (-0.2, 0.2, -0.2, 0.2, 0.0, 0.4)  # centre (0, 0, 0.2)
MD = 0.02


def height(x, y):
    return 0.2 + 0.03 * np.sin(6.0 * x) * np.cos(5.0 * y) + 0.1 * x * y + 0.05 * x


def normal(x, y):
    hx = 0.18 * np.cos(6.0 * x) * np.cos(5.0 * y) + 0.1 * y + 0.05
    hy = -0.15 * np.sin(6.0 * x) * np.sin(5.0 * y) + 0.1 * x
    n = np.stack([-hx, -hy, np.ones_like(hx)], axis=-1)
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def patch_rows(n=18, lo=-0.12, hi=0.12):
    """n * n rows on the surface, offset from the mesh's lattice, with the analytic normals."""
    u = np.linspace(lo, hi, n) + 0.0013
    x, y = (a.ravel() for a in np.meshgrid(u, u, indexing="ij"))
    r = np.zeros(len(x), D.ROW_DTYPE)
    r["x"], r["y"], r["z"] = x, y, height(x, y)
    nn = normal(x, y)
    r["nx"], r["ny"], r["nz"] = nn[:, 0], nn[:, 1], nn[:, 2]
    r["count"] = 5
    r["ix"] = np.arange(len(x))
    return r


def surface_mesh(m=41, lo=-0.16, hi=0.16, ylo=None, yhi=None):
    """The surface on an m x m lattice, two triangles per cell, wound to look along +z."""
    ylo, yhi = lo if ylo is None else ylo, hi if yhi is None else yhi
    x, y = np.meshgrid(np.linspace(lo, hi, m), np.linspace(ylo, yhi, m), indexing="ij")
    verts = np.stack([x, y, height(x, y)], axis=-1).reshape(-1, 3).astype(np.float32)
    i, j = (a.ravel() for a in np.meshgrid(np.arange(m - 1), np.arange(m - 1), indexing="ij"))
    a, b, c, d = i * m + j, (i + 1) * m + j, (i + 1) * m + j + 1, i * m + j + 1
    return verts, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.uint32)


def test_reference_converges_on_a_displaced_patch():
    rows = patch_rows()
    verts, tris = surface_mesh()
    # the mesh file is the surface moved by S^-1, so the true mesh -> fusion pose is S; the start pose is the identity
    S = A.rigid(0.8, (0.3, -0.5, 1.0), (0.003, -0.002, 0.0025), A.centre(BBOX))
    S4 = np.vstack([S, [0, 0, 0, 1]])
    moved = (np.hstack([verts.astype(np.float64), np.ones((len(verts), 1))]) @ np.linalg.inv(S4).T)[:, :3].astype(np.float32)
    start = np.eye(4)[:3]
    got = A.align(rows, moved, 12, tris, start, BBOX, max_iterations=30, max_distance=MD, eps_rotation=1e-5, eps_translation=1e-5)
    d0, d1 = A.corner_displacement(start, S, BBOX), A.corner_displacement(got["pose"], S, BBOX)
    print("patch: %d rows, %d iterations, flags %d, inliers %d, rms %.3e -> %.3e, corner displacement %.6f -> %.6f m" % (
        len(rows), got["iterations"], got["flags"], got["inliers"], got["history"][0], got["rms"], d0, d1))
    assert got["flags"] == A.CONVERGED
    assert got["rows_sampled"] == len(rows) and got["inliers"] > len(rows) // 2
    assert got["rms"] < got["history"][0]
    assert d1 < d0
    # sampling: every third row, the same mesh
    s3 = A.align(rows, moved, 12, tris, start, BBOX, max_iterations=30, stride=3, max_distance=MD, eps_rotation=1e-5, eps_translation=1e-5)
    assert s3["rows_sampled"] == (len(rows) + 2) // 3 and s3["flags"] == A.CONVERGED
    assert A.corner_displacement(s3["pose"], S, BBOX) < d0


def test_plane_only_mesh_pins_the_degenerate_path():
    """Two big triangles and rows on the plane with equal normals: J has rank 3, so with damping = 0 the Cholesky must meet a pivot
    that is not > 0 in the first system, and the pose stays T_0 bit for bit."""
    u = np.linspace(-0.1, 0.1, 12)
    x, y = (a.ravel() for a in np.meshgrid(u, u, indexing="ij"))
    r = np.zeros(len(x), D.ROW_DTYPE)
    r["x"], r["y"], r["z"] = x, y, 0.2
    r["nz"] = 1.0
    r["count"] = 1
    quad = np.array([[-1, -1, 0.2], [1, -1, 0.2], [1, 1, 0.2], [-1, 1, 0.2]], np.float32)
    t2 = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    start = A.rigid(0.0, (0, 0, 1), (0, 0, 0.004), (0, 0, 0))
    got = A.align(r, quad, 12, t2, start, BBOX, max_distance=MD, damping=0.0)
    assert got["flags"] == A.DEGENERATE and got["iterations"] == 1 and got["inliers"] == len(r)
    assert got["pose"].tobytes() == np.ascontiguousarray(start, np.float64).tobytes()
    assert abs(got["rms"] - 0.004) < 1e-6
    damped = A.align(r, quad, 12, t2, start, BBOX, max_distance=MD, damping=1e-6)
    assert damped["flags"] == A.CONVERGED and abs(damped["pose"][2, 3]) < 1e-5
    # no triangle in reach: TOO_FEW after one system, the pose untouched
    far = A.rigid(0.0, (0, 0, 1), (0, 0, 0.1), (0, 0, 0))
    none = A.align(r, quad, 12, t2, far, BBOX, max_distance=MD)
    assert none["flags"] == A.TOO_FEW and none["iterations"] == 1 and none["inliers"] == 0 and none["rms"] == 0.0
    assert none["pose"].tobytes() == np.ascontiguousarray(far, np.float64).tobytes()


def test_skip_boundary_drops_rows_past_the_rim_of_a_partial_mesh():
    rows = patch_rows()
    verts, tris = surface_mesh(ylo=-0.16, yhi=0.0)  # covers the rows with y < 0 only
    start = np.eye(4)[:3]
    kw = dict(max_iterations=1, max_distance=MD)
    plain = A.align(rows, verts, 12, tris, start, BBOX, **kw)
    skip = A.align(rows, verts, 12, tris, start, BBOX, flags=A.SKIP_BOUNDARY, **kw)
    print("partial mesh: %d inliers, %d with SKIP_BOUNDARY" % (plain["inliers"], skip["inliers"]))
    assert 0 < skip["inliers"] < plain["inliers"] <= len(rows)


def test_library_exports_the_align_calls(hfpf_mod):
    L = hfpf_mod.lib()
    for name in ("hfpf_align_mesh", "hfpf_align_mesh_device", "hfpf_check_align_opts"):
        assert hasattr(L, name), "libhfpf.so does not export %s" % name
    assert C.sizeof(hfpf_mod.AlignOpts) == 88 and C.sizeof(hfpf_mod.AlignResult) == 424
    assert C.sizeof(hfpf_mod.AlignResult) == C.sizeof(hfpf_mod.TrackResult)


def test_check_align_opts_rejects_each_bad_field(hfpf_mod):
    H = hfpf_mod
    assert H.check_align_opts(H.align_opts()) == 0
    assert H.check_align_opts(H.align_opts(skip_boundary=True, stride=65536, max_iterations=64, damping=0.0, eps_rotation=0.0)) == 0
    assert H.check_align_opts(None) == -2
    nan, inf = float("nan"), float("inf")
    bad = [("struct_size", 80), ("flags", 2), ("flags", 3), ("max_iterations", 0), ("max_iterations", 65), ("stride", 0), ("stride", 65537),
           ("min_inliers", 5), ("reserved0", 1), ("reserved", 1), ("damping", -1.0), ("damping", nan), ("damping", inf),
           ("eps_rotation", -1e-9), ("eps_rotation", nan), ("eps_translation", -1e-9), ("eps_translation", inf)]
    for field, value in bad:
        o = H.align_opts()
        setattr(o, field, value)
        assert H.check_align_opts(o) == -2, (field, value)
    for field, value in [("struct_size", 24), ("flags", 1), ("reserved", 7), ("min_count", nan), ("max_distance", 0.0), ("max_distance", inf),
                         ("max_distance", 1.5)]:
        o = H.align_opts()
        setattr(o.compare, field, value)
        assert H.check_align_opts(o) == -2, ("compare." + field, value)
