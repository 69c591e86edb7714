"""GPU: coverage of a triangle mesh by the fused model (hfpf_cover_mesh, hfpf_cover_mesh_device).  The call is defined on the rows
hfpf_extract returns and the cells hfpf_get_occupied lists, so every record and every summary is compared byte for byte with
tests/cover_ref.py run on those: the contract is exact, no tolerance is involved.  The session is the one of the deviation tests
(three 160 x 120 synthetic depth frames at 2 mm), and every mesh is cut so that the numpy reference sees some ten thousands of
samples."""
import ctypes as C

import numpy as np
import pytest

import cover_ref as V
from gpu_support import IDENT, RES, counters, cover_device, coverage_sums, grid, run, same_coverage, uploaded
from scenes import DepthScene

pytestmark = pytest.mark.gpu
OWN = 4000  # triangles of the model's own mesh that are covered


@pytest.fixture(scope="module")
def session(hfpf_mod, synth_mod):
    sc = DepthScene(3, 160, 120, clean_every=2)
    g = grid(hfpf_mod)
    run(g, sc)
    rows = g.extract().copy()
    occ = g.occupied().copy()
    verts, tris = g.extract_mesh()
    print("session: %d rows, own mesh %d vertices / %d triangles" % (len(rows), len(verts), len(tris)))
    assert len(rows) > 1000 and len(tris) > OWN
    yield sc, g, rows, occ, verts, tris
    g.close()


def _ref(g, rows, occ, verts, stride, tris, pose, **kw):
    return V.cover(rows, occ, verts, stride, tris, pose, tuple(g.cfg.bbox), g.dims[1], **kw)


# ---- 1. the model's own mesh, without leaving HBM ----------------------------------------------------------------------

@pytest.mark.parametrize("voxels", [1.0, 0.5])
def test_own_mesh_device_and_host_forms(hfpf_mod, session, voxels):
    sc, g, rows, occ, verts, tris = session
    kw = dict(radius=2, max_distance=2 * RES, spacing=voxels * RES)
    ref = _ref(g, rows, occ, verts, 32, tris[:OWN], IDENT, **kw)
    dv, nv, dt, nt = g.extract_mesh_device()
    try:
        assert nv == len(verts) and nt == len(tris)
        dev = cover_device(g, hfpf_mod, dv, nv, 32, dt, OWN, IDENT, **kw)
    finally:
        g.device_free(dv), g.device_free(dt)
    s = dev[1]
    print("own mesh, spacing %.1f voxels: %d samples, %d covered, area %.6f m^2, covered %.6f m^2" % (voxels, s["n_samples"], s["n_covered"], s["area"],
                                                                                                     s["covered_area"]))
    same_coverage(dev, ref, "device form, spacing %.1f" % voxels)
    host = g.cover_mesh(verts, tris[:OWN], IDENT, **kw)
    same_coverage(host, ref, "host form, spacing %.1f" % voxels)
    assert host[0].tobytes() == dev[0].tobytes() and host[1] == dev[1]
    assert s["n_covered"] > 0 and s["n_samples"] >= OWN - s["n_tris_invalid"] and s["n_samples"] < 70000
    coverage_sums(*dev)
    assert 0.0 < s["covered_area"] <= s["area"]


# ---- 2. two huge triangles through the box -----------------------------------------------------------------------------

def _plane_quad():
    """Two triangles, 1.6 m across, on the synthetic scene's back plane z = 0.56 + 0.05 x (hfpf_synth), turned 0.4 rad in that plane:
    they leave the 1 m box on every side, and inside it they run along the rows of the back plane wherever the sphere and the box of
    the scene do not hide it."""
    quad = np.array([[-0.8, -0.8, 0], [0.8, -0.8, 0], [0.8, 0.8, 0], [-0.8, 0.8, 0]], np.float32)
    a, b = 0.4, np.arctan(0.05)
    R = (np.array([[np.cos(b), 0, -np.sin(b)], [0, 1, 0], [np.sin(b), 0, np.cos(b)]]) @  # z -> the plane's normal (-0.05, 0, 1) / |.|
         np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]]))
    return quad, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.hstack([R, [[0.0], [0.0], [0.56]]])


@pytest.mark.parametrize("max_subdivision", [64, 5])
def test_two_huge_triangles_through_the_box(hfpf_mod, session, max_subdivision):
    sc, g, rows, occ, verts, tris = session
    quad, t2, pose = _plane_quad()
    kw = dict(radius=2, max_distance=2 * RES, spacing=RES, max_subdivision=max_subdivision)
    got = g.cover_mesh(quad, t2, pose, **kw)
    cov, s = got
    print("quad, cap %d: %d samples, %d in the box, %d covered" % (max_subdivision, s["n_samples"], s["n_in_bbox"], s["n_covered"]))
    same_coverage(got, _ref(g, rows, occ, quad, 12, t2, pose, **kw), "quad, cap %d" % max_subdivision)
    assert (cov["flags"] == V.VALID | V.CAPPED).all() and (cov["n_samples"] == max_subdivision ** 2).all()
    assert 0 < s["n_covered"] < s["n_samples"] and s["n_in_bbox"] < s["n_samples"]
    coverage_sums(cov, s)


# ---- 3. a mixed soup: every n, every lane position of a triangle boundary, every invalid kind ----------------------------

def soup(rows, pose, n=777, seed=0x50FA):
    """Triangles of the mesh frame that `pose` carries to within two voxels of a row's point each (seeded as the deviation tests' soup)."""
    rng = np.random.default_rng(seed)
    P = np.stack([rows[k] for k in ("x", "y", "z")], axis=1).astype(np.float64)
    c = P[rng.integers(0, len(P), n)] + rng.uniform(-0.004, 0.004, (n, 3))
    c = (c - pose[:, 3]) @ pose[:, :3]  # R^T (c - t)
    edge = RES * np.exp(rng.uniform(np.log(0.2), np.log(40.0), (n, 1, 1)))  # 0.2 to 40 voxels, log-uniform: most triangles are small
    verts = (c[:, None, :] + rng.uniform(-0.5, 0.5, (n, 3, 3)) * edge).reshape(-1, 3).astype(np.float32)
    tris = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    kinds = rng.permutation(n)[:78].reshape(3, 26)
    tris[kinds[0][:13], 2] = 3 * n + rng.integers(0, 1000, 13)          # indices out of range
    tris[kinds[0][13:], 0] = 0xFFFFFFFF
    verts[tris[kinds[1], 1], 2] = np.nan                                # a NaN vertex
    tris[kinds[2], 1] = tris[kinds[2], 0]                               # zero area: a repeated vertex
    return verts, tris


def _rigid():
    a, b = 0.02, -0.015
    R = (np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]]) @
         np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]]))
    return np.hstack([R, [[0.003], [-0.002], [0.004]]])


def test_mixed_soup_with_invalid_triangles(hfpf_mod, session):
    sc, g, rows, occ, verts, tris = session
    pose = _rigid()
    sv, st = soup(rows, pose)
    kw = dict(radius=2, max_distance=2 * RES, spacing=RES, max_subdivision=24)
    ref = _ref(g, rows, occ, sv, 12, st, pose, **kw)
    got = g.cover_mesh(sv, st, pose, **kw)
    cov, s = got
    n = np.sqrt(cov["n_samples"]).astype(int)
    print("soup: %d samples, %d in the box, %d covered, %d invalid, n from %d to %d, %d capped" % (
        s["n_samples"], s["n_in_bbox"], s["n_covered"], s["n_tris_invalid"], n[n > 0].min(), n.max(), int(((cov["flags"] & V.CAPPED) != 0).sum())))
    same_coverage(got, ref, "soup")
    coverage_sums(cov, s)
    assert s["n_tris_invalid"] == 78 and s["n_tris_valid"] == 777 - 78
    assert n[n > 0].min() == 1 and n.max() == 24 and ((cov["flags"] & V.CAPPED) != 0).any() and len(np.unique(n)) > 12
    assert 0 < s["n_covered"] < s["n_in_bbox"] <= s["n_samples"] < 150000
    # triangle boundaries at every lane position of a wave
    first = np.cumsum(cov["n_samples"].astype(np.int64)) - cov["n_samples"]
    assert len(np.unique(first[cov["n_samples"] > 0] % 64)) == 64
    with uploaded(g, sv, st) as (dsv, dst):
        same_coverage(cover_device(g, hfpf_mod, dsv, len(sv), 12, dst, len(st), pose, **kw), ref, "soup, device form")


# ---- 4. the normal gate ------------------------------------------------------------------------------------------------

def test_normal_gate_on_the_reversed_own_mesh(hfpf_mod, session):
    sc, g, rows, occ, verts, tris = session
    back = np.ascontiguousarray(tris[:OWN, ::-1])
    base = dict(radius=2, max_distance=2 * RES, spacing=RES)
    res = {}
    for name, kw in (("off", dict(min_normal_dot=-2.0)), ("gate", dict(min_normal_dot=0.5)), ("abs", dict(min_normal_dot=0.5, abs_normal=True))):
        for winding, tt in (("own", tris[:OWN]), ("reversed", back)):
            got = g.cover_mesh(verts, tt, IDENT, **base, **kw)
            same_coverage(got, _ref(g, rows, occ, verts, 32, tt, IDENT, **base, **kw), "%s, %s winding" % (name, winding))
            res[name, winding] = got[1]["n_covered"]
    print("normal gate: %r" % res)
    for winding in ("own", "reversed"):  # each gate passes a subset of the next
        assert res["gate", winding] <= res["abs", winding] <= res["off", winding] and res["off", winding] > 0
    assert res["gate", "own"] != res["gate", "reversed"], "the gate tells the two windings apart"


# ---- 5. the count gate -------------------------------------------------------------------------------------------------

def test_min_count_above_the_median(hfpf_mod, session):
    sc, g, rows, occ, verts, tris = session
    mc = float(np.median(rows["count"])) + 1.0
    kw = dict(radius=2, max_distance=2 * RES, spacing=RES)
    all_rows = g.cover_mesh(verts, tris[:OWN], IDENT, **kw)
    got = g.cover_mesh(verts, tris[:OWN], IDENT, min_count=mc, **kw)
    same_coverage(got, _ref(g, rows, occ, verts, 32, tris[:OWN], IDENT, min_count=mc, **kw), "min_count %.0f" % mc)
    assert got[0].tobytes() != all_rows[0].tobytes() and 0 < got[1]["n_covered"] < all_rows[1]["n_covered"]


# ---- 6. the own mesh, ten voxels off ---------------------------------------------------------------------------------------

def test_translated_mesh_is_not_covered(hfpf_mod, session):
    sc, g, rows, occ, verts, tris = session
    pose = np.hstack([np.eye(3), [[0.0], [0.0], [10 * RES]]])
    kw = dict(radius=2, max_distance=1.0, spacing=RES)
    got = g.cover_mesh(verts, tris[:OWN], pose, **kw)
    same_coverage(got, _ref(g, rows, occ, verts, 32, tris[:OWN], pose, **kw), "ten voxels along +z")
    here = g.cover_mesh(verts, tris[:OWN], IDENT, **kw)
    cov, s = got
    assert s["n_covered"] == 0 and s["sum_dist_q30"] == 0 and s["max_distance"] == 0.0 and s["covered_q40_lo"] == 0 and s["covered_q40_hi"] == 0
    for k in ("n_samples", "flags", "area"):
        assert cov[k].tobytes() == here[0][k].tobytes(), k
    assert s["n_in_bbox"] > 0 and (s["area_q40_lo"], s["area_q40_hi"]) == (here[1]["area_q40_lo"], here[1]["area_q40_hi"])


# ---- 7. empty and edge cases ---------------------------------------------------------------------------------------------

def test_empty_and_edge_cases_leave_the_handle_usable(hfpf_mod, session):
    H = hfpf_mod
    sc, g, rows, occ, verts, tris = session
    c = [float(np.median(rows[k])) for k in ("x", "y", "z")]
    tri1 = (np.array([c, [c[0] + 0.01, c[1], c[2]], [c[0], c[1] + 0.01, c[2]]], np.float32), np.array([[0, 1, 2]], np.uint32))
    zero = {k: 0 for k in V.SUMMARY_KEYS}
    cov, s = g.cover_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32), IDENT)
    assert len(cov) == 0 and {k: s[k] for k in V.SUMMARY_KEYS} == zero and s["area"] == 0.0 and s["covered_area"] == 0.0
    ptr, s = g.cover_mesh(0, 0, IDENT, device=True, n_verts=0, vertex_stride=12, n_tris=0)
    assert ptr == 0 and {k: s[k] for k in V.SUMMARY_KEYS} == zero
    kw = dict(radius=2, max_distance=2 * RES, spacing=RES)
    with grid(H) as fresh:
        no_rows, no_occ = np.zeros(0, H.ROW_DTYPE), np.zeros((0, 3), np.int32)
        ref = V.cover(no_rows, no_occ, tri1[0], 12, tri1[1], IDENT, tuple(fresh.cfg.bbox), fresh.dims[1], **kw)
        got = fresh.cover_mesh(*tri1, IDENT, **kw)
        same_coverage(got, ref, "a fresh handle")
        assert got[0]["n_in_bbox"][0] == got[0]["n_samples"][0] > 1 and got[1]["n_covered"] == 0 and got[1]["n_tris_valid"] == 1
        sc.integrate(fresh, 0)  # points, but no clean pass yet
        same_coverage(fresh.cover_mesh(*tri1, IDENT, **kw), ref, "frames but no clean pass")
    # every BAD_ARG of include/hfpf.h
    L, h = H.lib(), g._h
    v, t = np.ascontiguousarray(tri1[0]), np.ascontiguousarray(tri1[1])
    pose = np.ascontiguousarray(IDENT, np.float64).reshape(12)
    out = dict(c=C.c_void_p(), s=H.CoverageSummary())
    C.memset(C.byref(out["s"]), 0xAB, C.sizeof(out["s"]))
    untouched = bytes(out["s"])
    dv, dt = g.device_alloc(64), g.device_alloc(64)

    def call(o=None, verts=v.ctypes.data, n_verts=3, stride=12, tris=t.ctypes.data, n_tris=1, pose=pose.ctypes.data, cov=True, s=True, device=False):
        o = o if o is not None else H.cover_opts(**kw)
        fn = L.hfpf_cover_mesh_device if device else L.hfpf_cover_mesh
        return fn(h, C.byref(o), verts, n_verts, stride, tris, n_tris, pose, C.byref(out["c"]) if cov else None, C.byref(out["s"]) if s else None)

    def opts(**fields):
        o = H.cover_opts(**kw)
        for k, val in fields.items():
            setattr(o, k, val)
        return o

    bad_pose = pose.copy()
    bad_pose[7] = np.inf
    try:
        faults = [dict(o=opts(struct_size=48)), dict(o=opts(flags=2)), dict(o=opts(reserved=7)), dict(o=opts(radius=0)), dict(o=opts(radius=5)),
                  dict(o=opts(max_subdivision=0)), dict(o=opts(max_subdivision=65)), dict(o=opts(min_count=float("nan"))),
                  dict(o=opts(max_distance=0.0)), dict(o=opts(max_distance=1.5)), dict(o=opts(max_distance=float("inf"))),
                  dict(o=opts(spacing=0.0)), dict(o=opts(spacing=float("inf"))), dict(o=opts(min_normal_dot=-2.5)), dict(o=opts(min_normal_dot=1.5)),
                  dict(o=opts(min_normal_dot=float("nan"))),
                  dict(pose=None), dict(pose=bad_pose.ctypes.data), dict(stride=8), dict(stride=14), dict(verts=None), dict(tris=None),
                  dict(n_verts=2 ** 32 - 1), dict(n_tris=2 ** 32 - 1), dict(cov=False), dict(s=False),
                  dict(device=True, verts=dv + 2, tris=dt), dict(device=True, verts=dv, tris=dt + 1)]
        for f in faults:
            assert call(**f) == -2, f
            assert out["c"].value is None and bytes(out["s"]) == untouched, "a rejected call writes nothing"
        assert call() == 0 and out["c"].value and out["s"].n_tris_valid == 1  # the handle is still usable
        L.hfpf_free_coverage(out["c"])
    finally:
        g.device_free(dv), g.device_free(dt)
    assert g.extract().tobytes() == rows.tobytes()


def test_both_forms_return_the_documented_empties(hfpf_mod, session):
    """A mesh without triangles (vertices or none) and an empty handle: the same records and the same summary out of either form."""
    sc, g, rows, occ, verts, tris = session
    kw = dict(radius=2, max_distance=2 * RES, spacing=RES)
    no_tris = np.zeros((0, 3), np.uint32)
    with uploaded(g, verts) as (dv,):
        pairs = [(g.cover_mesh(verts, no_tris, IDENT, **kw), g.cover_mesh(dv, 0, IDENT, device=True, n_verts=len(verts), vertex_stride=32, n_tris=0, **kw)),
                 (g.cover_mesh(np.zeros((0, 3), np.float32), no_tris, IDENT), g.cover_mesh(0, 0, IDENT, device=True, n_verts=0, vertex_stride=12, n_tris=0))]
    for host, dev in pairs:
        assert len(host[0]) == 0 and dev[0] == 0 and host[1] == dev[1] and all(x == 0 for x in host[1].values())
    c = [float(np.median(rows[k])) for k in ("x", "y", "z")]
    tv = np.array([c, [c[0] + 0.01, c[1], c[2]], [c[0], c[1] + 0.01, c[2]], [c[0], c[1], c[2] + 0.01]], np.float32)
    tt = np.array([[0, 1, 2], [0, 1, 3], [1, 1, 2]], np.uint32)  # the last one is invalid
    with grid(hfpf_mod) as fresh:
        ref = V.cover(np.zeros(0, hfpf_mod.ROW_DTYPE), np.zeros((0, 3), np.int32), tv, 12, tt, IDENT, tuple(fresh.cfg.bbox), fresh.dims[1], **kw)
        host = fresh.cover_mesh(tv, tt, IDENT, **kw)
        with uploaded(fresh, tv, tt) as (dv, dt):
            dev = cover_device(fresh, hfpf_mod, dv, len(tv), 12, dt, len(tt), IDENT, **kw)
        same_coverage(host, ref, "an empty handle, host form")
        assert host[0].tobytes() == dev[0].tobytes() and host[1] == dev[1] and host[1]["n_covered"] == 0 < host[1]["n_in_bbox"]


def test_every_rejection_of_the_device_form_leaves_the_outputs_untouched(hfpf_mod, session):
    """The BAD_ARGs of test_empty_and_edge_cases_leave_the_handle_usable again, through hfpf_cover_mesh_device on a mesh in HBM."""
    H = hfpf_mod
    sc, g, rows, occ, verts, tris = session
    L = H.lib()
    kw = dict(radius=2, max_distance=2 * RES, spacing=RES)
    c = [float(np.median(rows[k])) for k in ("x", "y", "z")]
    v, t = np.array([c, [c[0] + 0.01, c[1], c[2]], [c[0], c[1] + 0.01, c[2]]], np.float32), np.array([[0, 1, 2]], np.uint32)
    pose = np.ascontiguousarray(IDENT, np.float64).reshape(12)
    bad_pose = pose.copy()
    bad_pose[7] = np.inf
    out = dict(c=C.c_void_p(0x5A), s=H.CoverageSummary())
    C.memset(C.byref(out["s"]), 0x5A, C.sizeof(out["s"]))
    untouched = bytes(out["s"])

    def opts(**fields):
        o = H.cover_opts(**kw)
        for k, val in fields.items():
            setattr(o, k, val)
        return o

    with uploaded(g, v, t) as (dv, dt):
        def call(o=None, verts=dv, n_verts=3, stride=12, tris=dt, n_tris=1, pose=pose.ctypes.data, cov=True, s=True):
            o = o if o is not None else H.cover_opts(**kw)
            return L.hfpf_cover_mesh_device(g._h, C.byref(o), verts, n_verts, stride, tris, n_tris, pose, C.byref(out["c"]) if cov else None,
                                            C.byref(out["s"]) if s else None)

        faults = [dict(o=opts(struct_size=48)), dict(o=opts(flags=2)), dict(o=opts(reserved=7)), dict(o=opts(radius=0)), dict(o=opts(radius=5)),
                  dict(o=opts(max_subdivision=0)), dict(o=opts(max_subdivision=65)), dict(o=opts(min_count=float("nan"))),
                  dict(o=opts(max_distance=0.0)), dict(o=opts(max_distance=1.5)), dict(o=opts(max_distance=float("inf"))),
                  dict(o=opts(spacing=0.0)), dict(o=opts(spacing=float("inf"))), dict(o=opts(min_normal_dot=-2.5)), dict(o=opts(min_normal_dot=1.5)),
                  dict(o=opts(min_normal_dot=float("nan"))),
                  dict(pose=None), dict(pose=bad_pose.ctypes.data), dict(stride=8), dict(stride=14), dict(verts=None), dict(tris=None),
                  dict(n_verts=2 ** 32 - 1), dict(n_tris=2 ** 32 - 1), dict(cov=False), dict(s=False), dict(verts=dv + 2), dict(tris=dt + 1)]
        for f in faults:
            assert call(**f) == -2, f
            assert out["c"].value == 0x5A and bytes(out["s"]) == untouched, "a rejected call writes nothing: %r" % (f,)
        assert call() == 0 and out["c"].value not in (None, 0x5A) and out["s"].n_tris_valid == 1  # the handle is still usable
        g.device_free(out["c"].value)
    assert g.extract().tobytes() == rows.tobytes()


# ---- 8. a cover is read-only, and a restored handle answers the same ---------------------------------------------------------

def test_cover_is_read_only_and_survives_a_restore(hfpf_mod, session):
    sc, g, rows, occ, verts, tris = session
    sv, st = soup(rows, _rigid())
    kw = dict(radius=2, max_distance=2 * RES, spacing=RES, max_subdivision=24, min_normal_dot=0.2)
    before = (counters(g), g.extract().tobytes(), g.occupied().tobytes())
    own = g.cover_mesh(verts, tris[:OWN], IDENT, **kw)
    mixed = g.cover_mesh(sv, st, _rigid(), **kw)
    assert (counters(g), g.extract().tobytes(), g.occupied().tobytes()) == before
    blob = g.snapshot()
    with grid(hfpf_mod) as g2:
        g2.restore(blob)
        for got, want, what in ((g2.cover_mesh(verts, tris[:OWN], IDENT, **kw), own, "own mesh"), (g2.cover_mesh(sv, st, _rigid(), **kw), mixed, "soup")):
            assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1], "%s on the restored handle" % what
