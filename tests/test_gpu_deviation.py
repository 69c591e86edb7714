"""GPU: deviation of the fused model from a triangle mesh (hfpf_compare_mesh, hfpf_compare_mesh_device).  The call is defined on the
rows hfpf_extract_filtered returns, so every record and every summary is compared byte for byte with tests/deviation_ref.py run on
those rows: the contract is exact, no tolerance is involved.  The session is the synthetic depth stream of the render tests at 2 mm
with colour, cut to three 160 x 120 frames: the numpy reference against the model's own mesh costs seconds per 10,000 rows (most
of all for the rows with no triangle in reach, which meet every triangle within max_distance), and the 190,000 rows of the twelve
640 x 480 frames would put a minute on each such test while adding bricks, not cases."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import deviation_ref as D
from gpu_support import BBOX, IDENT, RES, compare_device, counters, grid, run, same_deviation, uploaded
from scenes import DepthScene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def session(hfpf_mod, synth_mod):
    sc = DepthScene(3, 160, 120, clean_every=2)
    g = grid(hfpf_mod)
    run(g, sc)
    rows = g.extract().copy()
    verts, tris = g.extract_mesh()
    print("session: %d rows, own mesh %d vertices / %d triangles" % (len(rows), len(verts), len(tris)))
    assert len(rows) > 1000 and len(tris) > 1000
    yield sc, g, rows, verts, tris
    g.close()


# ---- 1. the model's own mesh, without leaving HBM ----------------------------------------------------------------------

@pytest.mark.parametrize("voxels", [3, 20])
def test_own_mesh_device_and_host_forms(hfpf_mod, session, voxels):
    sc, g, rows, verts, tris = session
    md = voxels * RES
    t0 = time.time()
    ref = D.compare(rows, verts, 32, tris, IDENT, 0.0, md)
    print("reference: %.2f s" % (time.time() - t0))
    dv, nv, dt, nt = g.extract_mesh_device()
    try:
        assert nv == len(verts) and nt == len(tris)
        got_rows, dev, s = compare_device(g, hfpf_mod, dv, nv, 32, dt, nt, IDENT, rows=True, max_distance=md)
    finally:
        g.device_free(dv), g.device_free(dt)
    print("own mesh, %d voxels: found %d of %d, max %.6f, rms %.6f" % (voxels, s["n_found"], s["n_rows"], s["max_abs"],
                                                                       (s["sum_sq_q30"] / 2.0 ** 30 / max(1, s["n_found"])) ** 0.5))
    same_deviation((dev, s), ref, "device form, %d voxels" % voxels)
    assert got_rows.tobytes() == rows.tobytes()
    host = g.compare_mesh(verts, tris, IDENT, max_distance=md)
    same_deviation(host, ref, "host form, %d voxels" % voxels)
    # not a fidelity bound (DESIGN.md states the measured figures): the mesh is the rows' own surface, so a compare that finds less than
    # half of them within 3 voxels would be testing the "not found" path only
    assert s["n_found"] > 0.5 * len(rows)
    with_rows = g.compare_mesh(verts, tris, IDENT, rows=True, max_distance=md)
    assert with_rows[0].tobytes() == rows.tobytes() and with_rows[1].tobytes() == host[0].tobytes()


def test_min_count_gates_the_row_set(hfpf_mod, session):
    sc, g, rows, verts, tris = session
    gated = g.extract_filtered(2.0)
    assert 0 < len(gated) < len(rows)
    sv, st = soup(rows, 2000, seed=0x3C)
    got = g.compare_mesh(sv, st, IDENT, min_count=2.0, max_distance=5 * RES)
    same_deviation(got, D.compare(rows, sv, 12, st, IDENT, 2.0, 5 * RES), "min_count 2")
    assert got[1]["n_rows"] == len(gated)


# ---- 2. two huge triangles under an oblique pose -----------------------------------------------------------------------

def test_two_huge_triangles_through_the_box(hfpf_mod, session):
    sc, g, rows, verts, tris = session
    c = np.array([np.median(rows[k]) for k in ("x", "y", "z")], np.float64)
    quad = np.array([[-3, -3, 0], [3, -3, 0], [3, 3, 0], [-3, 3, 0]], np.float32)  # mesh frame: 6 m across, far beyond the box
    a, b = 0.4, 0.3
    R = (np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]]) @
         np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]]))
    pose = np.hstack([R, c.reshape(3, 1)])
    t2 = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    for voxels in (4, 32):
        got = g.compare_mesh(quad, t2, pose, max_distance=voxels * RES)
        same_deviation(got, D.compare(rows, quad, 12, t2, pose, 0.0, voxels * RES), "quad, %d voxels" % voxels)
        print("quad, %d voxels: found %d of %d, negative %d" % (voxels, got[1]["n_found"], len(rows), got[1]["n_negative"]))
        assert 0 < got[1]["n_found"] < len(rows) and 0 < got[1]["n_negative"] < got[1]["n_found"]
        assert set(np.unique(got[0]["tri"])) == {0, 1, D.NO_TRI}


# ---- 3. a soup near the surface, with every invalid kind -----------------------------------------------------------------

def soup(rows, n=5000, seed=0x50FA):
    rng = np.random.default_rng(seed)
    P = np.stack([rows[k] for k in ("x", "y", "z")], axis=1).astype(np.float64)
    c = P[rng.integers(0, len(P), n)] + rng.uniform(-0.01, 0.01, (n, 3))
    edge = rng.uniform(0.001, 0.03, (n, 1, 1))
    verts = (c[:, None, :] + rng.uniform(-0.5, 0.5, (n, 3, 3)) * edge).reshape(-1, 3).astype(np.float32)
    tris = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    kinds = rng.permutation(n)[:200].reshape(4, 50)
    tris[kinds[0], 1] = tris[kinds[0], 0]                               # a repeated vertex
    k1 = kinds[1]                                                       # collinear, exactly: A on a 2^-10 lattice, B = A + d, C = A + 2 d
    base = np.round(verts[tris[k1, 0]].astype(np.float64) * 1024) / 1024
    step = np.array([1, 2, 3]) / 1024
    verts[tris[k1, 0]], verts[tris[k1, 1]], verts[tris[k1, 2]] = base, base + step, base + 2 * step
    verts[tris[kinds[2], 0], 1] = np.nan                                # a NaN vertex
    tris[kinds[3][:25], 2] = 3 * n + rng.integers(0, 1000, 25)          # indices out of range
    tris[kinds[3][25:], 0] = 0xFFFFFFFF
    return verts, tris


def test_soup_with_invalid_triangles(hfpf_mod, session):
    sc, g, rows, verts, tris = session
    sv, st = soup(rows)
    for voxels in (5, 16):
        ref = D.compare(rows, sv, 12, st, IDENT, 0.0, voxels * RES)
        got = g.compare_mesh(sv, st, IDENT, max_distance=voxels * RES)
        print("soup, %d voxels: found %d of %d, invalid %d" % (voxels, got[1]["n_found"], len(rows), got[1]["n_tris_invalid"]))
        same_deviation(got, ref, "soup, %d voxels" % voxels)
        assert got[1]["n_tris_invalid"] == 200 and got[1]["n_tris_valid"] == 4800 and got[1]["n_found"] > 0
    flags = got[0]["flags"][(got[0]["flags"] & 1) != 0]
    assert {1, 3, 5} == set(np.unique(flags)), "face, edge and vertex regions all occur"


# ---- 4. a crowd in one brick across LDS tiles, and a snapshot restored into a second handle --------------------------------

def crowd(rows, n=600, seed=0xC0D):
    rng = np.random.default_rng(seed)
    lo = np.asarray(BBOX, np.float64)[0::2]
    P = np.stack([rows[k] for k in ("x", "y", "z")], axis=1).astype(np.float64)
    brick = np.floor((P - lo) / (8 * RES)).astype(np.int64)
    keys, counts = np.unique(brick, axis=0, return_counts=True)
    b = keys[np.argmax(counts)]  # the fullest brick
    verts = (lo + (b + rng.uniform(0.1, 0.9, (n, 1, 3))) * 8 * RES)[:, :, :] + rng.uniform(-0.002, 0.002, (n, 3, 3))
    return verts.reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.uint32).reshape(n, 3), int(counts.max())


def test_crowd_across_tiles_and_after_a_restore(hfpf_mod, session):
    sc, g, rows, verts, tris = session
    cv, ct, in_brick = crowd(rows)
    md = 6 * RES
    ref = D.compare(rows, cv, 12, ct, IDENT, 0.0, md)
    got = g.compare_mesh(cv, ct, IDENT, max_distance=md)
    print("crowd: %d rows in the brick, found %d" % (in_brick, got[1]["n_found"]))
    same_deviation(got, ref, "crowd, default tile")
    assert got[1]["n_found"] >= in_brick // 2
    own = g.compare_mesh(verts, tris, IDENT, max_distance=3 * RES)
    blob = g.snapshot()
    os.environ["HFPF_TEST_DEV_TILE"] = "32"
    try:
        g2 = grid(hfpf_mod)
    finally:
        del os.environ["HFPF_TEST_DEV_TILE"]
    try:
        g2.restore(blob)
        same_deviation(g2.compare_mesh(cv, ct, IDENT, max_distance=md), got, "crowd, tile 32, restored handle")
        same_deviation(g2.compare_mesh(verts, tris, IDENT, max_distance=3 * RES), own, "own mesh, tile 32, restored handle")
    finally:
        g2.close()


# ---- 5. empty and edge cases ---------------------------------------------------------------------------------------------

def _not_found(dev):
    assert (dev["flags"] == 0).all() and (dev["tri"] == D.NO_TRI).all() and not dev["reserved"].any()
    for k in ("distance", "signed_distance", "q"):
        assert (dev[k].view(np.uint32) == D.NAN_BITS).all()


def test_empty_and_edge_cases_leave_the_handle_usable(hfpf_mod, session):
    H = hfpf_mod
    sc, g, rows, verts, tris = session
    tri1 = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32))
    dev, s = g.compare_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32), IDENT)
    assert len(dev) == len(rows) and s["n_found"] == 0 and s["n_tris_valid"] == 0 and s["max_abs"] == 0.0 and s["sum_abs_q30"] == 0
    _not_found(dev)
    far = np.hstack([np.eye(3), [[50.0], [50.0], [50.0]]])
    dev, s = g.compare_mesh(*tri1, far, max_distance=32 * RES)
    assert len(dev) == len(rows) and s["n_found"] == 0 and s["n_tris_valid"] == 1
    _not_found(dev)
    dev, s = g.compare_mesh(verts, tris, IDENT, min_count=1e9)
    assert len(dev) == 0 and s["n_rows"] == 0 and s["n_found"] == 0 and s["n_tris_valid"] + s["n_tris_invalid"] == len(tris)
    r, d, nr, s = g.compare_mesh(0, 0, IDENT, device=True, rows=True, n_verts=0, vertex_stride=12, n_tris=0, min_count=1e9)
    assert (r, d, nr) == (0, 0, 0)
    with grid(H) as fresh:
        dev, s = fresh.compare_mesh(*tri1, IDENT)
        assert len(dev) == 0 and s["n_rows"] == 0 and s["n_tris_valid"] == 1
        sc.integrate(fresh, 0)  # points, but no clean pass yet
        dev, s = fresh.compare_mesh(*tri1, IDENT)
        assert len(dev) == 0 and s["n_rows"] == 0
    # every BAD_ARG of include/hfpf.h
    L, h = H.lib(), g._h
    v, t = np.ascontiguousarray(tri1[0]), np.ascontiguousarray(tri1[1])
    pose = np.ascontiguousarray(IDENT, np.float64).reshape(12)
    out = dict(r=C.c_void_p(), d=C.c_void_p(), n=C.c_uint64(), s=H.DeviationSummary())
    dv, dt = g.device_alloc(64), g.device_alloc(64)

    def call(o=None, verts=v.ctypes.data, n_verts=3, stride=12, tris=t.ctypes.data, n_tris=1, pose=pose.ctypes.data, dev=True, n=True, s=True, device=False):
        o = o if o is not None else H.deviation_opts()
        fn = L.hfpf_compare_mesh_device if device else L.hfpf_compare_mesh
        return fn(h, C.byref(o), verts, n_verts, stride, tris, n_tris, pose, C.byref(out["r"]), C.byref(out["d"]) if dev else None,
                  C.byref(out["n"]) if n else None, C.byref(out["s"]) if s else None)

    def opts(**kw):
        o = H.deviation_opts()
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    bad_pose = pose.copy()
    bad_pose[7] = np.inf
    try:
        faults = [dict(o=opts(max_distance=33 * RES)), dict(o=opts(struct_size=24)), dict(o=opts(flags=2)), dict(o=opts(reserved=7)),
                  dict(o=opts(min_count=float("nan"))), dict(o=opts(max_distance=0.0)), dict(o=opts(max_distance=float("inf"))),
                  dict(pose=None), dict(pose=bad_pose.ctypes.data), dict(stride=8), dict(stride=14), dict(verts=None), dict(tris=None),
                  dict(n_verts=2 ** 32 - 1), dict(n_tris=2 ** 32 - 1), dict(dev=False), dict(n=False), dict(s=False),
                  dict(device=True, verts=dv + 2, tris=dt), dict(device=True, verts=dv, tris=dt + 1)]
        for kw in faults:
            assert call(**kw) == -2, kw
            assert out["d"].value is None and out["n"].value == 0, "a rejected call writes nothing"
        assert call(o=opts(max_distance=32 * RES)) == 0  # the bound itself is legal
        L.hfpf_free_deviation(out["r"], out["d"])
    finally:
        g.device_free(dv), g.device_free(dt)
    assert g.extract().tobytes() == rows.tobytes()


def test_both_forms_return_the_documented_empties(hfpf_mod, session):
    """A mesh without triangles, a gate no row passes and an empty handle: the same arrays and the same summary out of either form."""
    sc, g, rows, verts, tris = session
    none = g.compare_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32), IDENT, rows=True)
    dev = compare_device(g, hfpf_mod, 0, 0, 12, 0, 0, IDENT, rows=True)
    assert none[0].tobytes() == dev[0].tobytes() == rows.tobytes() and none[1].tobytes() == dev[1].tobytes() and none[2] == dev[2]
    assert none[2]["n_rows"] == len(rows) and none[2]["n_found"] == 0 and none[2]["n_tris_valid"] == none[2]["n_tris_invalid"] == 0
    _not_found(none[1])
    with grid(hfpf_mod) as fresh:
        for h, kw, what in ((g, dict(min_count=1e9), "no row passes the gate"), (fresh, dict(), "an empty handle")):
            host = h.compare_mesh(verts, tris, IDENT, rows=True, **kw)
            with uploaded(h, verts, tris) as (hv, ht):
                r, d, nr, s = h.compare_mesh(hv, ht, IDENT, device=True, rows=True, n_verts=len(verts), vertex_stride=32, n_tris=len(tris), **kw)
            assert (r, d, nr) == (0, 0, 0) and len(host[0]) == len(host[1]) == 0 and s == host[2], what
            assert s["n_rows"] == s["n_found"] == 0 and s["n_tris_valid"] + s["n_tris_invalid"] == len(tris), what


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_every_rejection_leaves_the_outputs_untouched(hfpf_mod, session, device):
    """Every HFPF_ERR_BAD_ARG of either form, with each output preset to a sentinel and compared after the call."""
    H = hfpf_mod
    sc, g, rows, verts, tris = session
    L = H.lib()
    v, t = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32)
    pose = np.ascontiguousarray(IDENT, np.float64).reshape(12)
    bad_pose = pose.copy()
    bad_pose[7] = np.inf
    fn = L.hfpf_compare_mesh_device if device else L.hfpf_compare_mesh

    def opts(**kw):
        o = H.deviation_opts()
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    with uploaded(g, v, t) as (dv, dt):
        mv, mt = (dv, dt) if device else (v.ctypes.data, t.ctypes.data)

        def call(o=None, verts=mv, n_verts=3, stride=12, tris=mt, n_tris=1, pose=pose.ctypes.data, rows=True, dev=True, n=True, s=True):
            o = o if o is not None else H.deviation_opts()
            out = dict(r=C.c_void_p(0x5A), d=C.c_void_p(0x5A), n=C.c_uint64(0x5A), s=H.DeviationSummary())
            C.memset(C.byref(out["s"]), 0x5A, C.sizeof(out["s"]))
            rc = fn(g._h, C.byref(o), verts, n_verts, stride, tris, n_tris, pose, C.byref(out["r"]) if rows else None, C.byref(out["d"]) if dev else None,
                    C.byref(out["n"]) if n else None, C.byref(out["s"]) if s else None)
            untouched = (out["r"].value, out["d"].value, out["n"].value) == (0x5A, 0x5A, 0x5A) and bytes(out["s"]) == b"\x5a" * C.sizeof(out["s"])
            return rc, untouched, out

        faults = [dict(o=opts(max_distance=33 * RES)), dict(o=opts(struct_size=24)), dict(o=opts(flags=2)), dict(o=opts(reserved=7)),
                  dict(o=opts(min_count=float("nan"))), dict(o=opts(max_distance=0.0)), dict(o=opts(max_distance=float("inf"))),
                  dict(pose=None), dict(pose=bad_pose.ctypes.data), dict(stride=8), dict(stride=14), dict(verts=None), dict(tris=None),
                  dict(n_verts=2 ** 32 - 1), dict(n_tris=2 ** 32 - 1), dict(dev=False), dict(n=False), dict(s=False)]
        if device:
            faults += [dict(verts=dv + 2), dict(tris=dt + 1)]
        for kw in faults:
            rc, untouched, _ = call(**kw)
            assert rc == -2 and untouched, kw
        rc, untouched, out = call(rows=False)  # and the unspoiled call works on the same handle, without the optional rows
        assert rc == 0 and not untouched and out["r"].value == 0x5A and out["n"].value == len(rows) == out["s"].n_rows
        if device:
            g.device_free(out["d"].value)
        else:
            L.hfpf_free_deviation(None, out["d"])
    assert g.extract().tobytes() == rows.tobytes()


# ---- 6. a compare is read-only -------------------------------------------------------------------------------------------

def test_compare_is_read_only_and_timed(hfpf_mod, session):
    sc, g, rows, verts, tris = session
    before = (counters(g), g.extract().tobytes(), g.occupied().tobytes())
    g.kernel_timing(True)
    try:
        g.compare_mesh(verts, tris, IDENT, max_distance=3 * RES)
        ms, n = g.kernel_time(7)
    finally:
        g.kernel_timing(False)
    assert n == 1 and ms > 0
    assert (counters(g), g.extract().tobytes(), g.occupied().tobytes()) == before
