"""GPU: best-fitting a triangle mesh to the fused model (hfpf_align_mesh, hfpf_align_mesh_device).  The call is defined on the rows
hfpf_extract_filtered returns, so every field of the result is compared with tests/align_ref.py run on those rows, the pose and the
information matrix byte for byte: the contract is exact, no tolerance is involved.  The session is test_gpu_deviation.py's (three
160 x 120 depth frames at 2 mm) and the mesh is the model's own, started from a pose a few tenths of a degree and 1.5 voxels off."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import align_ref as A
from gpu_support import (ALIGN_KW, ALIGN_MD, ALIGN_START, BBOX, DEPTH_CAPS, IDENT, RES, align_device, counters, deviation_csv,
                         deviation_summary_csv, fitted, grid, node_feed, node_grid, run, same_align, same_deviation, uploaded)
from scenes import DepthScene

pytestmark = pytest.mark.gpu
_REF = {}


@pytest.fixture(scope="module")
def session(hfpf_mod, synth_mod):
    """The session of test_gpu_deviation.py."""
    sc = DepthScene(3, 160, 120, clean_every=2)
    g = grid(hfpf_mod)
    run(g, sc)
    rows = g.extract().copy()
    verts, tris = g.extract_mesh()
    print("session: %d rows, own mesh %d vertices / %d triangles" % (len(rows), len(verts), len(tris)))
    assert len(rows) > 1000 and len(tris) > 1000
    yield sc, g, rows, verts, tris
    g.close()


def _ref(rows, verts, tris, stride=1, flags=0):
    """align_ref on the session's own mesh from ALIGN_START, computed once per (stride, flags)."""
    key = (stride, flags)
    if key not in _REF:
        t0 = time.time()
        _REF[key] = A.align(rows, verts, 32, tris, ALIGN_START, BBOX, stride=stride, flags=flags, **ALIGN_KW)
        r = _REF[key]
        print("reference, stride %d, flags %d: %.2f s, %d iterations, flags %d, %d of %d inliers, rms %.3e -> %.3e, corners %.6f -> %.6f m" % (
            stride, flags, time.time() - t0, r["iterations"], r["flags"], r["inliers"], r["rows_sampled"], r["history"][0], r["rms"],
            A.corner_displacement(ALIGN_START, IDENT, BBOX), A.corner_displacement(r["pose"], IDENT, BBOX)))
    return _REF[key]


# ---- 1. the model's own mesh from a perturbed pose -----------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [1, 3])
def test_own_mesh_device_and_host_forms(hfpf_mod, session, stride):
    sc, g, rows, verts, tris = session
    ref = _ref(rows, verts, tris, stride)
    # a test of equality alone would pass on two failed fits: the reference must have fitted
    assert fitted(ref) and ref["rms"] < ref["history"][0], ref
    assert ref["rows_sampled"] == (len(rows) + stride - 1) // stride
    dev = align_device(g, verts, tris, ALIGN_START, stride=stride, **ALIGN_KW)
    print("device form, stride %d: %d iterations, flags %d, %d of %d inliers, rms %.3e" % (stride, dev["iterations"], dev["flags"], dev["inliers"],
                                                                                          dev["rows_sampled"], dev["rms"]))
    same_align(dev, ref, "device form, stride %d" % stride)
    host = g.align_mesh(verts, tris, ALIGN_START, stride=stride, **ALIGN_KW)
    same_align(host, ref, "host form, stride %d" % stride)
    assert fitted(host) and host["rms"] < ref["history"][0]
    assert A.corner_displacement(host["pose"], IDENT, BBOX) < A.corner_displacement(ALIGN_START, IDENT, BBOX)


def test_skip_boundary(hfpf_mod, session):
    sc, g, rows, verts, tris = session
    ref = _ref(rows, verts, tris, 3, A.SKIP_BOUNDARY)  # every third row: a third of the reference's time, the same paths
    assert 0 < ref["inliers"] < _ref(rows, verts, tris, 3)["inliers"]
    same_align(g.align_mesh(verts, tris, ALIGN_START, stride=3, skip_boundary=True, **ALIGN_KW), ref, "SKIP_BOUNDARY")


# ---- 2. many LDS tiles per brick, and a snapshot restored into a second handle -------------------------------------------------

def test_small_tiles_in_a_restored_handle(hfpf_mod, session):
    sc, g, rows, verts, tris = session
    ref = _ref(rows, verts, tris)
    blob = g.snapshot()
    os.environ["HFPF_TEST_DEV_TILE"] = "8"
    try:
        g2 = grid(hfpf_mod)
    finally:
        del os.environ["HFPF_TEST_DEV_TILE"]
    try:
        g2.restore(blob)
        same_align(g2.align_mesh(verts, tris, ALIGN_START, **ALIGN_KW), ref, "tile 8, restored handle")
    finally:
        g2.close()
    with grid(hfpf_mod) as g3:
        g3.restore(blob)
        same_align(g3.align_mesh(verts, tris, ALIGN_START, **ALIGN_KW), ref, "restored handle")


# ---- 3. nothing to fit -----------------------------------------------------------------------------------------------------------

def _too_few(r, pose, rows_sampled):
    assert r["flags"] == A.TOO_FEW and r["iterations"] == 1 and r["inliers"] == 0 and r["rms"] == 0.0 and r["rows_sampled"] == rows_sampled
    assert r["pose"].tobytes() == np.ascontiguousarray(pose, np.float64).tobytes()
    assert not r["information"].any()


def test_too_few_empty_mesh_and_empty_handle(hfpf_mod, session):
    sc, g, rows, verts, tris = session
    # 40 voxels along the rows' mean normal: off the surface, not along it
    nbar = np.array([rows[k].astype(np.float64).mean() for k in ("nx", "ny", "nz")])
    away = ALIGN_START.copy()
    away[:, 3] += 40 * RES * nbar / np.linalg.norm(nbar)
    assert A.align(rows, verts, 32, tris, away, BBOX, max_iterations=1, max_distance=ALIGN_MD)["flags"] == A.TOO_FEW
    _too_few(g.align_mesh(verts, tris, away, **ALIGN_KW), away, len(rows))
    _too_few(align_device(g, verts, tris, away, **ALIGN_KW), away, len(rows))
    none_v, none_t = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32)
    _too_few(g.align_mesh(none_v, none_t, ALIGN_START, **ALIGN_KW), ALIGN_START, len(rows))
    _too_few(g.align_mesh(0, 0, ALIGN_START, device=True, n_verts=0, vertex_stride=12, n_tris=0, **ALIGN_KW), ALIGN_START, len(rows))
    with grid(hfpf_mod) as fresh:
        _too_few(fresh.align_mesh(verts, tris, ALIGN_START, **ALIGN_KW), ALIGN_START, 0)
        sc.integrate(fresh, 0)  # points, but no clean pass yet
        _too_few(fresh.align_mesh(verts, tris, ALIGN_START, **ALIGN_KW), ALIGN_START, 0)


def test_bad_arguments_leave_the_handle_usable(hfpf_mod, session):
    H = hfpf_mod
    sc, g, rows, verts, tris = session
    L, h = H.lib(), g._h
    v, t = np.ascontiguousarray(verts), np.ascontiguousarray(tris)
    pose = np.ascontiguousarray(ALIGN_START, np.float64).reshape(12)
    bad_pose = pose.copy()
    bad_pose[5] = np.nan
    res = H.align_result()
    marker = bytes(res)

    def call(o=None, pose=pose.ctypes.data, stride=32, result=True, n_tris=len(t)):
        o = o if o is not None else H.align_opts(**ALIGN_KW)
        return L.hfpf_align_mesh(h, C.byref(o), v.ctypes.data, len(v), stride, t.ctypes.data, n_tris, pose, C.byref(res) if result else None)

    def opts(compare=None, **kw):
        o = H.align_opts(**ALIGN_KW)
        for k, val in kw.items():
            setattr(o, k, val)
        for k, val in (compare or {}).items():
            setattr(o.compare, k, val)
        return o

    wrong = H.align_result()
    wrong.struct_size = 400
    faults = [dict(pose=bad_pose.ctypes.data), dict(pose=None), dict(o=opts(stride=0)), dict(o=opts(max_iterations=65)),
              dict(o=opts(compare=dict(max_distance=33 * RES))), dict(result=False), dict(o=opts(min_inliers=5)), dict(o=opts(flags=2)),
              dict(o=opts(reserved=1)), dict(o=opts(compare=dict(struct_size=24))), dict(stride=8)]
    for kw in faults:
        assert call(**kw) == -2, kw
        assert bytes(res) == marker, "a rejected call writes nothing"
        assert g.extract().tobytes() == rows.tobytes(), kw
    assert L.hfpf_align_mesh(h, C.byref(H.align_opts(**ALIGN_KW)), v.ctypes.data, len(v), 32, t.ctypes.data, len(t), pose.ctypes.data, C.byref(wrong)) == -2
    assert call(o=opts(compare=dict(max_distance=32 * RES), max_iterations=1), n_tris=64) == 0  # the bound itself is legal
    assert res.iterations == 1 and res.rows_sampled == len(rows)
    assert g.extract().tobytes() == rows.tobytes()


def test_both_forms_on_an_empty_handle_and_the_rejections_of_the_device_form(hfpf_mod, session):
    """What test_too_few_empty_mesh_and_empty_handle and test_bad_arguments_leave_the_handle_usable ask of the host form, through
    hfpf_align_mesh_device: TOO_FEW at the start pose on a handle without rows, and a rejected call leaves the result as it was."""
    H = hfpf_mod
    sc, g, rows, verts, tris = session
    v, t = np.ascontiguousarray(verts[:64]), np.array([[0, 1, 2], [3, 4, 5], [6, 6, 7]], np.uint32)
    with grid(hfpf_mod) as fresh:
        host, dev = fresh.align_mesh(v, t, ALIGN_START, **ALIGN_KW), align_device(fresh, v, t, ALIGN_START, **ALIGN_KW)
        _too_few(host, ALIGN_START, 0)
        same_align(dev, host, "an empty handle, device form")
        assert dev["rows_sampled"] == 0
    L = H.lib()
    pose = np.ascontiguousarray(ALIGN_START, np.float64).reshape(12)
    bad_pose = pose.copy()
    bad_pose[5] = np.nan
    res = H.align_result()
    res.iterations, res.rows_sampled, res.rms = 0x5A5A, 0x5A5A5A5A, 90.0
    marker = bytes(res)

    def opts(compare=None, **kw):
        o = H.align_opts(**ALIGN_KW)
        for k, val in kw.items():
            setattr(o, k, val)
        for k, val in (compare or {}).items():
            setattr(o.compare, k, val)
        return o

    wrong = H.align_result()
    wrong.struct_size = 400
    with uploaded(g, v, t) as (dv, dt):
        def call(o=None, verts=dv, n_verts=len(v), stride=32, tris=dt, n_tris=len(t), pose=pose.ctypes.data, result=res):
            o = o if o is not None else H.align_opts(**ALIGN_KW)
            return L.hfpf_align_mesh_device(g._h, C.byref(o), verts, n_verts, stride, tris, n_tris, pose, C.byref(result) if result is not None else None)

        faults = [dict(pose=bad_pose.ctypes.data), dict(pose=None), dict(o=opts(stride=0)), dict(o=opts(max_iterations=65)),
                  dict(o=opts(compare=dict(max_distance=33 * RES))), dict(result=None), dict(result=wrong), dict(o=opts(min_inliers=5)), dict(o=opts(flags=2)),
                  dict(o=opts(reserved=1)), dict(o=opts(compare=dict(struct_size=24))), dict(stride=8), dict(stride=14), dict(verts=None), dict(tris=None),
                  dict(n_verts=2 ** 32 - 1), dict(n_tris=2 ** 32 - 1), dict(verts=dv + 2), dict(tris=dt + 1)]
        for kw in faults:
            assert call(**kw) == -2, kw
            assert bytes(res) == marker, "a rejected call writes nothing: %r" % (kw,)
        assert call(o=opts(max_iterations=1)) == 0 and res.iterations == 1 and res.rows_sampled == len(rows)  # the handle is still usable
    assert g.extract().tobytes() == rows.tobytes()


# ---- 4. an align is read-only and leaves compare as it was ------------------------------------------------------------------------

def test_align_is_read_only_and_leaves_compare_untouched(hfpf_mod, session):
    sc, g, rows, verts, tris = session
    before = (counters(g), g.extract().tobytes(), g.occupied().tobytes())
    cmp_before = g.compare_mesh(verts, tris, IDENT, max_distance=3 * RES)
    g.kernel_timing(True)
    try:
        got = g.align_mesh(verts, tris, ALIGN_START, **ALIGN_KW)
        assert g.kernel_time(7) == (0.0, 0), "an align is not filed as a compare"
    finally:
        g.kernel_timing(False)
    same_align(got, _ref(rows, verts, tris), "with timing on")
    same_deviation(g.compare_mesh(verts, tris, IDENT, max_distance=3 * RES), cmp_before, "compare after an align")
    assert (counters(g), g.extract().tobytes(), g.occupied().tobytes()) == before
    # what the aligned pose is for: the compare at it finds more rows closer than the compare at the start pose
    at_start, at_fit = g.compare_mesh(verts, tris, ALIGN_START, max_distance=ALIGN_MD)[1], g.compare_mesh(verts, tris, got["pose"], max_distance=ALIGN_MD)[1]
    print("compare at the start pose: found %d, sum_sq %d; at the fitted pose: found %d, sum_sq %d" % (
        at_start["n_found"], at_start["sum_sq_q30"], at_fit["n_found"], at_fit["sum_sq_q30"]))
    assert at_fit["n_found"] >= at_start["n_found"] and at_fit["sum_sq_q30"] < at_start["sum_sq_q30"]


# ---- 5. the node shell: best-fit, then compare -----------------------------------------------------------------------------------

def test_node_aligns_before_it_compares(hfpf_mod, synth_mod, tmp_path):
    import hfpf_node
    sc = DepthScene(3, 160, 120, clean_every=0)
    out = {}
    for mode in ("off", "on"):
        d = tmp_path / mode
        d.mkdir()
        with hfpf_node.FusionNode(BBOX, directory_name=str(d), resolution=RES, final_clean_on_process=True, **DEPTH_CAPS) as n:
            with pytest.raises(hfpf_mod.HfpfError) as e:
                n.set_reference_alignment(stride=0)
            assert e.value.code == -2
            node_feed(n, sc)
            g = node_grid(hfpf_mod, hfpf_node, n)
            try:
                g.clean()
                verts, tris = g.extract_mesh()
                fit = g.align_mesh(verts, tris, ALIGN_START, **ALIGN_KW)
                pose = fit["pose"] if mode == "on" else ALIGN_START
                rows, dev, summary = g.compare_mesh(verts, tris, pose, rows=True, max_distance=ALIGN_MD)
            finally:
                g._h = None
            assert len(rows) > 1000 and summary["n_found"] > 0 and 2 * fit["inliers"] > fit["rows_sampled"]
            n.set_reference_mesh(verts, tris, ALIGN_START, max_distance=ALIGN_MD)
            if mode == "on":
                n.set_reference_alignment(**ALIGN_KW)
            else:
                n.set_reference_alignment(**ALIGN_KW)
                n.set_reference_alignment(None)  # off again: as a node that never called it
            rc, ok, msg = n.process()
            assert rc == 0 and ok, msg
        assert open(os.path.join(str(d), "deviation.csv")).read() == deviation_csv(rows, dev), mode
        assert open(os.path.join(str(d), "deviation_summary.csv")).read() == deviation_summary_csv(summary), mode
        out[mode] = fit
    assert not os.path.exists(os.path.join(str(tmp_path / "off"), "alignment.csv"))
    head, line = open(os.path.join(str(tmp_path / "on"), "alignment.csv")).read().splitlines()
    assert head == "iterations,flags,rows_sampled,inliers,rms," + ",".join("p%d" % i for i in range(12))
    f, vals = out["on"], line.split(",")
    assert [int(x) for x in vals[:4]] == [f["iterations"], f["flags"], f["rows_sampled"], f["inliers"]]
    assert float(vals[4]) == f["rms"]
    assert np.array([float(x) for x in vals[5:]], np.float64).tobytes() == f["pose"].tobytes()
