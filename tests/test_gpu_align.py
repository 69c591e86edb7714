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
from test_align_ref import corner_displacement, rigid
from test_gpu_deviation import IDENT, _same, session  # noqa: F401 (session is the module fixture of that file)
from test_gpu_render import BBOX, CAPS, RES, DepthScene, _counters, _grid

pytestmark = pytest.mark.gpu
MD = 6 * RES
KW = dict(max_iterations=8, max_distance=MD, eps_rotation=1e-5, eps_translation=1e-5)
# the start pose: 0.3 degrees about the bounding box's centre and 1.5 voxels of translation away from the true pose (the identity)
START = rigid(0.3, (0.5, 1.0, -0.4), (0.6 * 1.5 * RES, -0.64 * 1.5 * RES, 0.48 * 1.5 * RES), A.centre(BBOX))
FIELDS = ("iterations", "flags", "rows_sampled", "inliers", "rms")
_REF = {}


def _ref(rows, verts, tris, stride=1, flags=0):
    """align_ref on the session's own mesh from START, computed once per (stride, flags)."""
    key = (stride, flags)
    if key not in _REF:
        t0 = time.time()
        _REF[key] = A.align(rows, verts, 32, tris, START, BBOX, stride=stride, flags=flags, **KW)
        r = _REF[key]
        print("reference, stride %d, flags %d: %.2f s, %d iterations, flags %d, %d of %d inliers, rms %.3e -> %.3e, corners %.6f -> %.6f m" % (
            stride, flags, time.time() - t0, r["iterations"], r["flags"], r["inliers"], r["rows_sampled"], r["history"][0], r["rms"],
            corner_displacement(START, IDENT, BBOX), corner_displacement(r["pose"], IDENT, BBOX)))
    return _REF[key]


def _fitted(r):
    """A result that is a fit and not a failed one: most sampled rows are inliers and the residual went down."""
    return 2 * r["inliers"] > r["rows_sampled"] and r["flags"] in (0, A.CONVERGED) and r["iterations"] > 1


def _equal(got, ref, what):
    for k in FIELDS:
        assert got[k] == ref[k], "%s: %s: %r vs %r" % (what, k, got[k], ref[k])
    assert got["pose"].tobytes() == ref["pose"].tobytes(), "%s: pose\n%r\nvs\n%r" % (what, got["pose"], ref["pose"])
    assert got["information"].tobytes() == ref["information"].tobytes(), "%s: information" % what


def _device_align(g, verts, tris, pose, **kw):
    dv, dt = g.device_alloc(max(verts.nbytes, 16)), g.device_alloc(max(tris.nbytes, 16))
    try:
        g.device_upload(dv, verts), g.device_upload(dt, tris)
        return g.align_mesh(dv, dt, pose, device=True, n_verts=len(verts), vertex_stride=verts.dtype.itemsize, n_tris=len(tris), **kw)
    finally:
        g.device_free(dv), g.device_free(dt)


# ---- 1. the model's own mesh from a perturbed pose -----------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [1, 3])
def test_own_mesh_device_and_host_forms(hfpf_mod, session, stride):
    sc, g, rows, verts, tris = session
    ref = _ref(rows, verts, tris, stride)
    # a test of equality alone would pass on two failed fits: the reference must have fitted
    assert _fitted(ref) and ref["rms"] < ref["history"][0], ref
    assert ref["rows_sampled"] == (len(rows) + stride - 1) // stride
    dev = _device_align(g, verts, tris, START, stride=stride, **KW)
    print("device form, stride %d: %d iterations, flags %d, %d of %d inliers, rms %.3e" % (stride, dev["iterations"], dev["flags"], dev["inliers"],
                                                                                          dev["rows_sampled"], dev["rms"]))
    _equal(dev, ref, "device form, stride %d" % stride)
    host = g.align_mesh(verts, tris, START, stride=stride, **KW)
    _equal(host, ref, "host form, stride %d" % stride)
    assert _fitted(host) and host["rms"] < ref["history"][0]
    assert corner_displacement(host["pose"], IDENT, BBOX) < corner_displacement(START, IDENT, BBOX)


def test_skip_boundary(hfpf_mod, session):
    sc, g, rows, verts, tris = session
    ref = _ref(rows, verts, tris, 3, A.SKIP_BOUNDARY)  # every third row: a third of the reference's time, the same paths
    assert 0 < ref["inliers"] < _ref(rows, verts, tris, 3)["inliers"]
    _equal(g.align_mesh(verts, tris, START, stride=3, skip_boundary=True, **KW), ref, "SKIP_BOUNDARY")


# ---- 2. many LDS tiles per brick, and a snapshot restored into a second handle -------------------------------------------------

def test_small_tiles_in_a_restored_handle(hfpf_mod, session):
    sc, g, rows, verts, tris = session
    ref = _ref(rows, verts, tris)
    blob = g.snapshot()
    os.environ["HFPF_TEST_DEV_TILE"] = "8"
    try:
        g2 = _grid(hfpf_mod)
    finally:
        del os.environ["HFPF_TEST_DEV_TILE"]
    try:
        g2.restore(blob)
        _equal(g2.align_mesh(verts, tris, START, **KW), ref, "tile 8, restored handle")
    finally:
        g2.close()
    with _grid(hfpf_mod) as g3:
        g3.restore(blob)
        _equal(g3.align_mesh(verts, tris, START, **KW), ref, "restored handle")


# ---- 3. nothing to fit -----------------------------------------------------------------------------------------------------------

def _too_few(r, pose, rows_sampled):
    assert r["flags"] == A.TOO_FEW and r["iterations"] == 1 and r["inliers"] == 0 and r["rms"] == 0.0 and r["rows_sampled"] == rows_sampled
    assert r["pose"].tobytes() == np.ascontiguousarray(pose, np.float64).tobytes()
    assert not r["information"].any()


def test_too_few_empty_mesh_and_empty_handle(hfpf_mod, session):
    sc, g, rows, verts, tris = session
    # 40 voxels along the rows' mean normal: off the surface, not along it
    nbar = np.array([rows[k].astype(np.float64).mean() for k in ("nx", "ny", "nz")])
    away = START.copy()
    away[:, 3] += 40 * RES * nbar / np.linalg.norm(nbar)
    assert A.align(rows, verts, 32, tris, away, BBOX, max_iterations=1, max_distance=MD)["flags"] == A.TOO_FEW
    _too_few(g.align_mesh(verts, tris, away, **KW), away, len(rows))
    _too_few(_device_align(g, verts, tris, away, **KW), away, len(rows))
    none_v, none_t = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32)
    _too_few(g.align_mesh(none_v, none_t, START, **KW), START, len(rows))
    _too_few(g.align_mesh(0, 0, START, device=True, n_verts=0, vertex_stride=12, n_tris=0, **KW), START, len(rows))
    with _grid(hfpf_mod) as fresh:
        _too_few(fresh.align_mesh(verts, tris, START, **KW), START, 0)
        sc.integrate(fresh, 0)  # points, but no clean pass yet
        _too_few(fresh.align_mesh(verts, tris, START, **KW), START, 0)


def test_bad_arguments_leave_the_handle_usable(hfpf_mod, session):
    H = hfpf_mod
    sc, g, rows, verts, tris = session
    L, h = H.lib(), g._h
    v, t = np.ascontiguousarray(verts), np.ascontiguousarray(tris)
    pose = np.ascontiguousarray(START, np.float64).reshape(12)
    bad_pose = pose.copy()
    bad_pose[5] = np.nan
    res = H.align_result()
    marker = bytes(res)

    def call(o=None, pose=pose.ctypes.data, stride=32, result=True, n_tris=len(t)):
        o = o if o is not None else H.align_opts(**KW)
        return L.hfpf_align_mesh(h, C.byref(o), v.ctypes.data, len(v), stride, t.ctypes.data, n_tris, pose, C.byref(res) if result else None)

    def opts(compare=None, **kw):
        o = H.align_opts(**KW)
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
    assert L.hfpf_align_mesh(h, C.byref(H.align_opts(**KW)), v.ctypes.data, len(v), 32, t.ctypes.data, len(t), pose.ctypes.data, C.byref(wrong)) == -2
    assert call(o=opts(compare=dict(max_distance=32 * RES), max_iterations=1), n_tris=64) == 0  # the bound itself is legal
    assert res.iterations == 1 and res.rows_sampled == len(rows)
    assert g.extract().tobytes() == rows.tobytes()


# ---- 4. an align is read-only and leaves compare as it was ------------------------------------------------------------------------

def test_align_is_read_only_and_leaves_compare_untouched(hfpf_mod, session):
    sc, g, rows, verts, tris = session
    before = (_counters(g), g.extract().tobytes(), g.occupied().tobytes())
    cmp_before = g.compare_mesh(verts, tris, IDENT, max_distance=3 * RES)
    g.kernel_timing(True)
    try:
        got = g.align_mesh(verts, tris, START, **KW)
        assert g.kernel_time(7) == (0.0, 0), "an align is not filed as a compare"
    finally:
        g.kernel_timing(False)
    _equal(got, _ref(rows, verts, tris), "with timing on")
    _same(g.compare_mesh(verts, tris, IDENT, max_distance=3 * RES), cmp_before, "compare after an align")
    assert (_counters(g), g.extract().tobytes(), g.occupied().tobytes()) == before
    # what the aligned pose is for: the compare at it finds more rows closer than the compare at the start pose
    at_start, at_fit = g.compare_mesh(verts, tris, START, max_distance=MD)[1], g.compare_mesh(verts, tris, got["pose"], max_distance=MD)[1]
    print("compare at the start pose: found %d, sum_sq %d; at the fitted pose: found %d, sum_sq %d" % (
        at_start["n_found"], at_start["sum_sq_q30"], at_fit["n_found"], at_fit["sum_sq_q30"]))
    assert at_fit["n_found"] >= at_start["n_found"] and at_fit["sum_sq_q30"] < at_start["sum_sq_q30"]


# ---- 5. the node shell: best-fit, then compare -----------------------------------------------------------------------------------

def test_node_aligns_before_it_compares(hfpf_mod, synth_mod, tmp_path):
    import hfpf_node
    from test_gpu_node_components import _feed, _grid_of
    from test_gpu_node_deviation import _csv, _summary_csv
    sc = DepthScene(3, 160, 120, clean_every=0)
    out = {}
    for mode in ("off", "on"):
        d = tmp_path / mode
        d.mkdir()
        with hfpf_node.FusionNode(BBOX, directory_name=str(d), resolution=RES, final_clean_on_process=True, **CAPS) as n:
            with pytest.raises(hfpf_mod.HfpfError) as e:
                n.set_reference_alignment(stride=0)
            assert e.value.code == -2
            _feed(n, sc)
            g = _grid_of(hfpf_mod, hfpf_node, n)
            try:
                g.clean()
                verts, tris = g.extract_mesh()
                fit = g.align_mesh(verts, tris, START, **KW)
                pose = fit["pose"] if mode == "on" else START
                rows, dev, summary = g.compare_mesh(verts, tris, pose, rows=True, max_distance=MD)
            finally:
                g._h = None
            assert len(rows) > 1000 and summary["n_found"] > 0 and 2 * fit["inliers"] > fit["rows_sampled"]
            n.set_reference_mesh(verts, tris, START, max_distance=MD)
            if mode == "on":
                n.set_reference_alignment(**KW)
            else:
                n.set_reference_alignment(**KW)
                n.set_reference_alignment(None)  # off again: as a node that never called it
            rc, ok, msg = n.process()
            assert rc == 0 and ok, msg
        assert open(os.path.join(str(d), "deviation.csv")).read() == _csv(rows, dev), mode
        assert open(os.path.join(str(d), "deviation_summary.csv")).read() == _summary_csv(summary), mode
        out[mode] = fit
    assert not os.path.exists(os.path.join(str(tmp_path / "off"), "alignment.csv"))
    head, line = open(os.path.join(str(tmp_path / "on"), "alignment.csv")).read().splitlines()
    assert head == "iterations,flags,rows_sampled,inliers,rms," + ",".join("p%d" % i for i in range(12))
    f, vals = out["on"], line.split(",")
    assert [int(x) for x in vals[:4]] == [f["iterations"], f["flags"], f["rows_sampled"], f["inliers"]]
    assert float(vals[4]) == f["rms"]
    assert np.array([float(x) for x in vals[5:]], np.float64).tobytes() == f["pose"].tobytes()
