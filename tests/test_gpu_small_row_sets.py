"""GPU: every read-out that cuts one scratch buffer into several arrays, on row sets of 1, 2, 3 and 5 rows and on the whole model in
between, all on ONE handle: every buffer is first used small, then regrown, then reused small.  These are the smallest shapes at
which an odd element count puts an 8-byte array behind 4-byte ones, and at which a pointer taken before a buffer regrew would be
read.

The model is the scene of __graft_entry__.smoke() (4 frames of 160 x 120 at 1 mm).  Its seven best rows share the count 15 (and the
8-frame scene's third to eighth share 24), so no min_count leaves 3 or 5 rows of it: five rows of the highest counts, 30 voxels
apart, get 10, 8, 6, 4 and 2 more points at their fused positions, after which the counts separate behind the first, second, third
and fifth row.  The thresholds are read from the sorted count column and the sizes they leave are asserted.

Small sets are compared with components_ref, mesh_ref, deviation_ref and align_ref by the comparisons of
tests/gpu_support.py: byte for byte.  The whole model's results are compared with the same references
once, on their first visit, and must come back byte for byte on every later one.  tests/test_small_row_sets_scene.py holds the CPU
check of the statement about the counts."""
import numpy as np
import pytest

import align_ref as A
import components_ref as CR
import cover_ref as V
import deviation_ref as D
import gpu_support as G
import mesh_ref as M
import raycast_ref as RC
import scenes
from gpu_support import IDENT

pytestmark = pytest.mark.gpu
RES = 0.001
MD = 6 * RES  # compare's and align's max_distance
EXTRA = (10, 8, 6, 4, 2)
SIZES = (1, 2, 3, 5)
ORDER = (5, 0, 1, 0, 3, 2)  # 0 = the whole model
ALIGN_KW = dict(max_iterations=8, max_distance=MD, eps_rotation=1e-5, eps_translation=1e-5)
VIEW = (16, 12)


def _separate_the_best_rows(g, rows, sc):
    """EXTRA[j] more points on the j-th of five rows of the highest counts that lie 30 voxels apart (Chebyshev), each at the row's
    fused position, seen from a camera 0.44 m in front of their mean depth; then a clean."""
    order = np.argsort(-rows["count"].astype(np.int64), kind="stable")
    cell = np.stack([rows["ix"], rows["iy"], rows["iz"]], axis=1).astype(np.int64)
    pick = []
    for i in order:
        if all(np.abs(cell[i] - cell[j]).max() >= 30 for j in pick):
            pick.append(i)
        if len(pick) == len(EXTRA):
            break
    P = np.stack([rows[k][pick] for k in ("x", "y", "z")], axis=1).astype(np.float64)
    cam_z = P[:, 2].mean() - 0.44
    rec = np.zeros((sum(EXTRA), 4), np.float32)
    rec[:, :3] = np.repeat(P, EXTRA, axis=0) - np.array([0.0, 0.0, cam_z])
    assert 0.3 < rec[:, 2].min() and rec[:, 2].max() < 0.58, "inside the default z-clip"
    g.integrate(np.ascontiguousarray(rec), np.hstack([np.eye(3), [[0.0], [0.0], [cam_z]]]))
    g.clean()


@pytest.fixture(scope="module")
def session(hfpf_mod, synth_mod):
    sc = scenes.Scene(4, 160, 120, RES, fx=615.0, clean_every=2)
    g = hfpf_mod.OccupancyGrid(resolution=sc.resolution, bbox=sc.bbox, max_bricks=40000, max_log_points=1 << 21, max_normals=1 << 19, max_frames=64)
    _separate_the_best_rows(g, scenes.run(g, sc, "integrate").copy(), sc)
    rows = g.extract().copy()
    occ = g.occupied().copy()
    c = np.sort(rows["count"])[::-1].astype(np.int64)
    print("session: %d rows, %d occupied cells, best counts %s" % (len(rows), len(occ), c[:8]))
    thr = {}
    for k in SIZES:
        assert c[k - 1] > c[k], "no min_count leaves %d rows: counts %s" % (k, c[:8])
        thr[k] = float(c[k - 1])
        assert int(CR.count_gate(rows, thr[k]).sum()) == k
    thr[0] = 0.0
    yield sc, g, rows, occ, thr
    g.close()


def _device_compare(g, H, verts, tris, pose, **kw):
    with G.uploaded(g, verts, tris) as (dv, dt):
        return G.compare_device(g, H, dv, len(verts), verts.dtype.itemsize, dt, len(tris), pose, rows=True, **kw)


def _read_outs(g, H, mc, mesh, start):
    """Every read-out at min_count mc, host and device form: a dict of (host, device) pairs."""
    sv, st = mesh
    ckw = dict(reach=1, min_count=mc)
    mkw = dict(radius=2, min_count=mc)
    return dict(
        filtered=g.extract_filtered(mc).copy(),
        components=(g.extract_components(**ckw), G.components_device(g, H, **ckw)),
        mesh=(g.extract_mesh(**mkw), G.mesh_device(g, **mkw)),
        compare=(g.compare_mesh(sv, st, IDENT, rows=True, min_count=mc, max_distance=MD), _device_compare(g, H, sv, st, IDENT, min_count=mc, max_distance=MD)),
        align=(g.align_mesh(sv, st, start, min_count=mc, **ALIGN_KW), G.align_device(g, sv, st, start, min_count=mc, **ALIGN_KW)))


def test_small_row_sets_between_visits_of_the_whole_model(hfpf_mod, session):
    sc, g, rows, occ, thr = session
    H = hfpf_mod
    bbox = tuple(g.cfg.bbox)
    dims, res = g.dims
    # the mesh every compare and align runs against: the model's own at the gate of the five best rows
    mesh = g.extract_mesh(radius=2, min_count=thr[5])
    sv, st = mesh
    print("own mesh of the five best rows: %d vertices, %d triangles" % (len(sv), len(st)))
    assert len(st) > 0
    start = A.rigid(0.3, (0.5, 1.0, -0.4), (0.6 * 1.5 * RES, -0.64 * 1.5 * RES, 0.48 * 1.5 * RES), A.centre(bbox))
    whole = _read_outs(g, H, 0.0, mesh, start)  # the first growth of every buffer, pinned by the references like the small sets
    assert whole["filtered"].tobytes() == rows.tobytes() and len(whole["mesh"][0][1]) > 1000 and whole["align"][0]["iterations"] >= 1
    ref_whole = dict(components=CR.components(rows, reach=1), mesh=M.mesh(rows, occ, bbox, res, dims, radius=2)[:2],
                     compare=D.compare(rows, sv, 32, st, IDENT, 0.0, MD), align=A.align(rows, sv, 32, st, start, bbox, **ALIGN_KW))
    for form in (0, 1):
        name = "the whole model on the fresh handle, %s form" % ("host", "device")[form]
        G.same_components(whole["components"][form], ref_whole["components"], name)
        G.same_mesh(whole["mesh"][form], ref_whole["mesh"], name)
        G.same_deviation(whole["compare"][form][1:], ref_whole["compare"], name)
        G.same_align(whole["align"][form], ref_whole["align"], name)
    visits = 0
    for k in ORDER:
        mc = thr[k]
        got = _read_outs(g, H, mc, mesh, start)
        what = "%d rows (min_count %g)" % (k, mc) if k else "the whole model, visit %d" % (visits + 1)
        gated = rows[CR.count_gate(rows, mc)]
        assert got["filtered"].tobytes() == gated.tobytes(), what
        for form in (0, 1):
            name = "%s, %s form" % (what, ("host", "device")[form])
            if k == 0:
                G.same_components(got["components"][form], whole["components"][0], name)
                G.same_mesh(got["mesh"][form], whole["mesh"][0], name)
                assert got["compare"][form][0].tobytes() == rows.tobytes(), name
                G.same_deviation(got["compare"][form][1:], whole["compare"][0][1:], name)
                G.same_align(got["align"][form], whole["align"][0], name)
                continue
            assert len(gated) == k
            G.same_components(got["components"][form], CR.components(gated, reach=1), name)
            ref_mesh = M.mesh(rows, occ, bbox, res, dims, radius=2, min_count=mc)[:2]
            G.same_mesh(got["mesh"][form], ref_mesh, name)
            assert got["compare"][form][0].tobytes() == gated.tobytes(), name
            G.same_deviation(got["compare"][form][1:], D.compare(rows, sv, 32, st, IDENT, mc, MD), name)
            G.same_align(got["align"][form], A.align(rows, sv, 32, st, start, bbox, min_count=mc, **ALIGN_KW), name)
        if k == 0:
            visits += 1
        if k == 0 and visits == 2:  # the whole model between 1 row and 3 rows: the two read-outs that take no min_count gate from it
            ckw = dict(radius=2, max_distance=2 * RES, spacing=RES)
            G.same_coverage(g.cover_mesh(sv, st, IDENT, **ckw), V.cover(rows, occ, sv, 32, st, IDENT, bbox, res, **ckw), "cover_mesh")
            K = (sc.fx * VIEW[0] / sc.W, sc.fx * VIEW[0] / sc.W, (VIEW[0] - 1) / 2.0, (VIEW[1] - 1) / 2.0)
            pose = np.asarray(sc.poses[0], np.float64).reshape(3, 4)
            hits = g.raycast_view(pose, K, VIEW[0], VIEW[1], t_range=(0.25, 0.65))
            G.same_rays(hits, RC.raycast_view(rows, occ, pose, K, VIEW[0], VIEW[1], bbox, res, t_range=(0.25, 0.65)), "raycast_view")
            assert (hits["flags"] & RC.HIT != 0).any()
    assert visits == 2
    assert g.extract().tobytes() == rows.tobytes(), "the read-outs changed the model"
