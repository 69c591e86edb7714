"""GPU: the hot path and every read-out at the largest cell and brick indices a handle takes.  The scenes of faces.DEEP keep
CUT_BBOX's max corner and push the min corner away: deepx, deepy and deepz have 2,097,150 cells on one axis (the most hfpf_create
accepts: a 21-bit key field with index == dim = 0x1FFFFE in it, Morton codes of 63 bits, mesh lattice keys of 63 bits), deep3 has
12630^3 cells = 1579^3 = 3.94e9 brick-directory entries, so every row's linear brick index lies above 2^31.  The surface stays
where it is, so the rows sit in the max face layers, occupied cells at index == dim, and every coordinate keeps its f32 precision.
Everything is byte for byte against the oracle, or against the numpy restatement of the read-out run on the session's own extract()
rows and occupied() list, with the option tables of test_gpu_faces.py; the inputs are aimed at Session.model_box, where the model
is (faces.FaceScene).  deep3's tests stand last: its handle holds a 15.8 GB directory, is made when they begin and closed by the
last of them."""
import time

import numpy as np
import pytest

import align_ref as A
import components_ref as CR
import cover_ref as V
import deviation_ref as D
import faces
import gpu_support as G
import mesh_ref as M
import query_ref as Q
import raycast_ref as RC
import render_ref as R
import scenes
import track_ref as TR
from gpu_support import IDENT

pytestmark = pytest.mark.gpu
INF = float("inf")
STEP = 0.5
LONG = ("deepx", "deepy", "deepz")
MESHED = ("deepx", "deepz")   # components and the mesh comparisons, with deep3
# the option tables of test_gpu_faces.py
QUERY_OPTS = [(0, 0.0, INF), (1, 0.0, INF), (2, 0.0, INF), (3, 0.0, INF), (4, 0.0, INF), (2, 3.0, INF), (3, 0.0, 1.5)]
QUERY_IDS = ["r%d_mc%g_md%g" % o for o in QUERY_OPTS]
RAY_OPTS = [(1, False), (2, True), (4, False)]
RAY_IDS = ["r%d_c%d" % o for o in RAY_OPTS]
COMP_OPTS = [(1, -2.0, 0), (2, -2.0, 0), (3, -2.0, 0), (4, -2.0, 0), (2, 0.9, 0), (1, -2.0, 100)]
COMP_IDS = ["reach%d_dot%g_rows%d" % o for o in COMP_OPTS]
ALIGN_KW = dict(max_iterations=5, stride=4, eps_rotation=1e-5, eps_translation=1e-5)


@pytest.fixture(scope="module")
def sessions(hfpf_mod, synth_mod):
    """name -> Session, each built when first asked for and closed at the end of the module (deep3: by its last test)."""
    made = {}

    def get(name):
        if name not in made:
            t0 = time.time()
            made[name] = G.Session(hfpf_mod, name)
            print("%s: session built in %.1f s" % (name, time.time() - t0))
        return made[name]

    yield get
    for s in made.values():
        s.close()


def _deep_axes(name):
    return list(faces.DEEP_AXES[name])


# ---- a. the hot path ------------------------------------------------------------------------------------------------------------

def _oracle(oracle_mod, sc):
    og = oracle_mod.OracleGrid(resolution=sc.resolution, bbox=sc.bbox, fuse_color=True, exact_moments=True, **sc.config)
    scenes.run(og, sc, "capture", color=True)
    out = og.extract_exact(), og.occupied(), og.counters()
    og.close()
    return out


def _hot_path(oracle_mod, name, rows, occ, ctr):
    """Rows (fourteen columns byte for byte, the two distances within their derived bounds), occupied list and counters against the
    oracle, whose canonical mode keys cells with 21 bits an axis whatever the dims."""
    exact, occ_ref, oc = _oracle(oracle_mod, faces.FaceScene(name))
    assert np.array_equal(occ_ref, occ), "occupied lists differ"
    rep = scenes.compare_rows_exact(exact, rows)
    assert rep["exact_bytes_differing"] == 0 and rep["rows"] == faces.ORACLE_TABLE[name][0]
    for a, b in (("presented", "points_presented"), ("zclip_pass", "points_zclip_pass"), ("inserted", "points_in_bbox"),
                 ("buffered", "points_buffered"), ("occupied", "voxels_occupied"), ("normals", "voxels_with_normal")):
        assert oc[a] == ctr[b], "%s: counter %s %d, the oracle's %s %d" % (name, b, ctr[b], a, oc[a])
    assert ctr["voxels_occupied"] == len(occ)


@pytest.mark.parametrize("name", LONG)
def test_hot_path_against_the_oracle(oracle_mod, sessions, name):
    s = sessions(name)
    _hot_path(oracle_mod, name, s.rows, s.occ, s.g.counters())


def test_hot_path_of_the_direct_update_deepx(oracle_mod, hfpf_mod, synth_mod):
    """The update without bins (binned_update=False) takes every point through the directory by its own cell key."""
    s = G.Session(hfpf_mod, "deepx", binned_update=False)
    try:
        _hot_path(oracle_mod, "deepx", s.rows, s.occ, s.g.counters())
    finally:
        s.close()


# ---- b. query -------------------------------------------------------------------------------------------------------------------

def _query(s, opt):
    radius, min_count, md = opt
    kw = dict(radius=radius, min_count=min_count, max_distance=md * s.res)
    pts = faces.query_points(s.rows, s.bbox, s.res, s.dims)
    ref = Q.query(s.rows, s.occ, pts, IDENT, s.bbox, s.res, **kw)
    got = s.g.query(pts, IDENT, **kw)
    G.same_query(got, ref, "%s %r, host form" % (s.name, opt))
    with G.uploaded(s.g, pts) as (d,):
        G.same_query(s.g.query_device(d, len(pts), IDENT, **kw), ref, "%s %r, device form" % (s.name, opt))
    f = got[0]["flags"]
    inb, found = f & Q.IN_BBOX != 0, f & Q.FOUND != 0
    ax = _deep_axes(s.name)
    at_dim = inb & (got[0]["voxel"] == np.asarray(s.dims))[:, ax].any(axis=1)
    row_top = found & (got[0]["row_voxel"] == np.asarray(s.dims) - 1)[:, ax].any(axis=1)
    print("%s %r: %d points, %d in the box, %d in a cell of index dim of a deep axis (%d occupied, %d found), %d found, %d of them a row at dim - 1" % (
        s.name, opt, len(pts), inb.sum(), at_dim.sum(), (f[at_dim] & Q.OCCUPIED != 0).sum(), (found & at_dim).sum(), found.sum(), row_top.sum()))
    assert found.sum() > 1000 and (~inb).any()
    assert at_dim.any() and not (f[at_dim] & Q.HAS_ROW).any() and (f[at_dim] & Q.OCCUPIED).any()
    assert row_top.sum() >= 20
    if radius >= 1:  # (a cell of index dim has no row: radius 0 finds nothing there)
        assert (found & at_dim).any(), "no found point in a cell of index dim of a deep axis"


@pytest.mark.parametrize("opt", QUERY_OPTS, ids=QUERY_IDS)
@pytest.mark.parametrize("name", LONG)
def test_query(sessions, name, opt):
    _query(sessions(name), opt)


# ---- c. mesh --------------------------------------------------------------------------------------------------------------------

def _mesh(s, radius):
    rv, rt, sizes = M.mesh(s.rows, s.occ, s.bbox, s.res, s.dims, radius=radius)
    host = s.g.extract_mesh(radius=radius)
    G.same_mesh(host, (rv, rt), "%s, host form, radius %d" % (s.name, radius))
    G.same_mesh(G.mesh_device(s.g, radius=radius), (rv, rt), "%s, device form, radius %d" % (s.name, radius))
    v, t = host
    assert len(t) > 1000 and t.max() < len(v), "a triangle index out of range"
    lo, hi = faces.lo_hi(s.bbox)
    p = M.positions(v).astype(np.float64)
    assert (p >= lo).all() and (p <= hi).all(), "a vertex outside the closed box"
    near = faces.near_faces(p, s.bbox, s.res)
    print("%s, radius %d: %d vertices, %d triangles, %r; vertices within a voxel of each face %r" % (s.name, radius, len(v), len(t), sizes, near))
    for a in _deep_axes(s.name):
        assert near[2 * a] == 0 and near[2 * a + 1] >= 1, "axis %d: %r" % (a, near)


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("name", LONG)
def test_mesh(sessions, name, radius):
    _mesh(sessions(name), radius)


# ---- d. raycast -----------------------------------------------------------------------------------------------------------------

def _raycast(s, opt, rays):
    kw = dict(radius=opt[0], cull_backfaces=opt[1], step=STEP, t_range=(0.0, faces.ray_t_max(s.model_box, s.res, STEP)))
    ref = RC.raycast(s.rows, s.occ, rays, IDENT, s.bbox, s.res, **kw)
    hit = ref["flags"] & RC.HIT != 0
    top = (ref["row_voxel"][hit] == np.asarray(s.dims) - 1)[:, _deep_axes(s.name)].any(axis=1).sum()
    print("%s %r: %d rays, %d samples a ray, %d hits (%d on a row at dim - 1 of a deep axis), %d near without a hit" % (
        s.name, opt, len(rays), RC.n_samples(0.0, kw["t_range"][1], STEP, s.res), hit.sum(), top, ((ref["flags"] & RC.NEAR != 0) & ~hit).sum()))
    G.same_rays(s.g.raycast(rays, IDENT, **kw), ref, "%s, host form %r" % (s.name, opt))
    G.same_rays(G.rays_device(s.g, rays, IDENT, **kw), ref, "%s, device form %r" % (s.name, opt))
    assert hit.sum() >= 100 and top >= 1


def _raycast_view(s):
    """160 x 120 from 0.08 m outside the z-max face of the model's box, which is a face of the grid, looking along -z; the march
    runs from 0.02 m before that face to 0.05 m (25 voxels) behind it, which bounds the reference's run time and still meets every
    row of the face layer the view sees."""
    pose, K = faces.outside_view(s.model_box, max_face=True)
    kw = dict(radius=2, step=STEP, t_range=(0.06, 0.13))
    ref = RC.raycast_view(s.rows, s.occ, pose, K, 160, 120, s.bbox, s.res, **kw)
    hit = ref["flags"] & RC.HIT != 0
    top = (ref["row_voxel"][hit] == np.asarray(s.dims) - 1).any(axis=1).sum()
    print("%s: view of 160 x 120 from outside the z-max face: %d hits, %d on a row at dim - 1" % (s.name, hit.sum(), top))
    G.same_rays(s.g.raycast_view(pose, K, 160, 120, **kw), ref, "%s, view" % s.name)
    assert hit.sum() >= 100 and top >= 1


@pytest.mark.parametrize("opt", RAY_OPTS, ids=RAY_IDS)
@pytest.mark.parametrize("name", LONG)
def test_raycast(sessions, name, opt):
    """Every third ray of the sets of test_gpu_faces.test_raycast, aimed at the model's box: about 1000."""
    s = sessions(name)
    _raycast(s, opt, np.ascontiguousarray(faces.rays(s.model_box, s.res)[::3]))


@pytest.mark.parametrize("name", LONG)
def test_raycast_view_through_the_max_face(sessions, name):
    _raycast_view(sessions(name))


# ---- e. components --------------------------------------------------------------------------------------------------------------

def _components(s, opt):
    kw = dict(reach=opt[0], min_normal_dot=opt[1], min_rows=opt[2])
    ref = CR.components(s.rows, **kw)
    got = s.g.extract_components(**kw)
    print("%s %r: %d of %d rows kept in %d components, largest %d" % (s.name, opt, len(got[0]), len(s.rows), len(got[2]),
                                                                      got[2]["n_rows"].max() if len(got[2]) else 0))
    G.same_components(got, ref, "%s %r" % (s.name, opt))
    G.same_components(G.components_device(s.g, s.H, **kw), ref, "%s, device form %r" % (s.name, opt))
    assert len(got[2]) >= 1 and (got[2]["hi"] < np.asarray(s.dims)).all() and (got[2]["lo"] >= 0).all(), "a component reaches index dim"
    assert (got[2]["hi"].max(axis=0) == np.asarray(s.dims) - 1)[_deep_axes(s.name)].all(), "no component reaches dim - 1 of a deep axis"
    if opt[2]:
        assert 0 < len(got[0]) < len(s.rows), "min_rows should drop something and keep something"
    else:
        assert got[0].tobytes() == s.rows.tobytes()


@pytest.mark.parametrize("opt", COMP_OPTS, ids=COMP_IDS)
@pytest.mark.parametrize("name", MESHED)
def test_components(sessions, name, opt):
    _components(sessions(name), opt)


# ---- f. deviation, cover and align --------------------------------------------------------------------------------------------------

def _cover_kw(s):
    return dict(radius=2, max_distance=2 * s.res, spacing=s.res)


def _own_mesh(s):
    """compare and cover against the session's own mesh: the host forms on every fourth triangle, to bound the references' run time
    (it grows with the pairs of rows and nearby triangles), compare's device form on the device copy of all of them."""
    v, t, dv, dt = s.own_mesh()
    t4 = np.ascontiguousarray(t[::4])
    got = s.g.compare_mesh(v, t4, IDENT, max_distance=20 * s.res)
    print("%s, own mesh, 20 voxels: found %d of %d, max %.6f" % (s.name, got[1]["n_found"], got[1]["n_rows"], got[1]["max_abs"]))
    G.same_deviation(got, D.compare(s.rows, v, 32, t4, IDENT, 0.0, 20 * s.res), "%s, own mesh, 20 voxels" % s.name)
    assert got[1]["n_found"] > 0.5 * len(s.rows)
    got = G.compare_device(s.g, s.H, dv, len(v), 32, dt, len(t), IDENT, max_distance=3 * s.res)
    G.same_deviation(got, D.compare(s.rows, v, 32, t, IDENT, 0.0, 3 * s.res), "%s, own mesh, 3 voxels, device form" % s.name)
    assert got[1]["n_found"] > 0.9 * (s.rows["count"] > 0).sum(), "nearly every live row lies within 3 voxels of the mesh made of them"
    got = s.g.cover_mesh(v, t4, IDENT, **_cover_kw(s))
    print("%s, own mesh: %d samples, %d in the box, %d covered" % (s.name, got[1]["n_samples"], got[1]["n_in_bbox"], got[1]["n_covered"]))
    G.same_coverage(got, V.cover(s.rows, s.occ, v, 32, t4, IDENT, s.bbox, s.res, **_cover_kw(s)), "%s, own mesh" % s.name)
    G.coverage_sums(*got)
    assert got[1]["n_covered"] > 0.5 * got[1]["n_samples"]


def _displaced_mesh(s):
    """The own mesh (every fourth triangle) moved by (3, -2, 4) voxels: rows compare with triangles that lie partly outside the box,
    and cover samples fall beyond the max faces and must not count as in the box."""
    v, t, dv, dt = s.own_mesh()
    t4 = np.ascontiguousarray(t[::4])
    pose = faces.shift_pose((3, -2, 4), s.res)
    got = s.g.compare_mesh(v, t4, pose, max_distance=3 * s.res)
    G.same_deviation(got, D.compare(s.rows, v, 32, t4, pose, 0.0, 3 * s.res), "%s, displaced mesh" % s.name)
    assert 0 < got[1]["n_found"] < len(s.rows)
    got = s.g.cover_mesh(v, t4, pose, **_cover_kw(s))
    print("%s, displaced: %d samples, %d in the box, %d covered" % (s.name, got[1]["n_samples"], got[1]["n_in_bbox"], got[1]["n_covered"]))
    G.same_coverage(got, V.cover(s.rows, s.occ, v, 32, t4, pose, s.bbox, s.res, **_cover_kw(s)), "%s, displaced mesh" % s.name)
    G.coverage_sums(*got)
    assert 0 < got[1]["n_in_bbox"] < got[1]["n_samples"], "the displaced mesh leaves the box through the max faces"


def _align(s):
    """Every 16th row against every fourth triangle of the own mesh, from 0.3 degrees about the model's centre and 2 voxels away.
    The twist is taken about the centre of the handle's box, and a row whose lever from there has a component of 32 m or more is no
    inlier (include/hfpf.h): in deep3 the centre is 12.6 m from the model and the fit goes through; in the scenes with a 4.2 km axis
    it is 2.1 km away, and HFPF_ALIGN_TOO_FEW with the start pose is the documented answer."""
    v, t, dv, dt = s.own_mesh()
    t4 = np.ascontiguousarray(t[::4])
    start = A.rigid(0.3, (0.5, 1.0, -0.4), tuple(np.array([0.6, -0.64, 0.48]) * 2 * s.res), A.centre(s.model_box))
    kw = dict(ALIGN_KW, stride=16, max_distance=8 * s.res)
    ref = A.align(s.rows, v, 32, t4, start, s.bbox, **kw)
    print("%s: %d iterations, flags %d, %d of %d inliers, rms %r" % (s.name, ref["iterations"], ref["flags"], ref["inliers"], ref["rows_sampled"], ref["history"]))
    lever = np.abs(np.asarray(A.centre(s.bbox)) - np.asarray(A.centre(s.model_box))).max()
    if s.name == "deep3":
        assert lever < 16 and G.fitted(ref) and ref["rms"] < ref["history"][0], "the reference must have fitted: equality of two failed fits shows nothing"
    else:
        assert lever > 2000 and ref["flags"] == A.TOO_FEW and ref["inliers"] == 0 and ref["iterations"] == 1 and ref["pose"].tobytes() == start.tobytes()
    G.same_align(G.align_device(s.g, v, t4, start, **kw), ref, "%s, device form" % s.name)
    G.same_align(s.g.align_mesh(v, t4, start, **kw), ref, "%s, host form" % s.name)


def _huge_quad(s):
    """Two triangles 1.25 m across through the model: their boxes span every brick that holds a row, so the row side's sort runs over
    all bits of the linear brick key (32 on deep3, 25 to 26 on the others)."""
    quad, t2, pose = faces.huge_quad(s.model_box)
    bits = (faces.prod_bdims(s.dims) - 1).bit_length()
    assert bits == (32 if s.name == "deep3" else 25 if s.name == "deepx" else 26), "%s: %d bits of brick key" % (s.name, bits)
    for voxels in (4, 32):
        got = s.g.compare_mesh(quad, t2, pose, max_distance=voxels * s.res)
        G.same_deviation(got, D.compare(s.rows, quad, 12, t2, pose, 0.0, voxels * s.res), "%s, quad, %d voxels" % (s.name, voxels))
        print("%s, quad, %d voxels: found %d of %d, negative %d" % (s.name, voxels, got[1]["n_found"], len(s.rows), got[1]["n_negative"]))
        assert 0 < got[1]["n_found"] and 0 < got[1]["n_negative"] < got[1]["n_found"], "a non-empty pair list, rows on both sides"
    got = s.g.cover_mesh(quad, t2, pose, **_cover_kw(s))
    G.same_coverage(got, V.cover(s.rows, s.occ, quad, 12, t2, pose, s.bbox, s.res, **_cover_kw(s)), "%s, quad" % s.name)
    G.coverage_sums(*got)
    print("%s, quad: %d samples, %d in the box, %d covered" % (s.name, got[1]["n_samples"], got[1]["n_in_bbox"], got[1]["n_covered"]))
    assert (got[0]["flags"] & V.VALID != 0).all() and 0 < got[1]["n_in_bbox"] < got[1]["n_samples"]


@pytest.mark.parametrize("name", MESHED)
def test_compare_and_cover_own_mesh(sessions, name):
    _own_mesh(sessions(name))


@pytest.mark.parametrize("name", MESHED)
def test_compare_and_cover_a_displaced_mesh(sessions, name):
    _displaced_mesh(sessions(name))


@pytest.mark.parametrize("name", MESHED)
def test_align_own_mesh(sessions, name):
    _align(sessions(name))


@pytest.mark.parametrize("name", MESHED)
def test_two_huge_triangles_through_the_model(sessions, name):
    _huge_quad(sessions(name))


# ---- g. render and track ----------------------------------------------------------------------------------------------------------

def test_render_every_plane_deepx(sessions):
    s = sessions("deepx")
    K, W, H, z_range = (300.0, 300.0, 159.5, 119.5), 320, 240, (0.05, 3.0)
    for pose in (s.sc.poses[0], s.sc.poses[5]):
        got = s.g.render(pose, K, W, H, z_range=z_range, min_count=1, splat_radius=2, max_splat_radius=4, cull_backfaces=True, world_normals=True)
        assert sorted(got) == ["count", "depth", "normal", "rgb", "voxel"]
        G.same_planes(got, R.render(s.rows, pose, K, W, H, s.res, z_range, 1, 2, 4, R.CULL_BACKFACES | R.WORLD_NORMALS), s.name)
        seen = ~np.isnan(got["depth"])
        assert seen.sum() > 1000 and (got["voxel"][seen][:, 0] == s.dims[0] - 1).any(), "no pixel shows a row at ix = dim - 1"


def test_track_depth_deepx(synth_mod, sessions):
    """hfpf_track_depth of a held-out frame of the same stream at a perturbed pose, byte for byte against track_ref."""
    s = sessions("deepx")
    assert s.sc.resolution == G.RES
    W, H, f = 320, 240, s.sc.n_frames + 1
    true = synth_mod.pose(s.sc.pose_seed, f)
    depth, _, K = synth_mod.depth_frame(s.sc.seed, f, W, H, true)
    guess = G.perturb(true, 2.0, (0.006, -0.005, 0.006))
    got = s.g.track_depth(depth, guess, K, stride=1, **G.TRACK_OPTS)
    ref = G.track_reference(s.rows, TR.depth_points(depth, K, 1), guess, K, W, H)
    print("deepx: %d iterations, flags %d, %d of %d used points inliers, rms %.2e, error %s -> %s" % (
        got[1]["iterations"], got[1]["flags"], got[1]["inliers"], got[1]["points_used"], got[1]["rms"], G.pose_errors(guess, true),
        G.pose_errors(got[0], true)))
    G.same_track(got, ref, "deepx")
    assert ref["iterations"] > 1 and ref["inliers"] > 1000


# ---- h1. snapshot and restore -------------------------------------------------------------------------------------------------------

def _restored_handle_gives_the_same_bytes(hfpf_mod, s):
    pts = np.ascontiguousarray(faces.query_points(s.rows, s.bbox, s.res, s.dims)[::4])
    kw = dict(radius=2, min_count=3.0)
    first = s.g.query(pts, IDENT, **kw)
    blob = s.g.snapshot()
    info = hfpf_mod.snapshot_info(blob)
    print("%s: snapshot of %d bytes" % (s.name, info["total_bytes"]))
    assert info["total_bytes"] == len(np.frombuffer(blob, np.uint8)) < 64 << 20, "the directory is not in the blob"
    larger = dict(G.SMALL_CAPS, max_bricks=100000, max_normals=2 << 20, max_frames=8192)  # (max_log_points must be the snapshot's)
    with hfpf_mod.OccupancyGrid(resolution=s.sc.resolution, bbox=s.bbox, fuse_color=True, **s.sc.config, **larger) as g2:
        g2.restore(blob)
        assert g2.extract().tobytes() == s.rows.tobytes() and g2.occupied().tobytes() == s.occ.tobytes()
        second = g2.query(pts, IDENT, **kw)
        assert G.contract_counters(g2) == G.contract_counters(s.g)
    G.same_query(second, first, "%s, restored handle" % s.name)
    assert (first[0]["flags"] & Q.FOUND != 0).sum() > 1000


def test_a_restored_deepy_handle_gives_the_same_bytes(hfpf_mod, sessions):
    _restored_handle_gives_the_same_bytes(hfpf_mod, sessions("deepy"))


# ---- i. the limits of create --------------------------------------------------------------------------------------------------------

def test_the_limits_of_create(hfpf_mod):
    """2,097,150 cells an axis are taken and one more is HFPF_ERR_BAD_CONFIG, on each axis; a box of 1588^3 bricks (4.005e9 directory
    entries) is HFPF_ERR_BAD_CONFIG before anything is allocated."""
    H = hfpf_mod
    tiny = G.SMALL_CAPS
    r = float(np.float32(0.002))
    for a in range(3):
        cells = [0, 0, 0]
        cells[a] = faces.DEEP_CELLS
        with H.OccupancyGrid(resolution=0.002, bbox=faces.deep_bbox(cells), **tiny) as g:
            assert g.dims[0][a] == faces.DEEP_CELLS == 2097150
        box = list(faces.CUT_BBOX)
        box[2 * a] = box[2 * a + 1] - (faces.DEEP_CELLS + 1.25) * r
        with pytest.raises(H.HfpfError) as e:
            H.OccupancyGrid(resolution=0.002, bbox=box, **tiny)
        assert e.value.code == -1 and "2^21" in str(e.value), str(e.value)
    with H.OccupancyGrid(resolution=0.002, bbox=faces.CUT_BBOX, **tiny) as g:
        before = g.counters()["device_bytes"]
    n = 1588 * 8 - 2   # dim + 8 >> 3 = 1588 bricks an axis
    assert faces.prod_bdims((n,) * 3) == 1588 ** 3 > 4.0e9 and faces.prod_bdims((faces.DEEP3_CELLS,) * 3) <= 4.0e9
    with pytest.raises(H.HfpfError) as e:
        H.OccupancyGrid(resolution=0.002, bbox=faces.deep_bbox((n,) * 3), **tiny)
    assert e.value.code == -1 and "directory" in str(e.value), str(e.value)
    with H.OccupancyGrid(resolution=0.002, bbox=faces.CUT_BBOX, **tiny) as g:
        assert g.counters()["device_bytes"] == before, "a refused create left something allocated"


# ---- j. nothing changes -------------------------------------------------------------------------------------------------------------

def _the_read_outs_changed_nothing(s):
    """After every read-out above (and, for a run of this test alone, after one of each here) the session's rows, occupied list and
    counters are what they were when it was built."""
    pts = np.ascontiguousarray(faces.query_points(s.rows, s.bbox, s.res, s.dims)[::16])
    s.g.query(pts, IDENT, radius=2, min_count=3.0)
    v, t = s.g.extract_mesh(radius=2)
    t = np.ascontiguousarray(t[::16])
    s.g.raycast(np.ascontiguousarray(faces.rays(s.model_box, s.res)[::16]), IDENT, radius=2, cull_backfaces=True, step=STEP,
                t_range=(0.0, faces.ray_t_max(s.model_box, s.res, STEP)))
    s.g.raycast_view(*faces.outside_view(s.model_box, max_face=True), 160, 120, radius=1, step=STEP, t_range=(0.06, 0.2))
    s.g.extract_components(reach=2, min_normal_dot=0.9)
    pose = faces.shift_pose((3, -2, 4), s.res)
    s.g.compare_mesh(v, t, pose, max_distance=20 * s.res)
    s.g.cover_mesh(v, t, pose, **_cover_kw(s))
    s.g.align_mesh(v, t, A.rigid(0.3, (0.5, 1.0, -0.4), (0.002, -0.002, 0.002), A.centre(s.model_box)), max_distance=8 * s.res, **ALIGN_KW)
    assert s.g.extract().tobytes() == s.rows.tobytes()
    assert s.g.occupied().tobytes() == s.occ.tobytes()
    assert G.counters(s.g) == s.counters


@pytest.mark.parametrize("name", LONG)
def test_the_read_outs_changed_nothing(sessions, name):
    _the_read_outs_changed_nothing(sessions(name))


# ---- deep3: 3.94e9 directory entries ------------------------------------------------------------------------------------------------

def test_deep3_hot_path_against_the_oracle(oracle_mod, sessions):
    s = sessions("deep3")
    assert s.g.counters()["device_bytes"] > 4 * 1579 ** 3, "the directory alone is 15.7 GB"
    _hot_path(oracle_mod, "deep3", s.rows, s.occ, s.g.counters())


@pytest.mark.parametrize("opt", QUERY_OPTS, ids=QUERY_IDS)
def test_deep3_query(sessions, opt):
    _query(sessions("deep3"), opt)


@pytest.mark.parametrize("radius", [1, 2])
def test_deep3_mesh(sessions, radius):
    _mesh(sessions("deep3"), radius)


def test_deep3_raycast(sessions):
    """One general call of about 300 rays: the empty-space map has 3.94e9 cells (8 GB of byte maps), so its index has bit 31 set."""
    s = sessions("deep3")
    assert 2 ** 31 < faces.prod_bdims(s.dims) < 2 ** 32
    _raycast(s, (4, False), np.ascontiguousarray(faces.rays(s.model_box, s.res)[::10]))  # (302 rays; the reference alone: 164 hits)


def test_deep3_raycast_view_through_the_max_face(sessions):
    _raycast_view(sessions("deep3"))


@pytest.mark.parametrize("opt", COMP_OPTS, ids=COMP_IDS)
def test_deep3_components(sessions, opt):
    _components(sessions("deep3"), opt)


def test_deep3_compare_and_cover_own_mesh(sessions):
    _own_mesh(sessions("deep3"))


def test_deep3_compare_and_cover_a_displaced_mesh(sessions):
    _displaced_mesh(sessions("deep3"))


def test_deep3_align_own_mesh(sessions):
    _align(sessions("deep3"))


def test_deep3_two_huge_triangles_through_the_model(sessions):
    _huge_quad(sessions("deep3"))


def test_a_restored_deep3_handle_gives_the_same_bytes(hfpf_mod, sessions):
    """The brick_lin words of the blob exceed 2^31; the restore rebuilds a second 15.8 GB directory from them."""
    _restored_handle_gives_the_same_bytes(hfpf_mod, sessions("deep3"))


def test_deep3_the_read_outs_changed_nothing(sessions):
    _the_read_outs_changed_nothing(sessions("deep3"))


def test_deep3_clear_and_the_same_stream_again(sessions):
    """h2, and the last test of deep3: clear() resets the whole directory, the same stream then gives the same rows; closes the
    session."""
    s = sessions("deep3")
    try:
        s.g.clear()
        assert len(s.g.extract()) == 0 and len(s.g.occupied()) == 0
        rows = scenes.run(s.g, s.sc, "integrate")
        assert rows.tobytes() == s.rows.tobytes() and s.g.occupied().tobytes() == s.occ.tobytes()
    finally:
        s.close()
