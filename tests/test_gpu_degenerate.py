"""GPU: the plane fit where it degenerates -- flat, symmetric and tiny stencils -- and everything downstream of a row whose normal is NaN,
zero or arbitrary.  The models are those of tests/lattice.py (test_degenerate_oracle.py shows on the oracle alone that they contain
such rows):

a. the leaf: k_probe_normals against OracleGrid.probe_normal on every stencil family, every probe checked, totals 0, 1 and 2 included;
b. the hot path: k_normal's stencil from the neighbourhood() words, registration and replay of rows with such normals, against the
   oracle with exact moments -- NaN compared by position (sign and payload of a NaN are unspecified), everything else byte for byte;
c. every read-out on two such models against its numpy restatement, fed the engine's own rows."""
import numpy as np
import pytest

import components_ref as CR
import consistency_ref as CS
import cover_ref as V
import deviation_ref as D
import faces
import gpu_support as G
import hide_ref as HR
import lattice as L
import mesh_ref as M
import query_ref as Q
import raycast_ref as RC
import render_ref as R
import scenes
import track_ref as TR
from gpu_support import IDENT

pytestmark = pytest.mark.gpu
CAPS = dict(max_bricks=4096, max_log_points=1 << 18, max_normals=1 << 15, max_frames=64)
TINY = dict(max_bricks=1024, max_log_points=1 << 16, max_normals=1 << 12, max_frames=16)
ORACLE_COUNTERS = (("presented", "points_presented"), ("zclip_pass", "points_zclip_pass"), ("inserted", "points_in_bbox"),
                   ("occupied", "voxels_occupied"), ("normals", "voxels_with_normal"), ("buffered", "points_buffered"))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- a. the leaf ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shifted", [False, True], ids=["default", "shifted"])
@pytest.mark.parametrize("box", list(L.LEAF_BOXES))
def test_plane_fit_on_every_family(oracle_mod, hfpf_mod, box, shifted):
    res, bbox = L.LEAF_BOXES[box]
    og = oracle_mod.OracleGrid(resolution=res, bbox=bbox, pcl_shifted_cov=shifted)
    names, cells, occ, vps = L.leaf_inputs(og.dims[0], bbox, og.probe_center)
    t_ref, n_ref = L.leaf_reference(og, cells, occ, vps)
    dims = og.dims
    og.close()
    with hfpf_mod.OccupancyGrid(resolution=res, bbox=bbox, pcl_shifted_cov=shifted, **TINY) as g:
        assert g.dims == dims
        normals, totals = g.probe_normals(cells, occ, vps)
    nan_ref, nan_got = np.isnan(n_ref), np.isnan(normals)
    zero_ref = (n_ref == 0).all(axis=1)
    print("%s, %s: %d probes; oracle: %d NaN results (bits %s), %d zero results; engine: %d NaN results (bits %s)" % (
        box, "shifted" if shifted else "default", len(cells), nan_ref.any(axis=1).sum(), sorted({"0x%08X" % b for b in _bits(n_ref)[nan_ref]}),
        zero_ref.sum(), nan_got.any(axis=1).sum(), sorted({"0x%08X" % b for b in _bits(normals)[nan_got]})))
    bad = np.flatnonzero(totals != t_ref)
    assert not bad.size, "%d totals differ, first %s at %r: %d vs %d" % (bad.size, names[bad[0]], cells[bad[0]], totals[bad[0]], t_ref[bad[0]])
    bad = np.flatnonzero((nan_ref != nan_got).any(axis=1))
    assert not bad.size, "%d NaN masks differ (%r), first %s at %r: %r vs %r" % (
        bad.size, sorted(set(names[bad])), names[bad[0]], cells[bad[0]], normals[bad[0]], n_ref[bad[0]])
    same = (_bits(normals) == _bits(n_ref)) | nan_ref
    bad = np.flatnonzero(~same.all(axis=1))
    assert not bad.size, "%d normals differ (%r), first %s at %r, total %d: %r vs %r" % (
        bad.size, sorted(set(names[bad])), names[bad[0]], cells[bad[0]], t_ref[bad[0]], normals[bad[0]], n_ref[bad[0]])
    assert nan_ref.any(axis=1).sum() >= 20 and zero_ref.sum() >= 2 * L.LEAF_PER_FAMILY, "the run held too few NaN or zero results"
    assert all((t_ref == t).any() for t in (0, 1, 2)) and (t_ref < occ.sum(axis=1)).sum() >= 500, "totals 0, 1, 2 and clipped stencils"


# ---- b. the hot path --------------------------------------------------------------------------------------------------------------

def _hot_models():
    out = {}
    for tag, shift in (("0", (0.0, 0.0, 0.0)), ("128", faces.SHIFT_128), ("1024", faces.SHIFT_1024)):
        for axis in (2, 0):
            for layers in (1, 2):
                out["flat_%s%d_at_%s" % ("xyz"[axis], layers, tag)] = (L.flat_model, (shift, axis, layers))
    out["flat_z1_at_128_shifted_cov"] = (L.flat_model, (faces.SHIFT_128, 2, 1, True))
    out["flat_z1_at_1024_shifted_cov"] = (L.flat_model, (faces.SHIFT_1024, 2, 1, True))
    for gate in (0, 1, 2, 4):
        out["gate%d" % gate] = (L.low_gate_model, (gate,))
    for part in range(L.PLACEMENT_PARTS):
        out["placement%d" % part] = (L.placement_model, (part,))
    return out


HOT = _hot_models()
_models, _oracle_runs = {}, {}


def _model(name):
    """The model with its further layer and third clean, built once."""
    if name not in _models:
        make, args = HOT[name]
        _models[name] = make(*args, further=True)
    return _models[name]


def _oracle_run(oracle_mod, name):
    """(exact rows, occupied list, counters) of the oracle through the model's schedule, once per model (read-only)."""
    if name not in _oracle_runs:
        m = _model(name)
        og = oracle_mod.OracleGrid(resolution=m.resolution, bbox=m.bbox, exact_moments=True, **m.config)
        m.run(og, "capture")
        og.extract()
        exact, occ, ctr = og.extract_exact(), og.occupied(), og.counters()
        og.close()
        for a in (exact, occ):
            a.setflags(write=False)
        _oracle_runs[name] = (exact, occ, ctr)
    return _oracle_runs[name]


def _engine(hfpf_mod, m, **kw):
    return hfpf_mod.OccupancyGrid(resolution=m.resolution, bbox=m.bbox, **m.config, **dict(CAPS, **kw))


def _against_the_oracle(m, exact, occ_ref, ctr_ref, rows, occ, ctr, what):
    n, n_nan, n_zero, big = L.normal_counts(exact)
    print("%s: %d rows; oracle: %d NaN-normal rows (bits %s), %d zero-normal rows, |n_axis| > 0.99 at %r; engine: %d NaN-normal rows (bits %s), %d zero-normal rows" % (
        what, n, n_nan, L.nan_patterns(exact), n_zero, big, L.nan_mask(rows).sum(), L.nan_patterns(rows), L.zero_mask(rows).sum()))
    assert np.array_equal(occ_ref, occ), "%s: occupied lists differ (%d vs %d cells)" % (what, len(occ_ref), len(occ))
    assert len(exact) == len(rows), "%s: %d rows, the oracle has %d" % (what, len(rows), len(exact))
    for f in L.NORMAL_COLUMNS:
        bad = np.flatnonzero(np.isnan(exact[f]) != np.isnan(rows[f]))
        assert not bad.size, "%s: %s is NaN on one side only at %d rows, first (%d, %d, %d): %r vs the oracle's %r" % (
            what, f, bad.size, rows["ix"][bad[0]], rows["iy"][bad[0]], rows["iz"][bad[0]], rows[f][bad[0]], exact[f][bad[0]])
    rep = scenes.compare_rows_exact(L.canonical_nans(exact), L.canonical_nans(rows))
    assert rep["exact_bytes_differing"] == 0
    for a, b in ORACLE_COUNTERS:
        assert ctr_ref[a] == ctr[b], "%s: counter %s: %d, the oracle's %s %d" % (what, b, ctr[b], a, ctr_ref[a])
    odd = L.nan_mask(rows) | L.zero_mask(rows)
    assert (rows["count"][odd] == 0).all(), "%s: a row with a NaN or zero normal has members" % what


@pytest.mark.parametrize("binned", [True, False], ids=["binned", "direct"])
@pytest.mark.parametrize("name", list(HOT))
def test_hot_path_against_the_oracle(oracle_mod, hfpf_mod, name, binned):
    m = _model(name)
    exact, occ_ref, ctr_ref = _oracle_run(oracle_mod, name)
    assert len(exact) <= 5000 and m.max_points <= 12000 and len(m.ops) == 9
    with _engine(hfpf_mod, m, binned_update=binned) as g:
        assert g.dims[0] == L.DIMS
        m.run(g, "integrate")
        rows, occ, ctr = g.extract().copy(), g.occupied().copy(), g.counters()
    _against_the_oracle(m, exact, occ_ref, ctr_ref, rows, occ, ctr, "%s, %s" % (m.name, "binned" if binned else "direct"))
    assert ctr["clean_passes"] == 3 and ctr["frames_integrated"] == 6


def test_the_hot_models_hold_what_they_are_for(oracle_mod):
    """Over the models above, on the oracle's side: NaN normals far from the origin, none near it on one layer or with the shifted
    covariance, zero normals at gates 0 and 1, and cells that held a NaN normal in the stencils of the third pass's candidates."""
    nan = {name: int(L.nan_mask(_oracle_run(oracle_mod, name)[0]).sum()) for name in HOT}
    zero = {name: int(L.zero_mask(_oracle_run(oracle_mod, name)[0]).sum()) for name in HOT}
    print("NaN-normal rows: %r\nzero-normal rows: %r" % (nan, {k: v for k, v in zero.items() if v}))
    assert nan["flat_z1_at_128"] >= 20 and nan["flat_z1_at_1024"] >= 10 and nan["flat_z2_at_128"] >= 10 and nan["flat_x2_at_128"] >= 10
    assert nan["flat_z1_at_0"] == 0 and nan["flat_x1_at_0"] == 0 and nan["flat_z1_at_128_shifted_cov"] == 0 and nan["flat_z1_at_1024_shifted_cov"] == 0
    assert zero["gate0"] >= 10 and zero["gate1"] >= 10 and nan["gate0"] >= 50 and nan["gate2"] >= 50 and nan["gate4"] >= 10
    assert all(zero[k] == 0 for k in HOT if k not in ("gate0", "gate1"))
    assert sum(nan["placement%d" % p] for p in range(L.PLACEMENT_PARTS)) >= 20


# ---- c. the read-outs -------------------------------------------------------------------------------------------------------------

VIEW_K, VIEW_W, VIEW_H = (150.0, 150.0, 79.5, 59.5), 160, 120   # the models' own camera sees most of the box
PACKED = dict(point_step=16, off_x=0, off_y=4, off_z=8)
STEP = 0.5
SESSIONS = {"flat128": "flat_z1_at_128", "gate0": "gate0"}


class _Session:
    def __init__(self, hfpf_mod, key):
        self.key, self.H, self.m = key, hfpf_mod, _model(SESSIONS[key])
        self.bbox, self.res, self.dims = self.m.bbox, float(np.float32(self.m.resolution)), L.DIMS
        self.g = _engine(hfpf_mod, self.m)
        try:
            self.m.run(self.g, "integrate")
            self.rows, self.occ = self.g.extract().copy(), self.g.occupied().copy()
        except BaseException:
            self.g.close()
            raise
        self.nan, self.zero = L.nan_mask(self.rows), L.zero_mask(self.rows)
        for a in (self.rows, self.occ, self.nan, self.zero):
            a.setflags(write=False)
        print("%s: %d rows, %d with a NaN normal, %d with a zero normal, %d live" % (key, len(self.rows), self.nan.sum(), self.zero.sum(), (self.rows["count"] > 0).sum()))

    def odd(self):
        """Every read-out test begins here: the rows it is given hold NaN normals (and, at gate 0, zero normals)."""
        assert self.nan.sum() >= 20, "%s: %d rows with a NaN normal" % (self.key, self.nan.sum())
        assert self.key != "gate0" or self.zero.sum() >= 10, "%s: %d rows with a zero normal" % (self.key, self.zero.sum())
        assert (self.rows["count"] > 0).sum() >= 20, "%s: no live rows" % self.key
        return self

    def quad(self):
        """(vertices, triangles, pose): two triangles through the patch's layer (the box's middle at gate 0), in a frame whose origin is
        the box's minimum corner; at gate 0 a third, small one about the fusion frame's origin, where the rows without members lie."""
        lo, _ = faces.lo_hi(self.bbox)
        z = (41 + 0.5) * self.res
        v = [[0.05, 0.02, z], [0.17, 0.02, z], [0.17, 0.14, z], [0.05, 0.14, z]]
        t = [[0, 1, 2], [0, 2, 3]]
        if self.key == "gate0":
            v += [list(-lo + np.array(d)) for d in ((-0.01, -0.01, 0.0005), (0.01, -0.01, 0.0005), (0.0, 0.01, 0.0005))]
            t += [[4, 5, 6]]
        return np.array(v, np.float32), np.array(t, np.uint32), np.hstack([np.eye(3), lo.reshape(3, 1)])


@pytest.fixture(scope="module")
def sessions(hfpf_mod):
    made = {}

    def get(key):
        if key not in made:
            made[key] = _Session(hfpf_mod, key)
        return made[key].odd()

    yield get
    for s in made.values():
        s.g.close()


KEYS = list(SESSIONS)


@pytest.mark.parametrize("key", KEYS)
def test_extract_filtered(sessions, key):
    s = sessions(key)
    G.same_records(s.g.extract_filtered(min_count=0.0), s.rows, "%s: min_count 0" % key, "rows")
    kept = s.rows[s.rows["count"].astype(np.int32) >= 1]
    G.same_records(s.g.extract_filtered(min_count=1.0), kept, "%s: min_count 1" % key, "rows")
    assert not L.nan_mask(kept).any() and not L.zero_mask(kept).any() and 0 < len(kept) < len(s.rows)
    painted = s.g.extract_filtered(min_count=0.0, classify_threshold=1, paint_white=True)
    assert len(painted) == len(s.rows) and np.array_equal(_bits(painted["nx"]), _bits(s.rows["nx"]))


@pytest.mark.parametrize("key", KEYS)
def test_render(sessions, key):
    """A render draws rows with count >= max(1, min_count): no row with a NaN or zero normal is ever drawn, the arbitrary normals are."""
    s = sessions(key)
    for cull in (False, True):
        flags = R.WORLD_NORMALS | (R.CULL_BACKFACES if cull else 0)
        got = s.g.render(s.m.pose, VIEW_K, VIEW_W, VIEW_H, planes=("depth", "normal", "count", "voxel"), z_range=(0.05, 3.0), min_count=0.0,
                         splat_radius=1, max_splat_radius=4, cull_backfaces=cull, world_normals=True)
        ref = R.render(s.rows, s.m.pose, VIEW_K, VIEW_W, VIEW_H, s.res, (0.05, 3.0), 0.0, 1, 4, flags)
        G.same_planes(got, ref, "%s, cull %r" % (key, cull))
        drawn = ~np.isnan(got["depth"])
        print("%s, cull %r: %d pixels drawn" % (key, cull, drawn.sum()))
        assert drawn.sum() >= 100 and (got["count"][drawn] >= 1).all() and not np.isnan(got["normal"][drawn]).any()


def _query_points(s):
    pts = faces.query_points(s.rows, s.bbox, s.res, s.dims, per_face=500, per_value=40)
    lo, _ = faces.lo_hi(s.bbox)
    rng = np.random.default_rng(0xDE6)
    cells = np.stack([s.rows["ix"], s.rows["iy"], s.rows["iz"]], axis=1).astype(np.float64)
    own = (lo + (cells + rng.uniform(0.05, 0.95, cells.shape)) * s.res).astype(np.float32)   # a point in every row's own cell
    return np.ascontiguousarray(np.vstack([pts, own])), len(own)


@pytest.mark.parametrize("key", KEYS)
def test_query(sessions, key):
    s = sessions(key)
    pts, n_own = _query_points(s)
    kw = dict(radius=2, min_count=0.0)
    got = s.g.query(pts, IDENT, **kw)
    ref = Q.query(s.rows, s.occ, pts, IDENT, s.bbox, s.res, **kw)
    G.same_query(got, ref, key)
    f = got[0]["flags"][-n_own:]
    in_odd = f[s.nan | s.zero]
    print("%s: %d points, %d found; of the %d in the cell of a row without a usable normal: %d occupied, %d with a row, %d found" % (
        key, len(pts), (got[0]["flags"] & Q.FOUND != 0).sum(), len(in_odd), (in_odd & Q.OCCUPIED != 0).sum(), (in_odd & Q.HAS_ROW != 0).sum(),
        (in_odd & Q.FOUND != 0).sum()))
    assert (f & Q.FOUND != 0).sum() >= 20 and (in_odd & Q.OCCUPIED != 0).sum() >= 20


@pytest.mark.parametrize("key", KEYS)
def test_mesh(sessions, key):
    s = sessions(key)
    kw = dict(radius=2, min_count=0.0)
    rv, rt, sizes, _ = M.mesh(s.rows, s.occ, s.bbox, s.res, s.dims, with_ends=True, **kw)
    G.same_mesh(s.g.extract_mesh(**kw), (rv, rt), "%s, host form" % key)
    G.same_mesh(G.mesh_device(s.g, **kw), (rv, rt), "%s, device form" % key)
    print("%s: %d vertices, %d triangles, %r" % (key, len(rv), len(rt), sizes))
    assert len(rt) >= 20


@pytest.mark.parametrize("key", KEYS)
def test_raycast(sessions, key):
    s = sessions(key)
    kw = dict(radius=2, cull_backfaces=True, step=STEP, t_range=(0.0, faces.ray_t_max(s.bbox, s.res, STEP)))
    rays = faces.rays(s.bbox, s.res)[::3]
    ref = RC.raycast(s.rows, s.occ, rays, IDENT, s.bbox, s.res, **kw)
    hit = ref["flags"] & RC.HIT != 0
    print("%s: %d rays, %d hits" % (key, len(rays), hit.sum()))
    G.same_rays(s.g.raycast(rays, IDENT, **kw), ref, "%s, host form" % key)
    G.same_rays(G.rays_device(s.g, rays, IDENT, **kw), ref, "%s, device form" % key)
    lo, hi = faces.lo_hi(s.bbox)
    vkw = dict(radius=2, cull_backfaces=True, step=STEP, t_range=(0.06, 0.08 + float(hi[2] - lo[2]) + 0.01))
    pose, K = faces.outside_view(s.bbox, 64, 48)
    view = RC.raycast_view(s.rows, s.occ, pose, K, 64, 48, s.bbox, s.res, **vkw)
    G.same_rays(s.g.raycast_view(pose, K, 64, 48, **vkw), view, "%s, view" % key)
    print("%s: view through the z-min face: %d hits" % (key, (view["flags"] & RC.HIT != 0).sum()))
    assert hit.sum() + (view["flags"] & RC.HIT != 0).sum() >= 20


@pytest.mark.parametrize("key", KEYS)
def test_components(sessions, key):
    """A NaN compares false: under a normal gate a row with a NaN normal joins nothing; a zero normal has dot 0 with everything."""
    s = sessions(key)
    for kw in (dict(reach=2, min_normal_dot=0.9), dict(reach=2, min_normal_dot=0.0), dict(reach=1)):
        ref = CR.components(s.rows, **kw)
        got = s.g.extract_components(**kw)
        G.same_components(got, ref, "%s %r" % (key, kw))
        G.same_components(G.components_device(s.g, s.H, **kw), ref, "%s, device form %r" % (key, kw))
        rows, labels, comps = got
        print("%s %r: %d rows in %d components, largest %d" % (key, kw, len(rows), len(comps), comps["n_rows"].max()))
        assert rows.tobytes() == s.rows.tobytes()
        if "min_normal_dot" in kw:
            assert (comps["n_rows"][labels[s.nan]] == 1).all(), "a row with a NaN normal joined a component under a normal gate"


def _depth_frames(s):
    poses = [s.m.pose, G.perturb(s.m.pose, 1.0, (0.002, -0.001, 0.001))]
    frames = [s.g.render(p, VIEW_K, VIEW_W, VIEW_H, planes=("depth",), z_range=(0.05, 3.0), min_count=1.0, splat_radius=1)["depth"] for p in poses]
    far = frames[0].copy()   # the first view again with its left half 30 mm farther: the rows in front of it are seen through
    far[:, :VIEW_W // 2] += np.float32(0.03)
    return np.stack(frames + [far]), np.stack(poses + [poses[0]])


@pytest.mark.parametrize("key", KEYS)
def test_depth_consistency(sessions, key):
    s = sessions(key)
    frames, poses = _depth_frames(s)
    assert frames.dtype == np.float32 and np.isfinite(frames).sum() >= 300
    for kw in (dict(window=1, tolerance=0.004, min_cos=0.3, min_through=1, through_ratio=0.0), dict(window=0, tolerance=0.002, min_cos=-1.0, min_through=1, through_ratio=0.0)):
        rows, cons, summary = s.g.depth_consistency(frames, poses, VIEW_K, **kw)
        r_rows, r_cons, r_summary = CS.consistency(s.rows, frames, poses, VIEW_K, **kw)
        print("%s %r: %r" % (key, kw, summary))
        G.same_records((rows, cons), (r_rows, r_cons), "%s %r" % (key, kw), ("rows", "records"))
        G.same_summary(summary, r_summary, CS.SUMMARY_KEYS, "%s %r" % (key, kw))
        assert summary["n_seen"] >= 20 and summary["n_rows"] == len(s.rows)
        if kw["min_cos"] >= 0:
            assert not (cons["n_tested"][s.nan | s.zero] > 0).any(), "a row with a NaN or zero normal passed the facing gate"


@pytest.mark.parametrize("key", KEYS)
def test_compare_and_cover_a_quad(sessions, key):
    s = sessions(key)
    verts, tris, pose = s.quad()
    for md in (3 * s.res, 0.05):
        got = s.g.compare_mesh(verts, tris, pose, max_distance=md)
        G.same_deviation(got, D.compare(s.rows, verts, 12, tris, pose, 0.0, md), "%s, %g m" % (key, md))
        found = got[0]["flags"] & D.FOUND != 0
        print("%s, %g m: found %d of %d rows (%d of those with a NaN or zero normal), %d negative" % (
            key, md, found.sum(), len(s.rows), found[s.nan | s.zero].sum(), got[1]["n_negative"]))
        assert found.sum() >= 20
    if key == "gate0":  # the rows without members lie at the fusion frame's origin, under the third triangle
        assert found[s.nan | s.zero].all()
    for kw in (dict(min_normal_dot=0.5, abs_normal=True), dict(min_normal_dot=0.5), dict()):
        reach = 4 if key == "gate0" else 2   # the lines and single cells of gate 0 lie farther from the quad than a patch it runs through
        kw = dict(kw, radius=reach, max_distance=reach * s.res, spacing=s.res)
        got = s.g.cover_mesh(verts, tris, pose, **kw)
        G.same_coverage(got, V.cover(s.rows, s.occ, verts, 12, tris, pose, s.bbox, s.res, **kw), "%s %r" % (key, kw))
        G.coverage_sums(*got)
        print("%s %r: %d samples, %d in the box, %d covered" % (key, kw, got[1]["n_samples"], got[1]["n_in_bbox"], got[1]["n_covered"]))
    assert got[1]["n_in_bbox"] >= 1000


@pytest.mark.parametrize("key", KEYS)
def test_track(sessions, key):
    """One of the model's own frames from a slightly perturbed pose.  The model view draws rows with members only, so the guard on
    the normal's length in the reduction is not reached through rows of the hot path: their normals are unit vectors or the row has
    no member."""
    s = sessions(key)
    cloud = s.m.ops[0][1]
    guess = G.perturb(s.m.pose, 0.3, (0.0006, -0.0005, 0.0006))
    o = dict(G.TRACK_OPTS)
    got = s.g.track(cloud, PACKED, guess, VIEW_K, VIEW_W, VIEW_H, stride=1, **o)
    view = dict(K=VIEW_K, width=VIEW_W, height=VIEW_H, z_range=G.Z_RANGE, splat_radius=-1, max_splat_radius=4, flags=1)
    ref = TR.track(s.rows, TR.cloud_points(cloud[:, :3], 1), guess, s.res, view, G.Z_CLIP, max_iterations=o["max_iterations"], min_inliers=6,
                   max_distance=o["max_distance"], damping=o["damping"], eps_rotation=o["eps_rotation"], eps_translation=o["eps_translation"])
    print("%s: %d iterations, flags %d, %d of %d used points inliers, rms %.2e, error %s -> %s" % (
        key, got[1]["iterations"], got[1]["flags"], got[1]["inliers"], got[1]["points_used"], got[1]["rms"], G.pose_errors(guess, s.m.pose),
        G.pose_errors(got[0], s.m.pose)))
    G.same_track(got, ref, key)
    assert ref["points_used"] == len(cloud) and ref["inliers"] >= 6


@pytest.mark.parametrize("key", KEYS)
def test_hide_exactly_the_nan_rows(sessions, key):
    s = sessions(key)
    vox = HR.row_voxels(s.rows).astype(np.int32)
    select = np.ascontiguousarray(s.nan.astype(np.uint32))
    s.g.show_all()
    try:
        got = s.g.hide_voxels(s.rows, "hide", select=select, select_mask=1, select_value=1)
        H_ref, want = HR.hide_voxels(s.rows, None, s.dims, vox, "hide", select, 1, 1)
        assert got == want and got["n_hidden"] == int(s.nan.sum()), (got, want)
        assert s.g.hidden().tobytes() == np.ascontiguousarray(vox[s.nan]).tobytes(), "the hidden set is not the NaN-normal rows' voxels"
        left = s.g.extract()
        G.same_records(left, s.rows[~s.nan], "%s: extract with the NaN-normal rows hidden" % key, "rows")
        assert not L.nan_mask(left).any()
        G.same_components(s.g.extract_components(reach=2, min_normal_dot=0.9), CR.components(HR.visible(s.rows, H_ref), reach=2, min_normal_dot=0.9), "%s, hidden" % key)
    finally:
        s.g.show_all()
    G.same_records(s.g.extract(), s.rows, "%s: extract after show_all" % key, "rows")


@pytest.mark.parametrize("key", KEYS)
def test_snapshot_and_restore(hfpf_mod, sessions, key):
    s = sessions(key)
    blob = s.g.snapshot()
    with _engine(hfpf_mod, s.m) as g2:
        g2.restore(blob)
        G.same_records(g2.extract(), s.rows, "%s: extract of the restored handle" % key, "rows")
        assert g2.occupied().tobytes() == s.occ.tobytes()
        assert G.contract_counters(g2) == G.contract_counters(s.g)
        a = s.g.extract_components(reach=2, min_normal_dot=0.9)
        b = g2.extract_components(reach=2, min_normal_dot=0.9)
        G.same_components(b, a, "%s: components of the restored handle" % key)


@pytest.mark.parametrize("key", KEYS)
def test_the_read_outs_changed_nothing(sessions, key):
    s = sessions(key)
    G.same_records(s.g.extract(), s.rows, "%s: extract" % key, "rows")
    assert s.g.occupied().tobytes() == s.occ.tobytes()
