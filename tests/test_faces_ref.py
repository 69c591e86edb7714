"""CPU: the numpy restatements of the read-outs at the faces of the grid.  The references of query, mesh and raycast are written for any
box and any dims, and had only ever run on models more than 100 voxels from every face; here they run on the CPU oracle's rows and
occupied list of the scenes of tests/faces.py and are checked against their own independent forms: with `deepy` also at cell indices
up to 2^21 - 2 in the middle field of their 21-bit keys, where a window reaches past 2^21 and a carry would land in x.  This is also
the one place where the oracle's figures for the scenes are asserted exactly."""
import warnings

import numpy as np
import pytest

import components_ref as CR
import faces
from gpu_support import IDENT
import mesh_ref as M
import query_ref as Q
import raycast_ref as RC
import scenes

_MODELS = {}


def _model(oracle_mod, synth_mod, name):
    """(scene, rows, occupied, dims, res) of the oracle alone, computed once per scene."""
    if name not in _MODELS:
        sc = faces.FaceScene(name)
        og = oracle_mod.OracleGrid(resolution=sc.resolution, bbox=sc.bbox, fuse_color=True, **sc.config)
        rows = scenes.run(og, sc, "capture", color=True)
        occ = og.occupied()
        dims, res = og.dims
        og.close()
        _MODELS[name] = (sc, rows, occ, dims, res)
    return _MODELS[name]


@pytest.fixture(params=["cut", "thin", "deepy"])
def model(request, oracle_mod, synth_mod):
    return _model(oracle_mod, synth_mod, request.param)


@pytest.mark.parametrize("name", faces.ALL)
def test_the_scenes_are_what_the_oracle_says(oracle_mod, synth_mod, name):
    sc, rows, occ, dims, res = _model(oracle_mod, synth_mod, name)
    assert faces.face_counts(rows, occ, dims) == faces.ORACLE_TABLE[name]
    faces.check_conditions(name, rows, occ, dims)
    if name == "cut":  # every dim a multiple of 8: the index-dim cells sit alone in the last brick of their axis
        assert all(d % 8 == 0 for d in dims) and [(d + 1 + 7) // 8 for d in dims] == [14, 10, 12]
    if name == "far":
        assert np.abs(np.asarray(sc.bbox)).min() > 1.5
    if name.startswith("far137"):
        assert np.abs(np.asarray(sc.bbox)).min() > 23
    if name in faces.DYADIC:
        lo, hi = faces.lo_hi(sc.bbox)
        assert res == faces.DYADIC_RES and np.array_equal((hi - lo) / res, np.asarray(dims, np.float64)), "a box of whole cells"
        assert np.array_equal(np.asarray(sc.bbox, np.float32).astype(np.float64), np.asarray(sc.bbox))
        assert faces.boundary_counts(sc) == faces.BOUNDARY_TABLE[name]
    if name in faces.DEEP:
        assert tuple(dims) == faces.DEFS[name][3] and sc.model_box == faces.CUT_BBOX
        assert faces.lo_hi(sc.bbox)[1].tolist() == faces.lo_hi(faces.CUT_BBOX)[1].tolist(), "the max corner is CUT_BBOX's"
        if name == "deep3":
            assert 2 ** 31 < faces.prod_bdims(dims) <= 4.0e9 and faces.prod_bdims(tuple(d + 72 for d in dims)) > 4.0e9
        else:
            assert max(dims) == 2097150 == (1 << 21) - 2, "the largest axis hfpf_create takes: index == dim sets every bit but the lowest"


def test_key_widths_and_brick_lin():
    """faces.key_widths against hfpf_create's loop, written out; faces.brick_lin on hand-made rows."""
    for d in (1, 2, 3, 6, 7, 8, 72, 127, 128, 12630, (1 << 20) - 1, 1 << 20, 2097149, 2097150):
        b = 1
        while (1 << b) <= d:
            b += 1
        assert faces.key_widths((d, d, d)) == (b, b, b), d
    assert faces.key_widths((2097150, 72, 88)) == (21, 7, 7) and faces.key_widths((12630,) * 3) == (14, 14, 14)
    rows = np.zeros(3, [("ix", "<i4"), ("iy", "<i4"), ("iz", "<i4")])
    rows["ix"], rows["iy"], rows["iz"] = (0, 8, 12629), (7, 0, 12629), (15, 23, 12629)
    assert faces.brick_dims((12630,) * 3) == (1579,) * 3
    assert faces.brick_lin(rows, (12630,) * 3).tolist() == [1, 1579 * 1579 + 2, 1579 ** 3 - 1] and 1579 ** 3 - 1 > 2 ** 31


def test_components_on_a_deep_model_are_the_brute_force_ones(oracle_mod, synth_mod):
    """components_ref on rows at iy 2096998..2097149 (the middle key field: a carry out of it would land in x, and the window of a
    row at dim - 1 reaches dim + 3 >= 2^21) against a form that uses no key at all: the pairs from the Chebyshev distance of every two
    rows, the labels from a flood fill over them."""
    sc, rows, occ, dims, res = _model(oracle_mod, synth_mod, "deepy")
    rows = np.ascontiguousarray(rows).view(CR.ROW_DTYPE).reshape(-1)
    assert rows["iy"].max() + 4 >= 1 << CR.KEY_BITS
    v = np.stack([rows["ix"], rows["iy"], rows["iz"]], axis=1).astype(np.int32)
    cheb = []   # per 1000 rows, their Chebyshev distance to every row, cut at 100
    for i in range(0, len(v), 1000):
        d = np.abs(v[i:i + 1000, None, 0] - v[None, :, 0])
        for k in (1, 2):
            np.maximum(d, np.abs(v[i:i + 1000, None, k] - v[None, :, k]), out=d)
        cheb.append(np.minimum(d, 100).astype(np.int8))
    for reach, dot in ((1, -2.0), (2, 0.9), (4, -2.0)):
        a, b = CR.neighbour_pairs(rows, reach)
        pa, pb = (np.concatenate(x) for x in zip(*[np.nonzero(c <= reach) for c in cheb]))
        pa = pa + np.repeat(np.arange(0, len(v), 1000), [int((c <= reach).sum()) for c in cheb])
        up = pa < pb
        assert sorted(zip(a.tolist(), b.tolist())) == sorted(zip(pa[up].tolist(), pb[up].tolist())), "reach %d: the pair lists differ" % reach
        ok = CR.normal_gate(rows, pa, pb, dot)
        adj = [[] for _ in range(len(rows))]
        for x, y in zip(pa[ok].tolist(), pb[ok].tolist()):
            adj[x].append(y)
        seen = np.full(len(rows), -1)
        for s in range(len(rows)):
            if seen[s] < 0:
                seen[s] = s
                stack = [s]
                while stack:
                    for y in adj[stack.pop()]:
                        if seen[y] < 0:
                            seen[y] = s
                            stack.append(y)
        out = CR.components(rows, reach=reach, min_normal_dot=dot)
        print("deepy, reach %d, dot %g: %d pairs, %d components" % (reach, dot, up.sum(), len(out[2])))
        assert np.array_equal(out[2]["source_row"][out[1]], seen), (reach, dot)
        assert 1 < len(out[2]) < len(rows) and (out[2]["hi"][:, 1] == dims[1] - 1).any()


def test_near_the_origin_the_dyadic_box_meets_next_to_no_boundary(synth_mod):
    """What the shift is for: the same box and stream without it put 2 of 58,271 points on a cell boundary."""
    sc = faces.FaceScene("dy128s")
    sc.bbox, sc.poses = faces.DYADIC_BBOX, sc.render_poses
    assert faces.boundary_counts(sc) == (58271, 2, 1)


@pytest.mark.parametrize("name", ["far137s", "dy128s"])
def test_nearest_ties_is_the_brute_force_count(oracle_mod, synth_mod, name):
    """query_ref.nearest_ties against a scan of every candidate row per point, on 3000 of the scene's query points."""
    sc, rows, occ, dims, res = _model(oracle_mod, synth_mod, name)
    pts = faces.query_points(rows, sc.bbox, res, dims)
    pts = pts[np.random.default_rng(7).choice(len(pts), 3000, replace=False)]
    cand = Q.candidates(rows, 0.0)
    cv = np.stack([cand["ix"], cand["iy"], cand["iz"]], axis=1).astype(np.int64)
    cxyz = faces.centroids(cand).astype(np.float64)
    for radius in (1, 3):
        hits, _ = Q.query(rows, occ, pts, IDENT, sc.bbox, res, radius=radius)
        tied = Q.nearest_ties(rows, hits, pts, radius)
        want = np.zeros(len(pts), bool)
        for i in np.flatnonzero(hits["flags"] & Q.FOUND != 0):
            near = np.abs(cv - hits["voxel"][i].astype(np.int64)).max(axis=1) <= radius
            d = pts[i].astype(np.float64) - cxyz[near]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            want[i] = (d2 == d2.min()).sum() >= 2
        print("%s, radius %d: %d of %d found points tie" % (name, radius, want.sum(), (hits["flags"] & Q.FOUND != 0).sum()))
        assert np.array_equal(tied, want)
        assert want.sum() >= 1, "a scene without ties shows nothing"


@pytest.mark.parametrize("radius", [0, 1, 2, 3, 4])
def test_query_is_the_brute_force_scan(model, radius):
    sc, rows, occ, dims, res = model
    pts = faces.query_points(rows, sc.bbox, res, dims)
    pts = pts[np.random.default_rng(radius).choice(len(pts), 1500, replace=False)]
    for kw in (dict(), dict(min_count=3.0), dict(max_distance=1.5 * res)):
        a = Q.query(rows, occ, pts, IDENT, sc.bbox, res, radius=radius, **kw)
        b = Q.brute_force(rows, occ, pts, IDENT, sc.bbox, res, radius=radius, **kw)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), kw
    f = a[0]["flags"]
    at_dim = (f & Q.IN_BBOX != 0) & (a[0]["voxel"] == np.asarray(dims)).any(axis=1)
    assert at_dim.any() and not (f[at_dim] & Q.HAS_ROW).any()
    assert (f & Q.IN_BBOX == 0).any()


def test_mesh_agrees_with_the_unwelded_construction_and_stays_in_the_box(model):
    sc, rows, occ, dims, res = model
    v, t, sizes = M.mesh(rows, occ, sc.bbox, res, dims, radius=2)
    assert len(t) > 1000 and t.max() < len(v)
    loose = M.mesh_unwelded(rows, occ, sc.bbox, res, dims, radius=2)
    welded = M.positions(v)[np.asarray(t, np.int64)]
    assert loose.shape == welded.shape
    assert loose.tobytes() == welded.tobytes()
    lo, hi = faces.lo_hi(sc.bbox)
    p = M.positions(v).astype(np.float64)
    assert (p >= lo).all() and (p <= hi).all(), "a vertex outside the closed box"


def test_raycast_of_axis_parallel_and_in_face_rays_raises_no_warning(model):
    sc, rows, occ, dims, res = model
    sets = dict(faces.ray_sets(sc.model_box, res))
    rays = np.vstack([sets["axis-parallel"][::3], sets["in a face's plane"][::3]])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        h = RC.raycast(rows, occ, rays, IDENT, sc.bbox, res, radius=2, step=0.5, t_range=(0.0, faces.ray_t_max(sc.model_box, res)))
    assert (h["flags"] & RC.USED != 0).all() and (h["flags"] & RC.HIT != 0).any()


def test_a_ray_from_beyond_a_face_and_one_from_the_face_cross_at_the_same_point(model):
    """Two inward rays on one axis-parallel line, one starting on a face's plane and one m march steps before it, m chosen so that
    the outer origin is an f32 exactly: sample k + m of the outer ray is sample k of the inner one, bit for bit.  Both therefore see
    the same signed distances and rows: the same flags, the same crossing interval (the outer index is m larger), the same
    attributes; t and p are the same f64 expressions up to the association of a sum, so t differs by the offset and p is the same
    point, each to within one f32 spacing."""
    sc, rows, occ, dims, res = model
    t1 = faces.ray_t_max(sc.model_box, res) - 0.05
    n_hit = 0
    pairs = faces.face_pairs(sc.bbox, res, model_box=sc.model_box)
    assert len(pairs) >= 4
    for outer, inner, m, off in pairs:
        kw = dict(radius=2, step=0.5)
        ho = RC.raycast(rows, occ, outer, IDENT, sc.bbox, res, t_range=(0.0, t1 + off), **kw)
        hi = RC.raycast(rows, occ, inner, IDENT, sc.bbox, res, t_range=(0.0, t1), **kw)
        hit = hi["flags"] & RC.HIT != 0
        n_hit += int(hit.sum())
        assert np.array_equal(ho["flags"], hi["flags"])
        assert np.array_equal(ho["sample"][hit], hi["sample"][hit] + m)
        for k in ("row_voxel", "n", "rgb", "count"):
            assert ho[k].tobytes() == hi[k].tobytes(), k
        assert (np.abs(ho["p"][hit] - hi["p"][hit]) <= np.spacing(np.abs(hi["p"][hit]))).all()
        d = np.abs((ho["t"][hit].astype(np.float64) - hi["t"][hit].astype(np.float64)) - off)
        assert (d <= np.spacing(ho["t"][hit])).all()
    assert n_hit >= 30
