"""CPU: the raycast contract (tests/raycast_ref.py) on hand-built rows with known answers, hfpf_check_raycast_opts, and the ctypes /
numpy mirrors of the raycast structs against include/hfpf.h."""
import ctypes as C
import os
import re

import numpy as np

import hfpf
import raycast_ref as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.01
BBOX = (0.0, 0.2, 0.0, 0.2, 0.0, 0.2)  # 20 cells per axis
IDENT = RC.IDENT
STEP = 0.5
DT = STEP * RES


def layer(kz, normal, rgb=0x102030, count=3):
    """Rows in every cell (i, j, kz), centroid at the cell centre, one normal."""
    r = np.zeros(400, dtype=hfpf.ROW_DTYPE)
    i, j = np.divmod(np.arange(400), 20)
    r["ix"], r["iy"], r["iz"] = i, j, kz
    r["x"], r["y"], r["z"] = RES * i + RES / 2, RES * j + RES / 2, RES * kz + RES / 2
    r["nx"], r["ny"], r["nz"] = normal
    r["count"] = count
    r["rgb"] = rgb
    return r


def model(*layers):
    r = np.concatenate(layers)
    return r[np.lexsort((r["iz"], r["iy"], r["ix"]))]


def cast(rows, rays, pose=IDENT, **kw):
    occ = np.stack([rows["ix"], rows["iy"], rows["iz"]], axis=1) if len(rows) else np.zeros((0, 3), np.int32)
    kw.setdefault("step", STEP)
    kw.setdefault("t_range", (0.0, 0.3))
    return RC.raycast(rows, occ, np.asarray(rays, np.float32).reshape(-1, 6), pose, BBOX, RES, **kw)


def assert_no_hit(h, flags):
    assert (h["flags"] == flags).all()
    for k in ("t", "p", "n"):
        assert (h[k].view(np.uint32) == RC.NAN_BITS).all()
    assert (h["row_voxel"] == -1).all() and not h["rgb"].any() and not h["count"].any() and not h["sample"].any()
    assert not h["reserved"].any()


# ---- the options check (absent from the engine before the raycast) --------------------------------------------------------

def test_the_options_check():
    L = hfpf.lib()
    assert L.hfpf_check_raycast_opts(C.byref(hfpf.raycast_opts())) == 0
    for r in (1, 4):
        assert L.hfpf_check_raycast_opts(C.byref(hfpf.raycast_opts(radius=r, min_count=-1.0, max_distance=1e-6, step=0.125, t_range=(0.0, 1e-3)))) == 0
    assert L.hfpf_check_raycast_opts(C.byref(hfpf.raycast_opts(step=4.0, max_distance=float("inf"), cull_backfaces=True))) == 0
    nan, inf = float("nan"), float("inf")
    bad = [("struct_size", 56), ("flags", 2), ("reserved0", 1), ("reserved", 1), ("radius", 0), ("radius", 5), ("min_count", nan),
           ("max_distance", 0.0), ("max_distance", -1.0), ("max_distance", nan), ("step", 0.1), ("step", 4.5), ("step", nan), ("step", inf),
           ("t_min", -0.1), ("t_min", nan), ("t_min", 1.0), ("t_min", 2.0), ("t_max", inf), ("t_max", nan)]
    for field, val in bad:
        o = hfpf.raycast_opts()
        setattr(o, field, val)
        assert L.hfpf_check_raycast_opts(C.byref(o)) == -2, (field, val)
    assert L.hfpf_check_raycast_opts(None) == -2


def test_struct_mirrors_match_the_header():
    text = open(os.path.join(ROOT, "include", "hfpf.h")).read()
    for name, size in (("hfpf_ray", 24), ("hfpf_raycast_opts", 64), ("hfpf_ray_hit", 64)):
        assert re.search(r"static_assert\(sizeof\(%s\) == %d" % (name, size), text), name
    assert C.sizeof(hfpf.RaycastOpts) == 64 and hfpf.RAY_DTYPE.itemsize == 24 and hfpf.RAY_HIT_DTYPE.itemsize == 64
    assert hfpf.RAY_HIT_DTYPE == RC.HIT_DTYPE and hfpf.RAY_DTYPE == RC.RAY_DTYPE
    for py, c in (("RAY_USED", "HFPF_RAY_USED"), ("RAY_HIT", "HFPF_RAY_HIT"), ("RAY_BACKFACE", "HFPF_RAY_BACKFACE"), ("RAY_NEAR", "HFPF_RAY_NEAR"),
                  ("RAYCAST_CULL_BACKFACES", "HFPF_RAYCAST_CULL_BACKFACES")):
        assert getattr(hfpf, py) == int(re.search(r"#define\s+%s\s+(\d+)u" % c, text).group(1)), c
    assert (RC.USED, RC.HIT, RC.BACKFACE, RC.NEAR) == (hfpf.RAY_USED, hfpf.RAY_HIT, hfpf.RAY_BACKFACE, hfpf.RAY_NEAR)


def test_sample_count():
    assert RC.n_samples(0.0, 0.3, 0.5, 0.01) == 61
    assert RC.n_samples(0.25, 0.26, 4.0, 0.01) == 1


# ---- a plane of rows facing the rays ----------------------------------------------------------------------------------------

def test_plane_crossing_is_the_analytic_one():
    rows = model(layer(10, (0.0, 0.0, -1.0)))  # the plane z = 0.105, seen from z < 0.105
    rng = np.random.default_rng(7)
    o = np.column_stack([rng.uniform(0.06, 0.14, 200), rng.uniform(0.06, 0.14, 200), np.full(200, 0.013)])
    d = np.column_stack([rng.uniform(-0.3, 0.3, 200), rng.uniform(-0.3, 0.3, 200), np.ones(200)]) * rng.uniform(0.5, 3.0, (200, 1))
    rays = np.hstack([o, d]).astype(np.float32)
    for radius in (1, 2, 4):
        h = cast(rows, rays, radius=radius)
        assert (h["flags"] == RC.USED | RC.HIT | RC.NEAR).all()
        O, D, _ = RC.general_rays(rays, IDENT)
        t_true = (0.105 - O[:, 2]) / D[:, 2]
        assert np.abs(np.linalg.norm(D, axis=1) - 1.0).max() < 1e-12
        assert np.abs(h["t"] - t_true).max() <= DT * 1.0            # dt * |D|, |D| = 1
        assert np.abs(h["p"][:, 2] - 0.105).max() <= DT
        assert (h["row_voxel"][:, 2] == 10).all() and (h["count"] == 3).all() and (h["rgb"] == 0x102030).all()
        assert (h["n"] == np.array([0, 0, -1], np.float32)).all()
        k = h["sample"].astype(np.float64)
        assert ((k - 1) * DT <= h["t"] + 1e-6).all() and (h["t"] <= k * DT + 1e-6).all()
    # a posed camera: the same rays given in a frame shifted by the pose
    T = np.hstack([np.eye(3), np.array([[0.01], [-0.02], [0.003]])])
    shifted = rays.copy()
    shifted[:, :3] -= T[:, 3].astype(np.float32)
    hs = cast(rows, shifted, pose=T, radius=2)
    assert np.abs(hs["t"] - t_true).max() <= DT


def test_view_rays_report_camera_depth():
    rows = model(layer(10, (0.0, 0.0, -1.0)))
    occ = np.stack([rows["ix"], rows["iy"], rows["iz"]], axis=1)
    T = np.hstack([np.eye(3), np.array([[0.1], [0.1], [0.013]])])
    K = (40.0, 40.0, 7.5, 5.5)
    h = RC.raycast_view(rows, occ, T, K, 16, 12, BBOX, RES, radius=2, step=STEP, t_range=(0.01, 0.25))
    assert h.shape == (12, 16) and (h["flags"] == RC.USED | RC.HIT | RC.NEAR).all()
    O, D, _ = RC.view_rays(T, K, 16, 12)
    assert (D[:, 2] == 1.0).all()
    assert np.abs(h["t"].ravel() - (0.105 - 0.013)).max() <= DT * np.linalg.norm(D, axis=1).max()


# ---- a two-layer slab and a wall behind it ----------------------------------------------------------------------------------

def slab():
    """Front face z = 0.085 (normal -z), back face z = 0.125 (normal +z), and a second wall z = 0.165 facing -z."""
    return model(layer(8, (0.0, 0.0, -1.0), rgb=1), layer(12, (0.0, 0.0, 1.0), rgb=2), layer(16, (0.0, 0.0, -1.0), rgb=3))


def test_back_crossings_are_flagged_and_culling_marches_on():
    rows = slab()
    outside = np.array([[0.1, 0.1, 0.013, 0, 0, 1]], np.float32)
    inside = np.array([[0.1, 0.1, 0.101, 0, 0, 1]], np.float32)
    h = cast(rows, outside, radius=1)[0]
    assert h["flags"] == RC.USED | RC.HIT | RC.NEAR and abs(h["t"] - (0.085 - 0.013)) <= DT and h["rgb"] == 1
    h = cast(rows, inside, radius=1)[0]      # starts inside the slab: leaves it through the back face
    assert h["flags"] == RC.USED | RC.HIT | RC.BACKFACE | RC.NEAR and abs(h["t"] - (0.125 - 0.101)) <= DT and h["rgb"] == 2
    h = cast(rows, inside, radius=1, cull_backfaces=True)[0]   # the back face does not end it: the wall behind does
    assert h["flags"] == RC.USED | RC.HIT | RC.NEAR and abs(h["t"] - (0.165 - 0.101)) <= DT and h["rgb"] == 3
    assert h["sample"] > cast(rows, inside, radius=1)[0]["sample"]
    # a front crossing ends a culled march as it ends a plain one
    assert cast(rows, outside, radius=1, cull_backfaces=True).tobytes() == cast(rows, outside, radius=1).tobytes()
    # the ray towards -z from behind everything meets the wall's back first
    h = cast(rows, np.array([[0.1, 0.1, 0.195, 0, 0, -1]], np.float32), radius=1)[0]
    assert h["flags"] & RC.BACKFACE and abs(h["t"] - (0.195 - 0.165)) <= DT


def test_a_gap_between_defined_samples_is_no_crossing():
    # the max_distance gate leaves only samples within 2 mm of a centroid defined: with 5 mm steps no two neighbours are
    h = cast(slab(), np.array([[0.105, 0.105, 0.013, 0, 0, 1]], np.float32), radius=1, max_distance=0.002, t_range=(0.002, 0.18))
    assert_no_hit(h, RC.USED | RC.NEAR)
    # and the count gate removes every row
    assert_no_hit(cast(slab(), np.array([[0.1, 0.1, 0.013, 0, 0, 1]], np.float32), min_count=4.0), RC.USED)


def test_unused_rays_misses_and_empty_models():
    rows = model(layer(10, (0.0, 0.0, -1.0)))
    nan, inf = np.nan, np.inf
    unused = np.array([[nan, 0.1, 0.01, 0, 0, 1], [0.1, 0.1, 0.01, 0, 0, 0], [0.1, 0.1, 0.01, inf, 0, 1], [0.1, inf, 0.01, 0, 0, 1]], np.float32)
    assert_no_hit(cast(rows, unused), 0)
    away = np.array([[0.1, 0.1, 0.013, 0, 0, -1], [0.5, 0.5, 0.5, 1, 0, 0]], np.float32)  # leaves the box at once; never enters it
    assert_no_hit(cast(rows, away), RC.USED)
    along = np.array([[0.013, 0.1, 0.08, 1, 0, 0]], np.float32)  # parallel to the plane, in front of it: near, no crossing
    assert_no_hit(cast(rows, along, radius=3), RC.USED | RC.NEAR)
    some = np.array([[0.1, 0.1, 0.013, 0, 0, 1]], np.float32)
    assert_no_hit(cast(rows[:0], some), RC.USED)
    assert len(cast(rows, np.zeros((0, 6), np.float32))) == 0
