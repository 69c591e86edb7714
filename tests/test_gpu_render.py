"""GPU: depth, normal and colour views of the fused model (hfpf_render, hfpf_render_device).  A render is defined on the rows
hfpf_extract returns, so every image here is compared byte for byte with tests/render_ref.py's numpy render of the extracted rows."""
import ctypes as C

import numpy as np
import pytest

import render_ref as R
from gpu_support import BBOX, grid, run, same_planes, two_handles, unchanged
from scenes import DepthScene

pytestmark = pytest.mark.gpu
PLANES = ("depth", "normal", "rgb", "count", "voxel")
Z_RANGE = (0.05, 3.0)


def _pose(R3, t):
    return np.hstack([np.asarray(R3, np.float64), np.asarray(t, np.float64).reshape(3, 1)])


def _perturbed(pose, angle_deg, shift):
    a = np.radians(angle_deg)
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, np.cos(a / 2), -np.sin(a / 2)], [0, np.sin(a / 2), np.cos(a / 2)]])
    return _pose(pose[:, :3] @ rz @ rx, pose[:, 3] + np.asarray(shift))


def _behind(pose, rows):
    """The camera mirrored through the model's centre, turned 180 degrees about its y axis: it sees the back of the surface."""
    c = np.array([np.median(rows[k]) for k in ("x", "y", "z")], np.float64)
    return _pose(pose[:, :3] @ np.diag([-1.0, 1.0, -1.0]), 2 * c - pose[:, 3])


def _empty(img):
    assert (img["depth"].view(np.uint32) == R.NAN_BITS).all() and (img["normal"].view(np.uint32) == R.NAN_BITS).all()
    assert not img["rgb"].any() and not img["count"].any() and (img["voxel"] == -1).all()


@pytest.fixture(scope="module")
def session(hfpf_mod, synth_mod):
    sc = DepthScene(12, 640, 480, clean_every=4)
    g = grid(hfpf_mod)
    run(g, sc)
    rows = g.extract().copy()
    yield sc, g, rows
    g.close()


# ---- 1. bit-exact against the numpy contract -------------------------------------------------------------------------

OPTION_SETS = [  # (splat_radius, cull, min_count, world_normals): every value of every option, several combinations per pose
    (0, False, 1, False), (2, True, 5, True), (-1, True, 1, False), (-1, False, 5, True), (2, False, 1, False), (0, True, 5, False),
]


def test_bit_exact_against_render_ref(hfpf_mod, session):
    sc, g, rows = session
    views = [("integrate pose 0", sc.poses[0]), ("integrate pose 7", sc.poses[7]),
             ("perturbed pose 3", _perturbed(sc.poses[3], 4.0, (0.01, -0.02, 0.015))),
             ("perturbed pose 11", _perturbed(sc.poses[11], -7.0, (-0.03, 0.01, -0.04))),
             ("back of the surface", _behind(sc.poses[5], rows[rows["count"] > 0]))]
    res = g.dims[1]
    n_drawn = {}
    for vi, (label, pose) in enumerate(views):
        for oi, (rad, cull, mc, wn) in enumerate(OPTION_SETS):
            if (vi + oi) % 2:  # half of the combinations per view; every combination on some view
                continue
            kw = dict(z_range=Z_RANGE, min_count=mc, splat_radius=rad, max_splat_radius=4, cull_backfaces=cull, world_normals=wn)
            got = g.render(pose, sc.K, sc.W, sc.H, **kw)
            flags = (R.CULL_BACKFACES if cull else 0) | (R.WORLD_NORMALS if wn else 0)
            ref = R.render(rows, pose, sc.K, sc.W, sc.H, res, Z_RANGE, mc, rad, 4, flags)
            same_planes(got, ref, "%s, options %r" % (label, OPTION_SETS[oi]))
            drawn = ~np.isnan(got["depth"])
            assert (got["count"][drawn] >= max(1, mc)).all()
            n_drawn.setdefault(label, []).append(int(drawn.sum()))
    print("pixels drawn per view and option set:", n_drawn)
    assert all(max(n) > 1000 for n in n_drawn.values()), n_drawn  # every view sees a good part of the model
    # a grazing view: the camera plane passes 1e-8 m in front of two rows, one on the optical axis (drawn, its auto radius capped),
    # the other far to the side at the same depth: it passes the z test and its u leaves +-2^30
    pose, K, z_range = _grazing(R.drawn_rows(rows, 1), sc.K)
    W, H = 64, 48
    ok, zc, _, _ = R.project(R.drawn_rows(rows, 1), pose, K, z_range)
    assert ((z_range[0] < zc) & (zc < z_range[1]) & ~ok).any(), "no drawn row passes the z test and fails the 2^30 test"
    ref = R.render(rows, pose, K, W, H, res, z_range, 1, -1, 4, 0)
    assert (~np.isnan(ref["depth"])).any(), "the grazing view draws no row"
    same_planes(g.render(pose, K, W, H, z_range=z_range, min_count=1, splat_radius=-1, max_splat_radius=4), ref, "grazing view")


def _grazing(drawn, K):
    """(pose, K, z_range): row 0 of `drawn` on the optical axis and the row farthest from it on the camera's x axis, both 1e-8 m in
    front of the camera plane; z_near = 1e-9."""
    p = np.stack([drawn[k].astype(np.float64) for k in ("x", "y", "z")], axis=-1)
    d = p - p[0]
    x = d[np.argmax((d * d).sum(axis=1))]
    x /= np.linalg.norm(x)
    z = np.eye(3)[np.argmin(np.abs(x))]  # the world axis farthest from x, made orthogonal to it
    z = z - (z @ x) * x
    z /= np.linalg.norm(z)
    return _pose(np.stack([x, np.cross(z, x), z], axis=-1), p[0] - 1e-8 * z), (K[0], K[1], 32.0, 24.0), (1e-9, 3.0)


def test_count_zero_rows_are_never_drawn(hfpf_mod, session):
    """count == 0 rows sit at the origin (the zero centroid): a camera looking at the origin must not draw them."""
    sc, g, rows = session
    assert (rows["count"] == 0).any(), "the session should hold count == 0 rows"
    pose = _pose(np.eye(3), (0.0, 0.0, -0.5))
    for mc in (0, 1):
        got = g.render(pose, sc.K, sc.W, sc.H, z_range=Z_RANGE, min_count=mc, splat_radius=1)
        assert (got["count"][~np.isnan(got["depth"])] > 0).all()
        same_planes(got, R.render(rows, pose, sc.K, sc.W, sc.H, g.dims[1], Z_RANGE, mc, 1), "origin view")


# ---- 2. batches ---------------------------------------------------------------------------------------------------

def _device_batch(g, poses, K, W, H, planes, **kw):
    n, WH = len(poses), W * H
    shapes = {"depth": (np.float32, 1), "normal": (np.float32, 3), "rgb": (np.uint32, 1), "count": (np.uint32, 1), "voxel": (np.int32, 3)}
    ptrs = {p: g.device_alloc(n * WH * 4 * shapes[p][1]) for p in planes}
    try:
        g.render_device(poses, K, W, H, ptrs, **kw)
        out = {}
        for p in planes:
            dt, ch = shapes[p]
            a = g.device_download(ptrs[p], n * WH * 4 * ch, dtype=dt)
            out[p] = a.reshape((n, H, W, ch) if ch > 1 else (n, H, W))
        return out
    finally:
        for ptr in ptrs.values():
            g.device_free(ptr)


def _batch_poses(sc, n):
    return [_perturbed(sc.poses[i % sc.n_frames], 0.37 * i - 5.0, (0.002 * (i % 7), -0.001 * (i % 5), 0.003 * (i % 3))) for i in range(n)]


def test_device_batch_equals_single_views(hfpf_mod, session):
    sc, g, rows = session
    # 70 views of 64 x 48: the 64-view chunk limit splits them in two launches
    W, H = 64, 48
    K = (sc.K[0] / 10, sc.K[1] / 10, sc.K[2] / 10, sc.K[3] / 10)
    poses = _batch_poses(sc, 70)
    kw = dict(z_range=Z_RANGE, splat_radius=-1, max_splat_radius=3, cull_backfaces=True)
    got = _device_batch(g, poses, K, W, H, PLANES, **kw)
    for v, pose in enumerate(poses):
        one = g.render(pose, K, W, H, **kw)
        same_planes({p: got[p][v] for p in PLANES}, one, "view %d of 70" % v)
    assert (~np.isnan(got["depth"])).sum() > 70 * 100
    # 17 views of 2048 x 1024: 16 views fill the 256 MB z-buffer chunk, the 17th is a second chunk
    W, H = 2048, 1024
    K = (sc.K[0] * 3.2, sc.K[1] * 3.2, sc.K[2] * 3.2, sc.K[3] * 3.2)
    poses = _batch_poses(sc, 17)
    kw = dict(z_range=Z_RANGE, splat_radius=1, min_count=2)
    got = _device_batch(g, poses, K, W, H, ("depth", "rgb"), **kw)
    for v in (0, 15, 16):
        one = g.render(poses[v], K, W, H, planes=("depth", "rgb"), **kw)
        same_planes({p: got[p][v] for p in ("depth", "rgb")}, one, "view %d of 17 at 2048x1024" % v)
    ref = R.render(rows, poses[16], K, W, H, g.dims[1], Z_RANGE, 2, 1)
    same_planes({p: got[p][16] for p in ("depth", "rgb")}, {p: ref[p] for p in ("depth", "rgb")}, "view 16 against render_ref")


# ---- 3. no side effects ---------------------------------------------------------------------------------------------

def test_renders_change_nothing(hfpf_mod, synth_mod):
    sc = DepthScene(10, 320, 240, clean_every=3)
    K = sc.K

    def look(g, i):
        if i % 2 == 0:
            g.render(sc.poses[i % sc.n_frames], K, sc.W, sc.H, z_range=Z_RANGE, splat_radius=-1, min_count=2)
        else:
            ptr = g.device_alloc(2 * sc.W * sc.H * 4)
            g.render_device(np.stack([sc.poses[0], sc.poses[1]]), K, sc.W, sc.H, {"count": ptr}, z_range=Z_RANGE)
            g.device_free(ptr)

    with two_handles(hfpf_mod, sc, look, lambda b: b.render(sc.poses[0], K, sc.W, sc.H)) as (a, b, rb):
        one = b.render(sc.poses[2], K, sc.W, sc.H, z_range=Z_RANGE, splat_radius=2)
        two = b.render(sc.poses[2], K, sc.W, sc.H, z_range=Z_RANGE, splat_radius=2)
        same_planes(one, two, "second render")
        same_planes(one, R.render(rb, sc.poses[2], K, sc.W, sc.H, b.dims[1], Z_RANGE, 0, 2), "render_ref")
        unchanged(a, b, rb)


# ---- 4. edges -------------------------------------------------------------------------------------------------------

def test_empty_and_cleared_handles_render_nothing(hfpf_mod, synth_mod):
    sc = DepthScene(3, 160, 120, clean_every=0)
    with grid(hfpf_mod) as g:
        _empty(g.render(sc.poses[0], sc.K, sc.W, sc.H, splat_radius=2))
        run(g, sc)
        img = g.render(sc.poses[0], sc.K, sc.W, sc.H, z_range=Z_RANGE)
        assert (~np.isnan(img["depth"])).sum() > 100
        g.clear()
        _empty(g.render(sc.poses[0], sc.K, sc.W, sc.H, z_range=Z_RANGE))
        # an integrated but never cleaned session has no rows either (extract returns none)
        sc.integrate(g, 1)
        assert len(g.extract()) == 0
        _empty(g.render(sc.poses[0], sc.K, sc.W, sc.H, z_range=Z_RANGE))


def test_bad_arguments_are_refused_and_the_handle_stays_usable(hfpf_mod, synth_mod):
    H_ = hfpf_mod
    sc = DepthScene(6, 160, 120, clean_every=3)
    with grid(hfpf_mod) as ref:
        run(ref, sc)
        want = ref.extract().copy()
    L = H_.lib()
    bad = {
        "struct_size": ("struct_size", C.sizeof(H_.RenderOpts) - 8), "flags": ("flags", 4), "reserved": ("reserved", 1),
        "width 0": ("width", 0), "height 0": ("height", 0), "too many pixels": ("width", 65536),
        "fx 0": ("fx", 0.0), "fx inf": ("fx", float("inf")), "fy negative": ("fy", -1.0), "fy nan": ("fy", float("nan")),
        "cx nan": ("cx", float("nan")), "cy inf": ("cy", float("inf")), "z_near 0": ("z_near", 0.0),
        "z_near >= z_far": ("z_near", 5.0), "z_far inf": ("z_far", float("inf")), "min_count nan": ("min_count", float("nan")),
        "radius -2": ("splat_radius", -2), "radius 16": ("splat_radius", 16), "max radius -1": ("max_splat_radius", -1),
        "max radius 16": ("max_splat_radius", 16),
    }
    with grid(hfpf_mod) as g:
        for i, ev in enumerate(sc.schedule()):
            if ev[0] == "integrate":
                sc.integrate(g, ev[1])
            else:
                g.clean()
            if i != 2:
                continue
            pose = np.ascontiguousarray(sc.poses[0], np.float64).reshape(12)
            depth = np.zeros((sc.H * 2, sc.W), np.float32)  # room for the 65536 x 32769 case's first bytes: never written
            for what, (field, val) in bad.items():
                o = H_.render_opts(sc.K, sc.W, sc.H, z_range=(0.1, 2.0))
                setattr(o, field, val)
                if what == "too many pixels":
                    o.height = 32769
                pl = H_.RenderPlanes(depth=depth.ctypes.data)
                assert L.hfpf_render(g._h, C.byref(o), pose.ctypes.data, C.byref(pl)) == -2, what
                assert L.hfpf_render_device(g._h, C.byref(o), 1, pose.ctypes.data, C.byref(pl)) == -2, what
            assert not depth.any(), "a refused call wrote its plane"
            o = H_.render_opts(sc.K, sc.W, sc.H, z_range=(0.1, 2.0))
            pl = H_.RenderPlanes(depth=depth.ctypes.data)
            assert L.hfpf_render(g._h, C.byref(o), None, C.byref(pl)) == -2, "NULL pose"
            assert L.hfpf_render_device(g._h, C.byref(o), 1, None, C.byref(pl)) == -2, "NULL poses"
            assert L.hfpf_render(g._h, C.byref(o), pose.ctypes.data, C.byref(H_.RenderPlanes())) == -2, "no planes"
            assert L.hfpf_render_device(g._h, C.byref(o), 1, pose.ctypes.data, C.byref(H_.RenderPlanes())) == -2, "no planes"
            assert L.hfpf_render(g._h, None, pose.ctypes.data, C.byref(pl)) == -2, "NULL opts"
            assert L.hfpf_render_device(g._h, C.byref(o), 0, None, C.byref(pl)) == 0, "n_views = 0 is a no-op"
            with pytest.raises(ValueError):
                g.render(pose, sc.K, sc.W, sc.H, planes=("depth", "colour"))
        got = g.extract()
        assert got.tobytes() == want.tobytes()


# ---- 5. round trip: the model seen from an integrate pose resembles the frame taken there -----------------------------

# The first MI355X run measured coverage 0.948 (pose 0) and 0.972 (pose 5) with a median |dz| of 0.47 mm.  0.9 leaves room for a
# change of scene or schedule and still fails a render whose projection or splat footprint is off by a pixel, or whose pose
# convention is wrong (coverage then drops far below it).
MIN_COVERAGE = 0.9


def test_round_trip_from_an_integrate_pose(hfpf_mod, synth_mod):
    sc = DepthScene(8, 640, 480, clean_every=4)
    with grid(hfpf_mod) as g:
        run(g, sc)
        for f in (0, 5):
            depth, _, K = sc.frames[f]
            img = g.render(sc.poses[f], K, sc.W, sc.H, planes=("depth",), z_range=(0.1, 2.0), splat_radius=-1, max_splat_radius=4)
            z_in = depth.astype(np.float64) * np.float64(np.float32(0.001))
            valid = depth != 0
            both = valid & ~np.isnan(img["depth"])
            coverage = both.sum() / valid.sum()
            dz = np.median(np.abs(img["depth"][both].astype(np.float64) - z_in[both]))
            print("round trip, pose %d: coverage %.3f, median |dz| %.5f m" % (f, coverage, dz))
            assert dz < g.dims[1], "median |dz| %.5f m is not below one voxel" % dz
            assert coverage > MIN_COVERAGE, "coverage %.3f" % coverage


# ---- 6. a full-size model ---------------------------------------------------------------------------------------------

@pytest.mark.slow
def test_two_million_rows_against_render_ref(hfpf_mod, synth_mod):
    sc = DepthScene(120, 640, 480, clean_every=30)
    with hfpf_mod.OccupancyGrid(resolution=0.001, bbox=BBOX, fuse_color=True, max_bricks=400000, max_log_points=120 * 640 * 480,
                                max_normals=24 << 20, max_frames=4096, frame_width=640) as g:
        run(g, sc)
        rows = g.extract()
        assert len(rows) > 1_000_000, len(rows)
        for pose, kw in ((sc.poses[17], dict(splat_radius=-1, max_splat_radius=3, cull_backfaces=True)),
                         (_perturbed(sc.poses[90], 3.0, (0.02, 0.0, -0.01)), dict(splat_radius=1, min_count=3, world_normals=True))):
            got = g.render(pose, sc.K, sc.W, sc.H, z_range=Z_RANGE, **kw)
            flags = (R.CULL_BACKFACES if kw.get("cull_backfaces") else 0) | (R.WORLD_NORMALS if kw.get("world_normals") else 0)
            ref = R.render(rows, pose, sc.K, sc.W, sc.H, g.dims[1], Z_RANGE, kw.get("min_count", 0), kw["splat_radius"],
                           kw.get("max_splat_radius", 4), flags)
            same_planes(got, ref, "2M-row model, %r" % kw)
