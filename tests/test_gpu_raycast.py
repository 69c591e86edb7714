"""GPU: casting rays against the fused model (hfpf_raycast*).  A raycast is defined on the rows hfpf_extract returns and the cells
hfpf_get_occupied lists, as a dense march of query samples; the kernel skips what it can prove undefined.  Every hit is compared byte
for byte with tests/raycast_ref.py, which evaluates every sample."""
import ctypes as C

import numpy as np
import pytest

import query_ref as Q
import raycast_ref as RC
from gpu_support import HELD_OUT, IDENT, POSE_SEED, SEED, counters, grid, rays_device, run, same_rays, two_handles, unchanged, uploaded
from scenes import DepthScene

pytestmark = pytest.mark.gpu
INF = float("inf")
VIEW_W, VIEW_H = 128, 96   # (96 x 72 gave 95 NEAR-without-HIT rays on the reference at radius 3: enlarged to meet the condition)
VIEW_Z = (0.25, 0.65)
RAY_T = (0.0, 1.3)
# every radius, a count gate, a finite max_distance, steps 0.25 / 0.5 / 1.5, culling on and off
OPTION_SETS = [dict(radius=1, min_count=0.0, max_distance=INF, step=0.5, cull_backfaces=False),
               dict(radius=2, min_count=3.0, max_distance=INF, step=0.25, cull_backfaces=True),
               dict(radius=3, min_count=0.0, max_distance=0.004, step=0.5, cull_backfaces=False),
               dict(radius=4, min_count=0.0, max_distance=0.006, step=1.5, cull_backfaces=True)]
IDS = ["r%d_mc%g_md%g_s%g_c%d" % (o["radius"], o["min_count"], o["max_distance"], o["step"], o["cull_backfaces"]) for o in OPTION_SETS]


def _bbox(g):
    return tuple(g.cfg.bbox)


def _view(synth_mod, W=VIEW_W, H=VIEW_H, f=HELD_OUT):
    """The held-out frame's pose and its intrinsics scaled to W x H."""
    pose = synth_mod.pose(POSE_SEED, f)
    _, _, K = synth_mod.depth_frame(SEED, f, 640, 480, pose)
    s = W / 640.0
    return np.asarray(pose, np.float64).reshape(3, 4), (K[0] * s, K[1] * s, (K[2] + 0.5) * s - 0.5, (K[3] + 0.5) * s - 0.5)


def _frame(n):
    """Two unit vectors orthogonal to each unit vector of n."""
    a = np.where(np.abs(n[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    u = np.cross(n, a)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return u, np.cross(n, u)


def _random_rays(g, rows, res, seed=0xA11):
    """Rays in the fusion frame (identity pose): aimed at rows from their normal's side, from inside and outside the box; along the
    surface a cell or two in front of it (near, no crossing); and past the box altogether."""
    rng = np.random.default_rng(seed)
    live = rows[rows["count"] > 0]
    b = np.asarray(_bbox(g))

    def pick(n):
        r = live[rng.integers(0, len(live), n)]
        return (np.stack([r["x"], r["y"], r["z"]], axis=1).astype(np.float64),
                np.stack([r["nx"], r["ny"], r["nz"]], axis=1).astype(np.float64))

    c, n = pick(1600)
    o = c + (n + rng.normal(0, 0.25, c.shape)) * rng.uniform(0.03, 1.1, (len(c), 1))
    aimed = np.hstack([o, (c - o) * rng.uniform(0.5, 4.0, (len(c), 1))])
    c, n = pick(500)
    u, v = _frame(n)
    a = rng.uniform(0, 2 * np.pi, (len(c), 1))
    tang = np.cos(a) * u + np.sin(a) * v
    o = c + n * rng.uniform(0.5, 2.0, (len(c), 1)) * res - tang * rng.uniform(0.0, 0.05, (len(c), 1))
    along = np.hstack([o, tang + n * rng.uniform(0.0, 0.05, (len(c), 1))])
    centre, span = (b[0::2] + b[1::2]) / 2, b[1::2] - b[0::2]
    d = rng.normal(size=(300, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    away = np.hstack([centre + d * span * rng.uniform(0.9, 1.5, (300, 1)), d + rng.normal(0, 0.2, d.shape)])
    return np.vstack([aimed, along, away]).astype(np.float32)


def _axis_rays(g, rows, res, seed=0xA12):
    """Rays along +-x, +-y, +-z whose origins are lattice points (cell corners) and whose samples therefore fall on cell boundaries:
    through the corner of a row's cell, starting up to 90 cells before it (some outside the box)."""
    rng = np.random.default_rng(seed)
    live = rows[rows["count"] > 0]
    b = np.asarray(_bbox(g))
    out = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            r = live[rng.integers(0, len(live), 400)]
            cell = np.stack([r["ix"], r["iy"], r["iz"]], axis=1).astype(np.float64)
            cell[:, axis] -= sign * rng.integers(5, 90, len(r))
            o = b[0::2] + cell * res
            d = np.zeros_like(o)
            d[:, axis] = sign
            out.append(np.hstack([o, d]))
    return np.vstack(out).astype(np.float32)


def _coverage(label, opt, ref, hit_min, near_min):
    f = ref["flags"].reshape(-1)
    hit = int((f & RC.HIT != 0).sum())
    near_only = int(((f & RC.NEAR != 0) & (f & RC.HIT == 0)).sum())
    print("%s, %s: %d rays, %d used, %d HIT (%d back), %d NEAR without HIT (reference)" % (
        label, opt, f.size, (f & RC.USED != 0).sum(), hit, (f & RC.BACKFACE != 0).sum(), near_only))
    assert hit >= hit_min and near_only >= near_min, "%s, %s: the set does not cover the condition" % (label, opt)


@pytest.fixture(scope="module")
def session(hfpf_mod, synth_mod):
    sc = DepthScene(12, 640, 480, clean_every=4)
    g = grid(hfpf_mod)
    run(g, sc)
    rows = g.extract().copy()
    occ = g.occupied()
    yield sc, g, rows, occ
    g.close()


# ---- 1. byte-identical to the dense march of the numpy contract ---------------------------------------------------------------

@pytest.mark.parametrize("opt", OPTION_SETS, ids=IDS)
def test_byte_identical_to_raycast_ref(hfpf_mod, synth_mod, session, opt):
    sc, g, rows, occ = session
    res = g.dims[1]
    pose, K = _view(synth_mod)
    ref = RC.raycast_view(rows, occ, pose, K, VIEW_W, VIEW_H, _bbox(g), res, t_range=VIEW_Z, **opt)
    _coverage("held-out view %dx%d" % (VIEW_W, VIEW_H), opt, ref, 1000, 100)
    same_rays(g.raycast_view(pose, K, VIEW_W, VIEW_H, t_range=VIEW_Z, **opt), ref, "view, host form, %s" % opt)
    same_rays(g.raycast_views_device([pose], K, VIEW_W, VIEW_H, t_range=VIEW_Z, **opt), ref, "view, device form, %s" % opt)
    # (the axis-aligned set has 2,400 rays, 400 a direction, and meets the same condition)
    for label, rays, hit_min, near_min in (("random rays", _random_rays(g, rows, res), 1000, 100), ("axis rays on cell boundaries", _axis_rays(g, rows, res), 1000, 100)):
        ref = RC.raycast(rows, occ, rays, IDENT, _bbox(g), res, t_range=RAY_T, **opt)
        _coverage(label, opt, ref, hit_min, near_min)
        same_rays(g.raycast(rays, IDENT, t_range=RAY_T, **opt), ref, "%s, host form, %s" % (label, opt))
        same_rays(rays_device(g, rays, IDENT, t_range=RAY_T, **opt), ref, "%s, device form, %s" % (label, opt))


# ---- 2. equivalent forms ------------------------------------------------------------------------------------------------------

def test_equivalent_forms(hfpf_mod, synth_mod, session):
    sc, g, rows, occ = session
    res = g.dims[1]
    pose, K = _view(synth_mod, 160, 120)
    poses = [pose, np.asarray(sc.poses[3], np.float64).reshape(3, 4), np.asarray(sc.poses[7], np.float64).reshape(3, 4)]
    kw = dict(radius=2, step=0.5, t_range=VIEW_Z)
    batch = g.raycast_views_device(poses, K, 160, 120, **kw)
    for v, p in enumerate(poses):
        single = g.raycast_view(p, K, 160, 120, **kw)
        same_rays(batch[v], single, "view %d of a batch against the host form" % v)
        same_rays(g.raycast_views_device([p], K, 160, 120, **kw), single, "view %d alone on the device" % v)
        assert (single["flags"] & RC.HIT != 0).sum() > 1000
    # more than 2^20 rays through the host form (two chunks) against the same rays cast in two halves
    base = _random_rays(g, rows, res, seed=0xB22)
    rays = np.tile(base, ((1 << 20) // len(base) + 2, 1))
    rays[:, :3] += np.random.default_rng(5).normal(0, 1e-3, (len(rays), 3)).astype(np.float32)
    assert len(rays) > (1 << 20)
    kw = dict(radius=2, step=1.0, t_range=RAY_T)
    whole = g.raycast(rays, IDENT, **kw)
    half = len(rays) // 2 + 7
    same_rays(whole, np.concatenate([g.raycast(rays[:half], IDENT, **kw), g.raycast(rays[half:], IDENT, **kw)]), "chunked host call against two halves")
    same_rays(whole, rays_device(g, rays, IDENT, **kw), "chunked host call against one device call")
    assert (whole["flags"] & RC.HIT != 0).sum() > 100000


# ---- 3. a bound that follows from the contract -----------------------------------------------------------------------------------

def test_a_hit_lies_within_max_distance_of_its_row(hfpf_mod, synth_mod, session):
    """Both endpoints of a crossing lie within max_distance of their rows' centroids, |p_{k-1} - p_k| = dt * |D|, and the hit lies
    between the endpoints: |p - centroid(attribute row)| <= max_distance + dt * |D|."""
    sc, g, rows, occ = session
    res = g.dims[1]
    pose, K = _view(synth_mod, 320, 240)
    md, step = 0.004, 0.5
    h = g.raycast_view(pose, K, 320, 240, radius=2, max_distance=md, step=step, t_range=VIEW_Z).reshape(-1)
    O, D, _ = RC.view_rays(pose, K, 320, 240)
    hit = h["flags"] & RC.HIT != 0
    assert hit.sum() > 10000
    keys = Q.keys(rows["ix"], rows["iy"], rows["iz"])
    rv = h["row_voxel"][hit].astype(np.int64)
    j = np.searchsorted(keys, Q.keys(rv[:, 0], rv[:, 1], rv[:, 2]))
    assert (keys[j] == Q.keys(rv[:, 0], rv[:, 1], rv[:, 2])).all()
    c = np.stack([rows["x"][j], rows["y"][j], rows["z"][j]], axis=1).astype(np.float64)
    dist = np.linalg.norm(h["p"][hit].astype(np.float64) - c, axis=1)
    bound = md + step * res * np.linalg.norm(D[hit], axis=1)
    print("hits %d; |p - centroid| max %.6f m against a bound of at least %.6f m" % (hit.sum(), dist.max(), bound.min()))
    assert (dist <= bound + 1e-7).all()   # (1e-7 m: the f32 rounding of p and of the centroid)
    front = hit & (h["flags"] & RC.BACKFACE == 0)
    nd = (h["n"][front].astype(np.float64) * D[front]).sum(axis=1)
    print("front hits %d, of which the attribute normal faces the ray (n.D < 0): %.4f" % (front.sum(), (nd < 0).mean()))
    assert (h["rgb"][hit] == rows["rgb"][j].view(np.uint32)).all() and (h["count"][hit] == rows["count"][j]).all()


# ---- 4. no side effects -------------------------------------------------------------------------------------------------------

def test_a_raycast_changes_nothing(hfpf_mod, synth_mod):
    sc = DepthScene(10, 320, 240, clean_every=3)
    K = sc.K

    def look(g, i):
        g.raycast_view(sc.poses[i % sc.n_frames], K, 80, 60, radius=1 + i % 4, t_range=VIEW_Z, cull_backfaces=bool(i & 1))

    def on_empty(b):  # before the first clean
        h0 = b.raycast_view(sc.poses[0], K, 80, 60, t_range=VIEW_Z)
        assert (h0["flags"] == RC.USED).all()

    with two_handles(hfpf_mod, sc, look, on_empty) as (a, b, rb):
        one = b.raycast_view(sc.poses[2], K, sc.W, sc.H, t_range=VIEW_Z)
        two = b.raycast_view(sc.poses[2], K, sc.W, sc.H, t_range=VIEW_Z)
        same_rays(one, two, "second raycast")
        assert (one["flags"] & RC.HIT != 0).sum() > 10000
        unchanged(a, b, rb)
        depth, rgb, Kf = sc.frames[1]
        for g in (a, b):
            g.integrate_depth(depth, sc.poses[1], Kf, color=rgb)
            g.clean()
        assert a.extract().tobytes() == b.extract().tobytes() and counters(a) == counters(b)
        assert a.occupied().tobytes() == b.occupied().tobytes()


# ---- 5. refusals, empty and cleared handles ---------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_and_the_handle_stays_usable(hfpf_mod, synth_mod):
    H_ = hfpf_mod
    L = H_.lib()
    sc = DepthScene(6, 160, 120, clean_every=3)
    nan, inf = float("nan"), float("inf")
    bad = [("struct_size", 56), ("flags", 2), ("reserved0", 1), ("reserved", 1), ("radius", 0), ("radius", 5), ("min_count", nan), ("max_distance", 0.0),
           ("max_distance", nan), ("step", 0.1), ("step", 4.5), ("step", nan), ("t_min", -0.1), ("t_min", nan), ("t_min", 2.0), ("t_max", inf)]
    with grid(hfpf_mod) as g:
        run(g, sc)
        want = g.extract().copy()
        pose = np.ascontiguousarray(sc.poses[1], np.float64).reshape(12)
        K = sc.K
        good = g.raycast_view(pose, K, 40, 30, t_range=VIEW_Z)
        rays = np.ascontiguousarray(_random_rays(g, want, g.dims[1])[:64])
        hits = np.full(40 * 30, 0xAB, np.uint8).repeat(64).view(H_.RAY_HIT_DTYPE)
        before = hits.tobytes()
        P = lambda x: x.ctypes.data_as(C.c_void_p)
        dev = g.device_alloc(1 << 20)

        def calls(o, which=(0, 1, 2, 3), pose_p=P(pose), hits_p=P(hits), rays_p=P(rays), w=40, h=30, fx=K[0], cx=K[2], dev_hits=dev, dev_rays=dev):
            """The return codes of the selected entry points (host rays, device rays, host view, device views)."""
            ob = C.byref(o) if o is not None else None
            fns = [lambda: L.hfpf_raycast(g._h, ob, rays_p, 64, pose_p, hits_p),
                   lambda: L.hfpf_raycast_device(g._h, ob, C.c_void_p(dev_rays), 64, pose_p, C.c_void_p(dev_hits)),
                   lambda: L.hfpf_raycast_view(g._h, ob, w, h, fx, K[1], cx, K[3], pose_p, hits_p),
                   lambda: L.hfpf_raycast_view_device(g._h, ob, w, h, fx, K[1], cx, K[3], 1, pose_p, C.c_void_p(dev_hits))]
            return [fns[i]() for i in which]

        ok = H_.raycast_opts(t_range=VIEW_Z)
        for field, val in bad:
            o = H_.raycast_opts(t_range=VIEW_Z)
            setattr(o, field, val)
            assert calls(o) == [-2] * 4, (field, val)
        assert calls(None) == [-2] * 4
        assert calls(H_.raycast_opts(step=0.125, t_range=(0.0, 300.0))) == [-2] * 4, "more than 2^20 samples a ray"
        assert calls(ok, pose_p=None) == [-2] * 4
        badpose = pose.copy()
        badpose[5] = nan
        assert calls(ok, pose_p=P(badpose)) == [-2] * 4
        assert calls(ok, hits_p=None, dev_hits=None) == [-2] * 4
        assert calls(ok, (0, 1), rays_p=None, dev_rays=None) == [-2] * 2
        assert calls(ok, (1, 3), dev_hits=dev + 8) == [-2] * 2 and calls(ok, (1,), dev_rays=dev + 2) == [-2]
        for kw in (dict(w=0), dict(h=0), dict(w=1 << 16, h=(1 << 15) + 1), dict(fx=0.0), dict(fx=nan), dict(fx=inf), dict(cx=nan), dict(cx=inf)):
            assert calls(ok, (2, 3), **kw) == [-2] * 2, kw
        assert hits.tobytes() == before, "a refused call wrote its output"
        # n_rays = 0 and n_views = 0 pass after the checks
        assert L.hfpf_raycast(g._h, C.byref(ok), None, 0, P(pose), P(hits)) == 0
        assert L.hfpf_raycast_view_device(g._h, C.byref(ok), 40, 30, K[0], K[1], K[2], K[3], 0, None, C.c_void_p(dev)) == 0
        assert hits.tobytes() == before
        g.device_free(dev)
        assert g.extract().tobytes() == want.tobytes()
        same_rays(g.raycast_view(pose, K, 40, 30, t_range=VIEW_Z), good, "after the refusals")


def test_empty_and_cleared_handles_return_no_hits(hfpf_mod, synth_mod):
    sc = DepthScene(4, 160, 120, clean_every=2)
    rays = np.array([[0, 0, -0.2, 0, 0, 1], [np.nan, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0]], np.float32)
    with grid(hfpf_mod) as g:
        def check():
            h = g.raycast_view(sc.poses[0], sc.K, 32, 24, t_range=VIEW_Z)
            same_rays(h, RC.raycast_view(np.zeros(0, hfpf_mod.ROW_DTYPE), np.zeros((0, 3), np.int32), sc.poses[0], sc.K, 32, 24, _bbox(g), g.dims[1], t_range=VIEW_Z),
                  "empty model")
            assert (h["flags"] == RC.USED).all()
            r = g.raycast(rays, IDENT, t_range=RAY_T)
            assert list(r["flags"]) == [RC.USED, 0, 0] and (r["t"].view(np.uint32) == RC.NAN_BITS).all() and (r["row_voxel"] == -1).all()
        check()
        run(g, sc)
        assert (g.raycast_view(sc.poses[0], sc.K, 32, 24, t_range=VIEW_Z)["flags"] & RC.HIT != 0).any()
        g.clear()
        check()


# ---- 6. full size: large jumps --------------------------------------------------------------------------------------------------

def test_full_size_view_against_the_sparse_oracle(hfpf_mod, synth_mod):
    """A 640x480 view of a 1 mm model.  The oracle is hfpf_query_device: on the samples k-1 and k of every hit (they must be defined,
    differ in sign and give the hit's values), and on every sample of 256 random rays (the whole march, through raycast_ref's rule)."""
    W, H, n_frames = 640, 480, 24
    sc = DepthScene(n_frames, W, H, clean_every=8)
    opt = dict(radius=2, step=0.5, t_range=VIEW_Z)
    with grid(hfpf_mod, resolution=0.001, max_bricks=400000, max_log_points=n_frames * W * H, max_normals=8 << 20) as g:
        run(g, sc)
        res = g.dims[1]
        pose, K = _view(synth_mod, W, H)
        h = g.raycast_view(pose, K, W, H, **opt).reshape(-1)
        O, D, _ = RC.view_rays(pose, K, W, H)
        dt = opt["step"] * res
        n = RC.n_samples(VIEW_Z[0], VIEW_Z[1], opt["step"], res)
        hit = np.flatnonzero(h["flags"] & RC.HIT != 0)
        print("1 mm model: %d of %d rays hit, %d near without a hit, %d samples a ray" % (
            len(hit), len(h), ((h["flags"] & RC.NEAR != 0) & (h["flags"] & RC.HIT == 0)).sum(), n))
        assert len(hit) > 100000

        def samples(ray, k):
            tk = VIEW_Z[0] + k.astype(np.float64) * dt
            return (O[ray] + tk[:, None] * D[ray]).astype(np.float32)

        def query(pts):
            with uploaded(g, pts) as (d,):
                return g.query_device(d, len(pts), IDENT, radius=opt["radius"])

        k = h["sample"][hit].astype(np.int64)
        (qa, ra), (qb, rb) = query(samples(hit, k - 1)), query(samples(hit, k))
        assert ((qa["flags"] & Q.FOUND != 0) & (qb["flags"] & Q.FOUND != 0)).all()
        sa, sb = qa["signed_distance"], qb["signed_distance"]
        assert ((sa < 0) != (sb < 0)).all()
        assert np.array_equal((h["flags"][hit] & RC.BACKFACE) != 0, sa < 0)
        w = sa.astype(np.float64) / (sa.astype(np.float64) - sb.astype(np.float64))
        th = (VIEW_Z[0] + (k - 1).astype(np.float64) * dt) + w * dt
        assert h["t"][hit].tobytes() == th.astype(np.float32).tobytes()
        assert h["p"][hit].tobytes() == (O[hit] + th[:, None] * D[hit]).astype(np.float32).tobytes()
        row = np.where(np.abs(sb) < np.abs(sa), rb, ra)
        assert np.array_equal(h["row_voxel"][hit], np.stack([row["ix"], row["iy"], row["iz"]], axis=1))
        assert h["n"][hit].tobytes() == np.stack([row["nx"], row["ny"], row["nz"]], axis=1).tobytes()
        assert np.array_equal(h["count"][hit], row["count"]) and np.array_equal(h["rgb"][hit], row["rgb"].view(np.uint32))
        # 256 whole rays: every sample queried on the device, then the contract's rule in numpy
        pick = np.random.default_rng(0xF5).choice(len(h), 256, replace=False)
        ks = np.arange(n)
        pts = np.concatenate([samples(np.full(n, r), ks) for r in pick])
        qh, qr = query(pts)
        df = (qh["flags"] & Q.FOUND != 0).reshape(256, n)
        s = qh["signed_distance"].reshape(256, n)
        for i, r in enumerate(pick):
            with np.errstate(invalid="ignore"):
                cross = df[i, :-1] & df[i, 1:] & ((s[i, :-1] < 0) != (s[i, 1:] < 0))
            first = int(np.flatnonzero(cross)[0]) + 1 if cross.any() else 0
            assert int(h["sample"][r]) == first, (r, first, h[r])
            assert bool(h["flags"][r] & RC.HIT) == bool(first)
            upto = first + 1 if first else n
            assert bool(h["flags"][r] & RC.NEAR) == bool(df[i, :upto].any()), (r, h[r])
