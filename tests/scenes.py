"""Shared scene / schedule helpers for the parity tests (imported by tests only)."""
import numpy as np

import hfpf_synth as S

BBOX_1M = (-0.5, 0.5, -0.5, 0.5, 0.0, 1.0)


class Scene:
    """A seeded synthetic stream: frames (camera-frame XYZRGB records) + poses + a clean schedule."""

    def __init__(self, n_frames, W, H, resolution, bbox=BBOX_1M, fx=0.0, seed=0xF051, pose_seed=0x5E3, clean_every=0,
                 identity=False, layout=None, max_angle=30.0, jitter=0.05, noise=0.0005, nan_permille=20):
        self.n_frames, self.W, self.H = n_frames, W, H
        self.resolution, self.bbox, self.fx = resolution, bbox, fx
        self.seed, self.pose_seed = seed, pose_seed
        self.clean_every = clean_every
        self.layout = layout or S.LAYOUT_PACKED16
        self.poses = [S.identity_pose() if identity else S.pose(pose_seed, f, max_angle, jitter) for f in range(n_frames)]
        self.noise, self.nan_permille = noise, nan_permille

    def frame(self, f):
        return S.frame(self.seed, f, self.W, self.H, self.poses[f], noise_sigma=self.noise, nan_permille=self.nan_permille,
                       fx=self.fx, layout=self.layout)

    def schedule(self):
        """Yields ('integrate', f) / ('clean',) events; always ends with a clean (explicit schedule)."""
        for f in range(self.n_frames):
            yield ("integrate", f)
            if self.clean_every and (f + 1) % self.clean_every == 0 and f + 1 < self.n_frames:
                yield ("clean",)
        yield ("clean",)


class DepthScene:
    """A seeded stream of synthetic depth frames (uint16 + RGB8) with random poses and a clean schedule."""

    def __init__(self, n_frames, W, H, clean_every=4, depth_scale=0.001, seed=0xD3F7, pose_seed=0x5E3):
        self.n_frames, self.W, self.H, self.clean_every, self.depth_scale = n_frames, W, H, clean_every, depth_scale
        self.poses = [S.pose(pose_seed, f) for f in range(n_frames)]
        self.frames = [S.depth_frame(seed, f, W, H, self.poses[f], depth_scale=depth_scale) for f in range(n_frames)]
        self.K = self.frames[0][2]

    def schedule(self):
        return Scene.schedule(self)

    def cloud(self, f):
        """Frame f as the packed cloud tests/depth_ref.py makes of it."""
        import depth_ref
        depth, rgb, K = self.frames[f]
        return depth_ref.packed_cloud(depth, K, rgb, depth_ref.COLOR_RGB8, self.depth_scale)

    def integrate(self, g, f):
        depth, rgb, K = self.frames[f]
        g.integrate_depth(depth, self.poses[f], K, color=rgb, depth_scale=self.depth_scale)


def run(grid, scene, capture_name, color=False):
    """Drive an oracle grid (capture) or an engine grid (integrate) through the scene's schedule.  color=True also hands
    the oracle the rgb field (its colour extension, fuse_color=True)."""
    lay = scene.layout
    for ev in scene.schedule():
        if ev[0] == "integrate":
            buf = scene.frame(ev[1])
            kw = dict(point_step=lay["point_step"], off_x=lay["off_x"], off_y=lay["off_y"], off_z=lay["off_z"])
            if capture_name == "integrate" or color:
                kw["off_rgb"] = lay["off_rgb"]
            getattr(grid, capture_name)(buf, scene.poses[ev[1]], **kw)
        else:
            grid.clean()
    return grid.extract()


XYZ_TOL = 1e-5  # north_star: fused XYZ within 1e-5


def error_report(ref, got):
    """Largest deviations of the float columns (engine vs oracle), for the tolerance ledger in DESIGN.md: absolute, and
    relative where the reference value is well above its own rounding noise."""
    out = {"rows": int(len(ref))}
    floors = {"x": 1e-3, "y": 1e-3, "z": 1e-3, "mean_dist": 1e-6, "sdx": 1e-9, "sdy": 1e-9, "sdz": 1e-9, "sd_dist": 1e-10}
    for f, floor in floors.items():
        a, b = ref[f].astype(np.float64), got[f].astype(np.float64)
        d = np.abs(a - b)
        out[f + "_abs"] = float(d.max(initial=0.0))
        big = np.abs(a) > floor
        out[f + "_rel"] = float((d[big] / np.abs(a[big])).max(initial=0.0))
    return out


def compare_rows(ref, got, normals_exact=True):
    """ref = oracle rows, got = engine rows.  Integer work bit-exact; XYZ within 1e-5 (north_star)."""
    assert len(ref) == len(got), "row count %d != %d" % (len(ref), len(got))
    for f in ("ix", "iy", "iz"):
        assert np.array_equal(ref[f], got[f]), "voxel index column %s differs" % f
    assert np.array_equal(ref["count"], got["count"]), "points-in-cylinder counts differ at %d rows" % int(
        np.sum(ref["count"] != got["count"]))
    # 0 everywhere as in the reference, or (colour extension on both sides) the members' mean colour, rounded half up: integer work
    assert np.array_equal(ref["rgb"], got["rgb"]), "rgb differs at %d rows" % int(np.sum(ref["rgb"] != got["rgb"]))
    for f in ("nx", "ny", "nz"):
        if normals_exact:
            assert np.array_equal(ref[f].view(np.uint32), got[f].view(np.uint32)), "normal %s not bit-identical" % f
        else:
            assert np.allclose(ref[f], got[f], atol=1e-5, rtol=0)
    for f in ("x", "y", "z"):
        d = np.abs(ref[f].astype(np.float64) - got[f].astype(np.float64))
        assert d.max(initial=0.0) <= XYZ_TOL, "fused %s differs by %.3g" % (f, d.max())
    # meta.csv columns (the reference prints them with 6 significant digits).  Measured over every comparison of the GPU suite
    # (63 scenes, up to 1.8 M rows): mean_dist within 4.7e-6 relative; sd_dist within 6e-4 relative;
    # sdx/sdy/sdz within 1.6e-10 m^2 absolute.  The per-axis variances differ by the quantisation of the reference's f32
    # projections (ulp 6e-8 m on coordinates near 1 m against deviations of ~3e-4 m), which the engine's exact moments of the
    # projection parameter do not contain: an absolute error, ~1e-3 of a variance along the normal (1e-7 m^2).
    assert np.allclose(ref["mean_dist"], got["mean_dist"], rtol=2e-5, atol=1e-10), "mean_dist"
    assert np.allclose(ref["sd_dist"], got["sd_dist"], rtol=1e-3, atol=1e-12), "sd_dist max abs diff %.3g" % (
        np.abs(ref["sd_dist"].astype(np.float64) - got["sd_dist"]).max(initial=0.0))
    for f in ("sdx", "sdy", "sdz"):
        assert np.allclose(ref[f], got[f], rtol=1e-3, atol=2e-10), "%s max abs diff %.3g" % (
            f, np.abs(ref[f].astype(np.float64) - got[f]).max(initial=0.0))
    import os
    if os.environ.get("HFPF_ERR_REPORT"):
        with open(os.environ["HFPF_ERR_REPORT"], "a") as fh:
            import json
            fh.write(json.dumps(error_report(ref, got)) + "\n")


# ---- exact comparison: the engine's own arithmetic, pinned (csrc/stats.hpp; the oracle's exact_moments side channel) ----

EXACT_COLUMNS = ("ix", "iy", "iz", "count", "nx", "ny", "nz", "rgb", "x", "y", "z", "sdx", "sdy", "sdz")


def dense_scene():
    """(scene, config) with thousands of members per voxel: 2 cm voxels and 1 cm cylinders under a zoomed, nearly still camera.  The
    oracle alone shows a largest count above 10,000 (statistic words beyond 2^39), rows with a negative sum of u and rows without
    members."""
    sc = Scene(12, 160, 120, 0.02, fx=615.0, clean_every=1, max_angle=5.0, jitter=0.01)
    return sc, dict(cylinder_radius=0.01, ball_radius=0.06)


def dist_bounds(ref_exact, cylinder_radius=0.001):
    """Per-row bounds (f64 arrays) on |mean_dist - ref| and |sd_dist - ref| of compare_rows_exact; derivation there."""
    import stats_ref
    eps = 2.0 ** -23
    slack = 1.0 + 2.0 ** -20
    r = float(cylinder_radius)
    fd, fdd = float(stats_ref.scale_for(r)), float(stats_ref.scale_for(r * r))
    M = ref_exact["mean_dist"].astype(np.float64)
    V = ref_exact["sd_dist"].astype(np.float64)
    kappa = 3.0 * eps * (1.0 + eps) ** 2
    D = eps * M + (1.0 + eps / 2.0) / fd
    E2 = V + M * M
    t_md = (2.0 * eps * M + 1.0 / fd) * slack
    t_sd = (kappa * E2 + 1.0 / fdd + D * (2.0 * M + D) + eps * V) * slack
    return t_md, t_sd


def compare_rows_exact(ref_exact, got, cylinder_radius=0.001):
    """ref_exact = OracleGrid.extract_exact() (exact_moments=True), got = engine rows of the same cells in the same order.

    Fourteen columns -- ix iy iz count nx ny nz rgb x y z sdx sdy sdz -- must be byte-identical: they are integer work, or the
    f64 expression of record_row over integer sums of f32 quantities that a CPU reproduces bit for bit (the projection parameter
    s, its fixed-point contributions, the voxel's f32 line).

    mean_dist and sd_dist are bounded instead, from ONE fact: a default build (HFPF_EXACT_SQRT=0) takes a member's distance d'
    from the hardware square root, which is within one f32 ulp of the correctly rounded d the oracle has; with eps = 2^-23,
    |d' - d| <= ulp(d) <= eps d.  Everything else is the same arithmetic on both sides.  Per voxel with n members, scales fd,
    fdd (powers of two, so scaling is exact), M = the exact side's mean_dist, V = its sd_dist, E2 = its mean of d^2 (E2 <= V + M^2
    because V = max(E2 - M^2, 0)):

      word 3   |rint(d' fd) - rint(d fd)| <= eps d fd + 1 per member (rint moves a difference by less than one step), and
               sum d fd <= word3 + n/2.  Divided by fd n:     |md' - md| <= D = eps M + (1 + eps/2) / fd          (in f64)
      narrowing to f32 adds half an ulp of each side:          |mean_dist' - mean_dist| <= 2 eps M + 1 / fd
      word 4   d'^2 = d^2 (1 + eta)^2, |eta| <= eps, and each side rounds its square to f32 (2^-24 relative):
               |fl(d'^2) - fl(d^2)| <= (3 eps + 2 eps^2 + eps^3/2) d^2 <= kappa fl(d^2), kappa = 3 eps (1 + eps)^2;
               with the rint step and the sum as above:        |E2' - E2| <= kappa E2 + (1 + kappa/2) / fdd
      variance vd = E2 - md^2, |md'^2 - md^2| <= D (2 M + D); the cnt == 1 zeroing and fmax(., 0) move nothing apart; narrowing
               adds eps V:                                     |sd_dist' - sd_dist| <= kappa E2 + 1 / fdd + D (2 M + D) + eps V

    Both bounds carry a factor 1 + 2^-20 for what was dropped: M, V known only as f32 (2^-24 relative), the eps/2 and kappa/2
    shares of a fixed-point step, and the f64 roundings of the row expression (2^-52 relative).  At the default radius
    (fd = 2^36, fdd = 2^46, M ~ 5e-4, V ~ 5e-8) they are ~1.3e-10 m (3e-7 relative, against 2e-5 in compare_rows) and
    ~3e-13 m^2 (5e-6 relative, against 1e-3).  Rows with count 0 or 1 must have the exact side's bytes (all zero / zero
    variance).  Returns the observed figures; prints them before it asserts."""
    assert len(ref_exact) == len(got), "row count %d != %d" % (len(ref_exact), len(got))
    rep = {"rows": int(len(got)), "max_count": int(ref_exact["count"].max(initial=0))}
    diff_bytes = {}
    for f in EXACT_COLUMNS:
        a = np.ascontiguousarray(ref_exact[f]).view(np.uint8)
        b = np.ascontiguousarray(got[f]).view(np.uint8)
        diff_bytes[f] = int(np.count_nonzero(a != b))
    rep["exact_bytes_differing"] = sum(diff_bytes.values())
    t_md, t_sd = dist_bounds(ref_exact, cylinder_radius)
    d_md = np.abs(ref_exact["mean_dist"].astype(np.float64) - got["mean_dist"].astype(np.float64))
    d_sd = np.abs(ref_exact["sd_dist"].astype(np.float64) - got["sd_dist"].astype(np.float64))
    rep["mean_dist_abs"] = float(d_md.max(initial=0.0))
    rep["mean_dist_of_bound"] = float((d_md / t_md).max(initial=0.0))
    rep["sd_dist_abs"] = float(d_sd.max(initial=0.0))
    rep["sd_dist_of_bound"] = float((d_sd / t_sd).max(initial=0.0))
    big_m, big_v = ref_exact["mean_dist"] > 1e-6, ref_exact["sd_dist"] > 1e-10
    rep["mean_dist_rel"] = float((d_md[big_m] / ref_exact["mean_dist"][big_m]).max(initial=0.0))
    rep["sd_dist_rel"] = float((d_sd[big_v] / ref_exact["sd_dist"][big_v]).max(initial=0.0))
    print("compare_rows_exact: %r" % rep)
    import os
    if os.environ.get("HFPF_EXACT_REPORT"):
        import json
        with open(os.environ["HFPF_EXACT_REPORT"], "a") as fh:
            fh.write(json.dumps(rep) + "\n")
    bad = {f: n for f, n in diff_bytes.items() if n}
    assert not bad, "columns not byte-identical with the exact rows (differing bytes per column): %r" % bad
    none, one = ref_exact["count"] == 0, ref_exact["count"] <= 1
    assert np.array_equal(ref_exact["mean_dist"][none].view(np.uint32), got["mean_dist"][none].view(np.uint32)), "mean_dist of rows without members"
    assert np.array_equal(ref_exact["sd_dist"][one].view(np.uint32), got["sd_dist"][one].view(np.uint32)), "sd_dist of rows with count <= 1"
    assert (d_md <= t_md).all(), "mean_dist off by %.3g, %.3g of the derived bound" % (rep["mean_dist_abs"], rep["mean_dist_of_bound"])
    assert (d_sd <= t_sd).all(), "sd_dist off by %.3g, %.3g of the derived bound" % (rep["sd_dist_abs"], rep["sd_dist_of_bound"])
    return rep
