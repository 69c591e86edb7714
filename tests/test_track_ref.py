"""CPU: the pose-tracking contract (tests/track_ref.py) on models ray-cast from the synthetic scene's analytic surfaces."""
import math

import numpy as np

import hfpf
import track_ref as T

RES = 0.002
Z_CLIP = (0.28, 0.6)


def _pose(R3, t):
    return np.hstack([np.asarray(R3, np.float64), np.asarray(t, np.float64).reshape(3, 1)])


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def _cast(o, d, surfaces):
    """Nearest hit along rays o + s d (d: (n, 3)) of the given surfaces: (s, normal), s = inf where nothing is hit."""
    n = d.shape[0]
    best, nrm = np.full(n, np.inf), np.zeros((n, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        if "plane" in surfaces:  # z - 0.05 x = 0.56
            den = d[:, 2] - 0.05 * d[:, 0]
            s = (0.56 - (o[2] - 0.05 * o[0])) / den
            hit = (s > 0) & (s < best)
            best[hit] = s[hit]
            nrm[hit] = np.array([0.05, 0.0, -1.0]) / math.sqrt(1.0025)
        if "flat" in surfaces:  # z = 0.5, normal exactly (0, 0, -1)
            s = (0.5 - o[2]) / d[:, 2]
            hit = (s > 0) & (s < best)
            best[hit] = s[hit]
            nrm[hit] = (0.0, 0.0, -1.0)
        if "sphere" in surfaces:
            c, r = np.array([0.05, 0.0, 0.45]), 0.10
            oc = o - c
            a = (d * d).sum(1)
            b = 2 * (d @ oc)
            disc = b * b - 4 * a * (oc @ oc - r * r)
            s = (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a)
            hit = (disc > 0) & (s > 0) & (s < best)
            best[hit] = s[hit]
            p = o + s[hit, None] * d[hit]
            nrm[hit] = (p - c) / r
        if "box" in surfaces:
            lo, hi = np.array([-0.20, -0.10, 0.40]), np.array([-0.08, 0.10, 0.60])
            ta, tb = (lo - o) / d, (hi - o) / d
            t0, t1 = np.minimum(ta, tb), np.maximum(ta, tb)
            s, ax = t0.max(1), t0.argmax(1)
            hit = (s <= t1.min(1)) & (s > 0) & (s < best)
            best[hit] = s[hit]
            nn = np.zeros((hit.sum(), 3))
            nn[np.arange(nn.shape[0]), ax[hit]] = -np.sign(d[hit, ax[hit]])
            nrm[hit] = nn
    return best, nrm


def _rays(W, H, K, R3):
    fx, fy, cx, cy = K
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dc = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1).reshape(-1, 3)
    return dc, dc @ np.asarray(R3).T


def model_rows(surfaces, pose, W=480, H=360, f=420.0):
    """Rows sampled from the surfaces seen from `pose`, with exact normals, in the lexicographic voxel order extract uses."""
    dc, dw = _rays(W, H, (f, f, W / 2, H / 2), pose[:, :3])
    s, nrm = _cast(pose[:, 3], dw, surfaces)
    hit = np.isfinite(s)
    p = pose[:, 3] + s[hit, None] * dw[hit]
    r = np.zeros(hit.sum(), dtype=hfpf.ROW_DTYPE)
    ijk = np.floor(p / RES).astype(np.int32)
    for k, (a, b) in enumerate((("ix", "x"), ("iy", "y"), ("iz", "z"))):
        r[a], r[b] = ijk[:, k], p[:, k]
    r["nx"], r["ny"], r["nz"] = nrm[hit].T
    r["count"] = 5
    order = np.lexsort((r["iz"], r["iy"], r["ix"]))
    r = r[order]
    keep = np.ones(len(r), bool)
    keep[1:] = (np.diff(r["ix"]) != 0) | (np.diff(r["iy"]) != 0) | (np.diff(r["iz"]) != 0)  # one row per voxel
    return r[keep]


def frame_points(surfaces, pose, W=160, H=120, f=150.0):
    """A camera-frame cloud (f32) of the surfaces seen from `pose` (half-pixel offset rays: no point coincides with a row)."""
    dc, dw = _rays(W, H, (f, f, W / 2 - 0.5, H / 2 - 0.5), pose[:, :3])
    s, _ = _cast(pose[:, 3], dw, surfaces)
    p = (s[:, None] * dc).astype(np.float32)
    p[~np.isfinite(s)] = np.nan
    return p


VIEW = dict(K=(150.0, 150.0, 80.0, 60.0), width=160, height=120, z_range=(0.05, 3.0), splat_radius=0)
TRUE = _pose(_rot((0.3, 1.0, 0.2), 2.0), (0.004, -0.003, 0.002))


def _errors(pose, ref):
    dR = pose[:, :3] @ ref[:, :3].T
    ang = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1) / 2))))
    return float(np.linalg.norm(pose[:, 3] - ref[:, 3])), ang


def test_recovers_a_centimetre_and_a_degree_on_plane_sphere_and_box():
    surf = ("plane", "sphere", "box")
    rows = model_rows(surf, _pose(np.eye(3), (0.0, 0.0, 0.0)))
    pts = T.cloud_points(frame_points(surf, TRUE))
    guess = _pose(_rot((1.0, -0.5, 0.3), 1.0) @ TRUE[:, :3], TRUE[:, 3] + np.array([0.006, -0.005, 0.006]))
    e0 = _errors(guess, TRUE)
    assert e0[0] > 0.009 and e0[1] > 0.99
    out = T.track(rows, pts, guess, RES, VIEW, Z_CLIP, max_iterations=20, max_distance=0.03, damping=1e-6, eps_rotation=1e-7,
                  eps_translation=1e-7)
    e1 = _errors(out["pose"], TRUE)
    print("start %.4f m / %.3f deg -> %.6f m / %.5f deg in %d iterations, flags %d, %d inliers, rms %.2e" % (
        *e0, *e1, out["iterations"], out["flags"], out["inliers"], out["rms"]))
    assert out["flags"] == T.CONVERGED
    assert e1[0] < 1e-4 and e1[1] < 0.01
    assert out["points_used"] > 5000 and out["inliers"] > 0.8 * out["points_used"]
    R = out["pose"][:, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14


def test_determinism_of_the_reference():
    surf = ("plane", "sphere", "box")
    rows = model_rows(surf, _pose(np.eye(3), (0.0, 0.0, 0.0)), 240, 180, 210.0)
    pts = T.cloud_points(frame_points(surf, TRUE), 2)
    guess = _pose(TRUE[:, :3], TRUE[:, 3] + 0.005)
    a = T.track(rows, pts, guess, RES, VIEW, Z_CLIP, max_iterations=3, max_distance=0.03, damping=1e-6)
    b = T.track(rows, pts, guess, RES, VIEW, Z_CLIP, max_iterations=3, max_distance=0.03, damping=1e-6)
    assert a["pose"].tobytes() == b["pose"].tobytes() and a["information"].tobytes() == b["information"].tobytes()


def test_a_single_plane_is_degenerate_without_damping_and_bounded_with_it():
    rows = model_rows(("flat",), _pose(np.eye(3), (0.0, 0.0, 0.0)))
    true = _pose(np.eye(3), (0.0, 0.0, 0.0))
    pts = T.cloud_points(frame_points(("flat",), true))
    guess = _pose(_rot((1.0, 0.4, 0.7), 1.0), (0.004, -0.003, 0.008))
    out = T.track(rows, pts, guess, RES, VIEW, Z_CLIP, max_iterations=10, max_distance=0.03, damping=0.0)
    assert out["flags"] == T.DEGENERATE and out["iterations"] == 1
    assert out["pose"].tobytes() == guess.tobytes()  # the last good estimate: the guess
    # the information matrix shows why: the rotation about the normal and the in-plane translation carry nothing
    for k in (2, 3, 4):
        assert not out["information"][k].any() and not out["information"][:, k].any()
    out = T.track(rows, pts, guess, RES, VIEW, Z_CLIP, max_iterations=20, max_distance=0.03, damping=1e-3, eps_rotation=1e-9,
                  eps_translation=1e-9)
    assert out["flags"] == T.CONVERGED, out["flags"]
    assert all(xi[2] == 0.0 and xi[3] == 0.0 and xi[4] == 0.0 for xi in out["history"])  # unconstrained twist parts stay exactly 0
    assert np.isfinite(out["pose"]).all()
    # the constrained degrees of freedom reach the truth: the optical axis is again the plane's normal, the plane 0.5 m away
    R, t = out["pose"][:, :3], out["pose"][:, 3]
    assert abs(R[2, 2] - 1.0) < 1e-9 and abs(t[2]) < 1e-6
    # the unconstrained ones stay at the guess (up to the second-order shift of the rotation about the camera centre)
    assert np.abs(t[:2] - guess[:2, 3]).max() < 5e-4
    yaw = math.atan2(R[1, 0] - R[0, 1], R[0, 0] + R[1, 1])
    yaw0 = math.atan2(guess[1, 0] - guess[0, 1], guess[0, 0] + guess[1, 1])
    assert abs(yaw - yaw0) < 1e-3


def test_cayley_rotations_are_orthonormal():
    rng = np.random.default_rng(7)
    for om in np.concatenate([rng.normal(size=(200, 3)) * 0.05, rng.normal(size=(50, 3)) * 2.0, [[0.0, 0.0, 0.0]]]):
        R = np.array(T.cayley([float(v) for v in om]))
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15
        assert abs(np.linalg.det(R) - 1.0) < 1e-15
    # first order: R(omega) = I + [omega]x + O(omega^2)
    R = np.array(T.cayley([1e-4, -2e-4, 3e-4]))
    assert abs(R[2, 1] - 1e-4) < 1e-7 and abs(R[0, 2] + 2e-4) < 1e-7 and abs(R[1, 0] - 3e-4) < 1e-7


def test_points_32_m_from_the_camera_centre_are_rejected():
    def one(dist):
        rows = np.zeros(1, dtype=hfpf.ROW_DTYPE)
        rows["z"], rows["nz"], rows["count"] = dist, -1.0, 1
        view = dict(K=(100.0, 100.0, 4.0, 4.0), width=9, height=9, z_range=(0.05, 100.0), splat_radius=4)
        pts = np.array([[0.0, 0.0, dist + 0.001]] * 8, np.float32)
        return T.track(rows, pts, _pose(np.eye(3), (0.0, 0.0, 0.0)), RES, view, (0.1, 100.0), max_iterations=1, max_distance=0.01,
                       damping=1.0)
    near = one(31.5)
    assert near["points_used"] == 8 and near["inliers"] == 8 and near["flags"] != T.TOO_FEW
    far = one(32.5)
    assert far["points_used"] == 8 and far["inliers"] == 0 and far["flags"] == T.TOO_FEW


def test_sums_are_exact_integers_of_the_quantised_terms():
    J = np.array([[1.0, 0.5, -0.25, 0.0, 0.0, 1.0], [2.0 ** -25, 3 * 2.0 ** -25, 0.0, 0.0, 1.0, 0.0]])
    r = np.array([0.001, -0.002])
    s = T.sums(J, r, 5)
    assert s[0] == (1 << 24) + 0  # 1 + rint(2^-50 * 2^24) = 2^24 + 0
    assert s[28] == 2 and s[29] == 5
    A, b, rr, inl = T.system(s)
    assert inl == 2 and A[0][5] == A[5][0] == 1.0 and b[5] == float(np.rint(0.001 * 2 ** 28)) / 2 ** 28
    assert rr == float(np.rint(1e-6 * 2 ** 32) + np.rint(4e-6 * 2 ** 32)) / 2 ** 32


def test_a_frame_with_too_few_points_is_left_at_the_guess():
    surf = ("plane",)
    rows = model_rows(surf, _pose(np.eye(3), (0.0, 0.0, 0.0)), 120, 90, 105.0)
    pts = T.cloud_points(frame_points(surf, TRUE))[:5]
    out = T.track(rows, pts, TRUE, RES, VIEW, Z_CLIP, max_iterations=4, max_distance=0.03, damping=1e-3)
    assert out["flags"] == T.TOO_FEW and out["iterations"] == 1 and out["pose"].tobytes() == TRUE.tobytes()
