"""The pose-tracking contract of include/hfpf.h restated in numpy (imported by tests only): extracted rows + a frame + a pose guess
-> the refined pose, flags, inliers, rms and information hfpf_track* return.  The model view is render_ref.zbuffer at the input
pose; per-point arithmetic is f64 arrays in the stated order, the 30 sums are exact int64, and the host solve runs on Python
floats (IEEE f64, one rounding per operation, nothing contracted), in the order the header states."""
import math

import numpy as np

import depth_ref
import render_ref

CONVERGED, DEGENERATE, TOO_FEW = 1, 2, 4
SCALE_JJ, SCALE_JR, SCALE_RR = 2.0 ** 24, 2.0 ** 28, 2.0 ** 32  # fixed-point scales of the J_i J_j, J_i r and r r terms
HEADROOM = 32.0        # |a| component at or beyond which a point is rejected (metres)
N_TERMS = 30           # 21 J_i J_j (i <= j), 6 J_i r, r r, inliers, points_used
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]


def depth_points(depth, K, stride=1, depth_scale=0.001):
    """The sampled points of a depth image: pixels with u % stride == 0 and v % stride == 0, back-projected as depth_ref does."""
    H, W = depth.shape
    xyz = depth_ref.backproject(depth, K, depth_scale).reshape(H, W, 3)
    return np.ascontiguousarray(xyz[::stride, ::stride].reshape(-1, 3))


def cloud_points(xyz, stride=1):
    """The sampled points of a cloud ((N, 3) f32): point i iff i % stride == 0."""
    return np.ascontiguousarray(np.asarray(xyz, np.float32)[::stride])


def used(points, z_clip):
    """Finite x, y, z and z_clip_min < z < z_clip_max (the f32 z widened to double, as integrate compares)."""
    p = np.asarray(points, np.float32)
    z = p[:, 2].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(p).all(axis=1) & (z > float(z_clip[0])) & (z < float(z_clip[1]))


def transform(T, p):
    """pw = T p in f64, rows summed left to right, not rounded."""
    T = np.asarray(T, np.float64).reshape(12)
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    return (((T[0] * x + T[1] * y) + T[2] * z) + T[3], ((T[4] * x + T[5] * y) + T[6] * z) + T[7],
            ((T[8] * x + T[9] * y) + T[10] * z) + T[11])


def associate(pw, V, zb, width, height, K, z_range):
    """(mask, row index) of each world point projected into the model view at V with the splat's arithmetic."""
    V = np.asarray(V, np.float64).reshape(12)
    fx, fy, cx, cy = (float(k) for k in K)
    dx, dy, dz = pw[0] - V[3], pw[1] - V[7], pw[2] - V[11]
    xc = (V[0] * dx + V[4] * dy) + V[8] * dz
    yc = (V[1] * dx + V[5] * dy) + V[9] * dz
    zc = (V[2] * dx + V[6] * dy) + V[10] * dz
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = (float(z_range[0]) < zc) & (zc < float(z_range[1]))
        u = (xc / zc) * fx + cx
        v = (yc / zc) * fy + cy
        ok &= (np.abs(u) < 2.0 ** 30) & (np.abs(v) < 2.0 ** 30)
        pu = np.where(ok, np.floor(u + 0.5), -1.0).astype(np.int64)
        pv = np.where(ok, np.floor(v + 0.5), -1.0).astype(np.int64)
    ok &= (pu >= 0) & (pu < width) & (pv >= 0) & (pv < height)
    word = np.full(pu.shape, render_ref.EMPTY, np.uint64)
    word[ok] = zb[pv[ok] * width + pu[ok]]
    ok &= word != render_ref.EMPTY
    return ok, (word & np.uint64(0xFFFFFFFF)).astype(np.int64)


def terms(points, T, V, zb, drawn, width, height, K, z_range, max_distance):
    """Per point: (inlier mask, J (n, 6), r) at estimate T, for points that are already `used`."""
    pw = transform(T, points)
    ok, row = associate(pw, V, zb, width, height, K, z_range)
    j = np.where(ok, row, 0)
    r_ = drawn[j] if len(drawn) else np.zeros(len(j), drawn.dtype)
    qx, qy, qz = (r_[k].astype(np.float64) for k in ("x", "y", "z"))
    nx, ny, nz = (r_[k].astype(np.float64) for k in ("nx", "ny", "nz"))
    V = np.asarray(V, np.float64).reshape(12)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = pw[0] - qx, pw[1] - qy, pw[2] - qz
        md = float(max_distance)
        ok &= ((dx * dx + dy * dy) + dz * dz) <= md * md
        ok &= ((nx * nx + ny * ny) + nz * nz) <= 2.0
        r = (nx * dx + ny * dy) + nz * dz
        ax, ay, az = pw[0] - V[3], pw[1] - V[7], pw[2] - V[11]
        ok &= np.maximum(np.maximum(np.abs(ax), np.abs(ay)), np.abs(az)) < HEADROOM
        J = np.stack([ay * nz - az * ny, az * nx - ax * nz, ax * ny - ay * nx, nx, ny, nz], axis=1)
    return ok, J[ok], r[ok]


def quantise(v, scale):
    """(int64) rint(v * scale), element-wise."""
    return np.rint(np.asarray(v, np.float64) * scale).astype(np.int64)


def sums(J, r, n_used):
    """The 30 int64 sums: 21 J_i J_j (i <= j, i outer), 6 J_i r, r r (each quantised), the inlier count, the used-point count."""
    s = np.zeros(N_TERMS, np.int64)
    for k, (a, b) in enumerate(PAIRS):
        s[k] = quantise(J[:, a] * J[:, b], SCALE_JJ).sum(dtype=np.int64)
    for a in range(6):
        s[21 + a] = quantise(J[:, a] * r, SCALE_JR).sum(dtype=np.int64)
    s[27] = quantise(r * r, SCALE_RR).sum(dtype=np.int64)
    s[28] = len(r)
    s[29] = n_used
    return s


def system(s):
    """(A 6x6 undamped J^T J, b, r r, inliers) as Python floats from the sums."""
    A = [[0.0] * 6 for _ in range(6)]
    for k, (a, b) in enumerate(PAIRS):
        A[a][b] = A[b][a] = float(int(s[k])) / SCALE_JJ
    b = [float(int(s[21 + a])) / SCALE_JR for a in range(6)]
    return A, b, float(int(s[27])) / SCALE_RR, int(s[28])


def solve(A, b, damping):
    """(A + damping I) x = -b by Cholesky L L^T, column j outer; None when a pivot is not > 0."""
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = A[j][j] + damping
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not s > 0.0:
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        s = -b[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s / L[i][i]
    return x


def cayley(omega):
    """R(omega) = I + (2 / (1 + w.w)) ([w]x + [w]x^2), w = omega / 2; a 3x3 list of floats."""
    wx, wy, wz = 0.5 * omega[0], 0.5 * omega[1], 0.5 * omega[2]
    ww = (wx * wx + wy * wy) + wz * wz
    f = 2.0 / (1.0 + ww)
    W = [[0.0, -wz, wy], [wz, 0.0, -wx], [-wy, wx, 0.0]]
    R = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            w2 = (W[i][0] * W[0][j] + W[i][1] * W[1][j]) + W[i][2] * W[2][j]
            R[i][j] = (1.0 if i == j else 0.0) + f * (W[i][j] + w2)
    return R


def update(T, xi, c):
    """R' = R(omega) R, t' = (c + R(omega) (t - c)) + tau; T as 12 floats row-major [R|t]."""
    Rw = cayley(xi[:3])
    e = [T[3] - c[0], T[7] - c[1], T[11] - c[2]]
    out = [0.0] * 12
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = (Rw[i][0] * T[j] + Rw[i][1] * T[4 + j]) + Rw[i][2] * T[8 + j]
        out[4 * i + 3] = (c[i] + ((Rw[i][0] * e[0] + Rw[i][1] * e[1]) + Rw[i][2] * e[2])) + xi[3 + i]
    return out


def model_view(rows, pose, res, view):
    """(drawn rows, z-buffer) of the view: render_ref.zbuffer at the input pose.  view: dict(K, width, height, z_range, min_count,
    splat_radius, max_splat_radius, flags)."""
    return render_ref.zbuffer(rows, pose, view["K"], view["width"], view["height"], res, view.get("z_range", (0.01, 100.0)),
                              view.get("min_count", 0.0), view.get("splat_radius", 0), view.get("max_splat_radius", 4),
                              view.get("flags", 0))


def track(rows, points, pose, res, view, z_clip=(0.28, 0.6), max_iterations=10, min_inliers=6, max_distance=0.05, damping=0.0,
          eps_rotation=1e-6, eps_translation=1e-6):
    """points = the sampled (n, 3) f32 points (depth_points / cloud_points).  Returns a dict shaped as OccupancyGrid.track*'s result
    plus 'history' (the solved twists, in order)."""
    T0 = [float(v) for v in np.asarray(pose, np.float64).reshape(12)]
    c = (T0[3], T0[7], T0[11])
    drawn, zb = model_view(rows, T0, res, view)
    pts = np.asarray(points, np.float32)
    pts = pts[used(pts, z_clip)]
    T, flags, it, history = list(T0), 0, 0, []
    A, rr, inl = [[0.0] * 6 for _ in range(6)], 0.0, 0
    for it in range(1, max_iterations + 1):
        ok, J, r = terms(pts, T, T0, zb, drawn, view["width"], view["height"], view["K"], view.get("z_range", (0.01, 100.0)),
                         max_distance)
        A, b, rr, inl = system(sums(J, r, len(pts)))
        if inl < min_inliers:
            flags = TOO_FEW
            break
        xi = solve(A, b, float(damping))
        if xi is None:
            flags = DEGENERATE
            break
        history.append(xi)
        T = update(T, xi, c)
        o, t = xi[:3], xi[3:]
        if ((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2] < eps_rotation * eps_rotation and
                (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2] < eps_translation * eps_translation):
            flags = CONVERGED
            break
    return {"pose": np.array(T, np.float64).reshape(3, 4), "iterations": it, "flags": flags, "points_used": len(pts),
            "inliers": inl, "rms": math.sqrt(rr / inl) if inl else 0.0, "information": np.array(A, np.float64), "history": history}
