"""The align contract of include/hfpf.h restated in numpy (imported by tests only): hfpf_extract_filtered's rows + a triangle mesh + a
start pose -> the refined pose, flags, inliers, rms and information hfpf_align_mesh* return.  The contract is "compare + track" and
nothing else, and so is this file: the per-row records are deviation_ref.compare's, the 28 sums, the system, the Cholesky solve and
the Cayley update are track_ref's."""
import math

import numpy as np

import deviation_ref as D
import track_ref as T
from components_ref import count_gate

CONVERGED, DEGENERATE, TOO_FEW = T.CONVERGED, T.DEGENERATE, T.TOO_FEW
SKIP_BOUNDARY = 1


def centre(bbox):
    """c[a] = (bbox_min[a] + bbox_max[a]) * 0.5; bbox = (xmin, xmax, ymin, ymax, zmin, zmax)."""
    b = [float(v) for v in bbox]
    return [(b[0] + b[1]) * 0.5, (b[2] + b[3]) * 0.5, (b[4] + b[5]) * 0.5]


def rigid(deg, axis, t, c):
    """The 3x4 pose of a rotation of `deg` degrees about `axis` through c, followed by the translation t."""
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.radians(deg)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    c = np.asarray(c, np.float64)
    return np.hstack([R, (c - R @ c + np.asarray(t, np.float64)).reshape(3, 1)])


def corner_displacement(pose, true_pose, bbox):
    """The largest displacement of a corner of the bbox under pose o true_pose^-1: 0 when the pose is the true one."""
    P, Q = np.vstack([pose, [0, 0, 0, 1]]), np.vstack([true_pose, [0, 0, 0, 1]])
    M = P @ np.linalg.inv(Q)
    corners = np.array([[bbox[i], bbox[2 + j], bbox[4 + k], 1.0] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    return float(np.linalg.norm((corners @ M.T - corners)[:, :3], axis=1).max())


def terms(rows, dev, c, flags=0):
    """(inlier mask, J (n, 6), r) of the sampled rows and their deviation records."""
    found = (dev["flags"] & D.FOUND) != 0
    ok = found.copy()
    if flags & SKIP_BOUNDARY:
        ok &= (dev["flags"] & (D.ON_EDGE | D.ON_VERTEX)) == 0
    px, py, pz = (rows[k].astype(np.float64) for k in ("x", "y", "z"))
    nx, ny, nz = (rows[k].astype(np.float64) for k in ("nx", "ny", "nz"))
    q = np.where(found[:, None], dev["q"], np.float32(0)).astype(np.float64)
    qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        ok &= ((nx * nx + ny * ny) + nz * nz) <= 2.0
        ax, ay, az = qx - c[0], qy - c[1], qz - c[2]
        ok &= np.maximum(np.maximum(np.abs(ax), np.abs(ay)), np.abs(az)) < T.HEADROOM
        dx, dy, dz = qx - px, qy - py, qz - pz
        r = (nx * dx + ny * dy) + nz * dz
        J = np.stack([ay * nz - az * ny, az * nx - ax * nz, ax * ny - ay * nx, nx, ny, nz], axis=1)
    return ok, J[ok], r[ok]


def align(rows, verts, stride_bytes, tris, pose, bbox, max_iterations=10, stride=1, min_inliers=6, min_count=0.0, max_distance=0.01,
          damping=1e-6, eps_rotation=1e-6, eps_translation=1e-6, flags=0, n_verts=None):
    """rows = hfpf_extract's rows; the mesh as deviation_ref.compare takes it; bbox = the handle's.  Returns a dict shaped as
    OccupancyGrid.align_mesh's plus 'history' (the rms of every system evaluated)."""
    rows = np.asarray(rows)
    rows = rows[count_gate(rows, min_count)]
    sampled = rows[::stride]
    T0 = [float(v) for v in np.asarray(pose, np.float64).reshape(12)]
    c = centre(bbox)
    Tk, out_flags, it, history = list(T0), 0, 0, []
    A, rr, inl = [[0.0] * 6 for _ in range(6)], 0.0, 0
    for it in range(1, max_iterations + 1):
        dev, _ = D.compare(sampled, verts, stride_bytes, tris, np.array(Tk).reshape(3, 4), 0.0, max_distance, n_verts=n_verts)
        ok, J, r = terms(sampled, dev, c, flags)
        A, b, rr, inl = T.system(T.sums(J, r, 0))
        history.append(math.sqrt(rr / inl) if inl else 0.0)
        if inl < min_inliers:
            out_flags = TOO_FEW
            break
        xi = T.solve(A, b, float(damping))
        if xi is None:
            out_flags = DEGENERATE
            break
        Tk = T.update(Tk, xi, c)
        o, t = xi[:3], xi[3:]
        if ((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2] < eps_rotation * eps_rotation and
                (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2] < eps_translation * eps_translation):
            out_flags = CONVERGED
            break
    return {"pose": np.array(Tk, np.float64).reshape(3, 4), "iterations": it, "flags": out_flags, "rows_sampled": len(sampled),
            "inliers": inl, "rms": math.sqrt(rr / inl) if inl else 0.0, "information": np.array(A, np.float64), "history": history}
