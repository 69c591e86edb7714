"""The raycast contract of include/hfpf.h restated in numpy (imported by tests only): extracted rows + the occupied list + rays and a
pose -> the hits hfpf_raycast* return.  Every sample of every ray is a query_ref.query of its f32 point under the identity pose;
nothing is skipped.  The rays march in lock step, `block` samples at a time, and a ray leaves the march only where the contract ends
it (at its crossing), so the work is the dense march's."""
import numpy as np

import query_ref as Q

USED, HIT, BACKFACE, NEAR = 1, 2, 4, 8
NAN_BITS = np.uint32(0x7FC00000)
RAY_DTYPE = np.dtype([("o", "<f4", (3,)), ("d", "<f4", (3,))])
HIT_DTYPE = np.dtype([("t", "<f4"), ("flags", "<u4"), ("p", "<f4", (3,)), ("n", "<f4", (3,)), ("row_voxel", "<i4", (3,)),
                      ("rgb", "<u4"), ("count", "<u4"), ("sample", "<u4"), ("reserved", "<u4", (2,))])
IDENT = np.hstack([np.eye(3), np.zeros((3, 1))])
MAX_SAMPLES = 1 << 20


def no_hits(n):
    h = np.zeros(n, HIT_DTYPE)
    for k in ("t", "p", "n"):
        h[k].view(np.uint32)[...] = NAN_BITS
    h["row_voxel"] = -1
    return h


def n_samples(t0, t1, step, res):
    """n = (uint64)floor((t1 - t0) / dt) + 1 with dt = step * res."""
    return int(np.floor((float(t1) - float(t0)) / (float(step) * float(res)))) + 1


def general_rays(rays, pose):
    """(O, D, used) of packed {o, d} f32 rays in the camera frame: f64, left to right; D normalised."""
    r = np.asarray(rays)
    r = r.view(np.float32).reshape(-1, 6) if r.dtype == RAY_DTYPE else np.asarray(r, np.float32).reshape(-1, 6)
    T = np.asarray(pose, np.float64).reshape(12)
    o, d = r[:, :3].astype(np.float64), r[:, 3:].astype(np.float64)
    with np.errstate(all="ignore"):
        O = np.stack([((T[4 * a] * o[:, 0] + T[4 * a + 1] * o[:, 1]) + T[4 * a + 2] * o[:, 2]) + T[4 * a + 3] for a in range(3)], axis=1)
        W = np.stack([(T[4 * a] * d[:, 0] + T[4 * a + 1] * d[:, 1]) + T[4 * a + 2] * d[:, 2] for a in range(3)], axis=1)
        L = np.sqrt((W[:, 0] * W[:, 0] + W[:, 1] * W[:, 1]) + W[:, 2] * W[:, 2])
        used = np.isfinite(r).all(axis=1) & np.isfinite(L) & (L > 0)
        D = W / L[:, None]
    return O, D, used


def view_rays(pose, K, width, height):
    """(O, D, used) of the view rays of a pinhole, ray i = pixel (i % width, i // width); D is not normalised."""
    T = np.asarray(pose, np.float64).reshape(12)
    fx, fy, cx, cy = (float(x) for x in K)
    v, u = np.divmod(np.arange(int(width) * int(height), dtype=np.int64), int(width))
    xn = (u.astype(np.float64) - cx) / fx
    yn = (v.astype(np.float64) - cy) / fy
    D = np.stack([(T[4 * a] * xn + T[4 * a + 1] * yn) + T[4 * a + 2] for a in range(3)], axis=1)
    O = np.broadcast_to(np.array([T[3], T[7], T[11]]), D.shape).copy()
    return O, D, np.ones(len(D), bool)


def march(rows, occupied, O, D, used, bbox, res, radius=2, min_count=0.0, max_distance=np.inf, step=0.5, t_range=(0.0, 1.0),
          cull_backfaces=False, block=16):
    """The hits of rays O + t * D (fusion frame, f64)."""
    t0, t1 = float(t_range[0]), float(t_range[1])
    dt = float(step) * float(res)
    n = n_samples(t0, t1, step, res)
    assert n <= MAX_SAMPLES
    hits = no_hits(len(O))
    hits["flags"][used] = USED
    act = np.flatnonzero(used)                 # rays still marching
    prev_def = np.zeros(len(O), bool)
    prev_s = np.zeros(len(O), np.float32)
    prev_row = Q.empty_rows(len(O), rows.dtype)
    near = np.zeros(len(O), bool)
    for k0 in range(0, n, block):
        if not len(act):
            break
        ks = np.arange(k0, min(k0 + block, n))
        tk = t0 + ks.astype(np.float64) * dt
        with np.errstate(all="ignore"):
            p = (O[act][:, None, :] + tk[None, :, None] * D[act][:, None, :]).astype(np.float32)
        qh, qr = Q.query(rows, occupied, p.reshape(-1, 3), IDENT, bbox, res, radius=radius, min_count=min_count, max_distance=max_distance)
        df = ((qh["flags"] & Q.FOUND) != 0).reshape(len(act), len(ks))
        s = qh["signed_distance"].reshape(len(act), len(ks))
        qr = qr.reshape(len(act), len(ks))
        done = np.zeros(len(act), bool)
        for j, k in enumerate(ks):
            live = ~done
            r = act[live]
            d_k, s_k = df[live, j], s[live, j]
            near[r] |= d_k
            with np.errstate(invalid="ignore"):
                cross = prev_def[r] & d_k & ((prev_s[r] < 0) != (s_k < 0))
                back = cross & (prev_s[r] < 0)
            end = cross & ~back if cull_backfaces else cross
            if end.any():
                e = r[end]
                sa, sb = prev_s[e].astype(np.float64), s_k[end].astype(np.float64)
                w = sa / (sa - sb)
                th = (t0 + float(k - 1) * dt) + w * dt
                cur = np.abs(s_k[end]) < np.abs(prev_s[e])
                row = np.where(cur, qr[live, j][end], prev_row[e])
                hits["t"][e] = th.astype(np.float32)
                hits["flags"][e] |= HIT | np.where(back[end], BACKFACE, 0).astype(np.uint32)
                hits["p"][e] = (O[e] + th[:, None] * D[e]).astype(np.float32)
                hits["n"][e] = np.stack([row["nx"], row["ny"], row["nz"]], axis=1)
                hits["row_voxel"][e] = np.stack([row["ix"], row["iy"], row["iz"]], axis=1)
                hits["rgb"][e] = row["rgb"].view(np.uint32) if row["rgb"].dtype.itemsize == 4 else row["rgb"]
                hits["count"][e] = row["count"]
                hits["sample"][e] = k
                done[np.flatnonzero(live)[end]] = True
            keep = r[~end]
            prev_def[keep] = d_k[~end]
            prev_s[keep] = s_k[~end]
            prev_row[keep] = qr[live, j][~end]
        act = act[~done]
    hits["flags"][near] |= NEAR
    return hits


def raycast(rows, occupied, rays, pose, bbox, res, **opts):
    """hfpf_raycast / hfpf_raycast_device."""
    O, D, used = general_rays(rays, pose)
    return march(rows, occupied, O, D, used, bbox, res, **opts)


def raycast_view(rows, occupied, pose, K, width, height, bbox, res, **opts):
    """hfpf_raycast_view / one view of hfpf_raycast_view_device, as (height, width) hits."""
    O, D, used = view_rays(pose, K, width, height)
    return march(rows, occupied, O, D, used, bbox, res, **opts).reshape(int(height), int(width))
