"""The point-query contract of include/hfpf.h restated in numpy (imported by tests only): extracted rows + the occupied list + points
and a pose -> the hits and rows hfpf_query* return.  The transform and voxel index are integrate's (tests/depth_ref.py,
hfpf_probe_points); rows come in extract's lexicographic order, so np.searchsorted on their keys finds a cell, and walking the
(2r+1)^3 offsets in lexicographic order with a strict-less running minimum gives the tie rule."""
import numpy as np

import depth_ref

USED, IN_BBOX, OCCUPIED, HAS_ROW, FOUND = 1, 2, 4, 8, 16
INT_MIN = np.iinfo(np.int32).min
NAN_BITS = np.uint32(0x7FC00000)
HIT_DTYPE = np.dtype([("voxel", "<i4", (3,)), ("flags", "<u4"), ("row_voxel", "<i4", (3,)), ("row_count", "<u4"),
                      ("p", "<f4", (3,)), ("distance", "<f4"), ("signed_distance", "<f4"), ("reserved", "<u4", (3,))])
ROW_FIELDS = ("ix", "iy", "iz", "count", "x", "y", "z", "nx", "ny", "nz", "sdx", "sdy", "sdz", "mean_dist", "sd_dist", "rgb")
KEY_BITS = 21  # cell coordinates below 2^21 per axis


def depth_points(depth, K, depth_scale=0.001):
    """Every pixel of a depth image as the f32 points a depth query reads, point i = pixel (i % W, i // W)."""
    return depth_ref.backproject(depth, K, depth_scale)


def transform(T, xyz):
    """p = (float)(((T[0]*x + T[1]*y) + T[2]*z) + T[3]) per row: f64 from the widened f32 input, one rounding to f32."""
    T = np.asarray(T, np.float64).reshape(12)
    x, y, z = (xyz[:, k].astype(np.float64) for k in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([(((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3]).astype(np.float32) for r in range(3)],
                        axis=1)


def voxel(p, bbox, res):
    """(int)floor(((double)p - bbox_min) / res) per axis; INT_MIN for NaN or outside the int range."""
    lo = np.asarray(bbox, np.float64)[0::2]
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((p.astype(np.float64) - lo) / float(res))
        ok = (f >= -2.0 ** 31) & (f < 2.0 ** 31)
    out = np.full(f.shape, INT_MIN, np.int32)
    out[ok] = f[ok].astype(np.int32)
    return out


def in_bbox(p, bbox):
    b = np.asarray(bbox, np.float64)
    q = p.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return ((q > b[0::2]) & (q < b[1::2])).all(axis=1)


def used(points, zclip, z_clip):
    p = np.asarray(points, np.float32)
    ok = np.isfinite(p).all(axis=1)
    if zclip:
        z = p[:, 2].astype(np.float64)
        with np.errstate(invalid="ignore"):
            ok &= (z > float(z_clip[0])) & (z < float(z_clip[1]))
    return ok


def keys(ix, iy, iz):
    return (np.asarray(ix, np.int64) << (2 * KEY_BITS)) | (np.asarray(iy, np.int64) << KEY_BITS) | np.asarray(iz, np.int64)


def candidates(rows, min_count):
    """The rows that are candidates at all: count >= max(1, min_count) (the int count against a double, as extract compares)."""
    return rows[rows["count"].astype(np.int32).astype(np.float64) >= max(1.0, float(min_count))]


def empty_rows(n, dtype):
    r = np.zeros(n, dtype)
    for k in ("ix", "iy", "iz"):
        r[k] = -1
    return r


def _finish(points, pose, bbox, res, occupied, z_clip, zclip):
    """The per-point part that needs no rows: (hits with flags USED / IN_BBOX / OCCUPIED, voxel and p; searched mask; voxel)."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    n = pts.shape[0]
    hits = np.zeros(n, HIT_DTYPE)
    hits["voxel"] = INT_MIN
    hits["row_voxel"] = -1
    for k in ("distance", "signed_distance"):
        hits[k].view(np.uint32)[:] = NAN_BITS
    hits["p"].view(np.uint32)[:] = NAN_BITS
    u = used(pts, zclip, z_clip)
    p = transform(pose, pts)
    v = voxel(p, bbox, res)
    ib = u & in_bbox(p, bbox)
    hits["flags"][u] = USED
    hits["flags"][ib] |= IN_BBOX
    hits["voxel"][u] = v[u]
    hits["p"][u] = p[u]
    occ = np.asarray(occupied, np.int64).reshape(-1, 3)
    if len(occ) and ib.any():
        ok = np.sort(keys(occ[:, 0], occ[:, 1], occ[:, 2]))
        vk = keys(v[ib, 0], v[ib, 1], v[ib, 2])
        j = np.minimum(np.searchsorted(ok, vk), len(ok) - 1)
        hits["flags"][np.flatnonzero(ib)[ok[j] == vk]] |= OCCUPIED
    return hits, p, v, ib


def query(rows, occupied, points, pose, bbox, res, z_clip=(0.28, 0.6), radius=1, min_count=0.0, max_distance=np.inf, zclip=False):
    """(hits, rows) of hfpf_query for extracted rows (lexicographic order) and hfpf_get_occupied's list."""
    hits, p, v, ib = _finish(points, pose, bbox, res, occupied, z_clip, zclip)
    out = empty_rows(len(hits), rows.dtype)
    cand = candidates(rows, min_count)
    if not len(cand) or not ib.any():
        return hits, out
    ck = keys(cand["ix"], cand["iy"], cand["iz"])
    assert (np.diff(ck) > 0).all(), "rows are not in extract's order"
    idx = np.flatnonzero(ib)
    pv = v[idx].astype(np.int64)
    pp = p[idx].astype(np.float64)
    md2 = float(max_distance) * float(max_distance)
    best = np.full(len(idx), -1, np.int64)
    best_d2 = np.full(len(idx), np.inf)
    has_row = np.zeros(len(idx), bool)
    cx, cy, cz = (cand[k].astype(np.float64) for k in ("x", "y", "z"))
    r = int(radius)
    for ox in range(-r, r + 1):
        for oy in range(-r, r + 1):
            for oz in range(-r, r + 1):
                t = pv + np.array([ox, oy, oz], np.int64)
                ok = ((t >= 0) & (t < (1 << KEY_BITS))).all(axis=1)
                tk = keys(t[:, 0], t[:, 1], t[:, 2])
                j = np.minimum(np.searchsorted(ck, tk), len(ck) - 1)
                ok &= ck[j] == tk
                if (ox, oy, oz) == (0, 0, 0):
                    has_row |= ok
                dx, dy, dz = pp[:, 0] - cx[j], pp[:, 1] - cy[j], pp[:, 2] - cz[j]
                d2 = (dx * dx + dy * dy) + dz * dz
                ok &= d2 <= md2
                take = ok & ((best < 0) | (d2 < best_d2))
                best = np.where(take, j, best)
                best_d2 = np.where(take, d2, best_d2)
    hits["flags"][idx[has_row]] |= HAS_ROW
    f = best >= 0
    fi, w = idx[f], cand[best[f]]
    d = pp[f] - np.stack([w["x"], w["y"], w["z"]], axis=1).astype(np.float64)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    hits["flags"][fi] |= FOUND
    hits["row_voxel"][fi] = np.stack([w["ix"], w["iy"], w["iz"]], axis=1)
    hits["row_count"][fi] = w["count"]
    hits["distance"][fi] = np.sqrt(d2).astype(np.float32)
    n = np.stack([w["nx"], w["ny"], w["nz"]], axis=1).astype(np.float64)
    hits["signed_distance"][fi] = ((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]).astype(np.float32)
    out[fi] = w
    return hits, out


def nearest_ties(rows, hits, pts, radius, min_count=0.0, max_distance=np.inf):
    """Per point (bool): FOUND, and the smallest d2 is shared by two or more candidate rows of the window, so that the tie rule
    (the lexicographically smallest (ix, iy, iz)) decided the row.  hits = query()'s of pts under the identity pose with the same
    options; d2 is query()'s expression, compared exactly."""
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    tied = np.zeros(len(p), bool)
    idx = np.flatnonzero(hits["flags"] & FOUND != 0)
    cand = candidates(rows, min_count)
    if not len(idx) or not len(cand):
        return tied
    ck = keys(cand["ix"], cand["iy"], cand["iz"])
    pv = hits["voxel"][idx].astype(np.int64)
    pp = p[idx].astype(np.float64)
    md2 = float(max_distance) * float(max_distance)
    best_d2 = np.full(len(idx), np.inf)
    n_best = np.zeros(len(idx), np.int64)
    cx, cy, cz = (cand[k].astype(np.float64) for k in ("x", "y", "z"))
    r = int(radius)
    for ox in range(-r, r + 1):
        for oy in range(-r, r + 1):
            for oz in range(-r, r + 1):
                t = pv + np.array([ox, oy, oz], np.int64)
                ok = ((t >= 0) & (t < (1 << KEY_BITS))).all(axis=1)
                tk = keys(t[:, 0], t[:, 1], t[:, 2])
                j = np.minimum(np.searchsorted(ck, tk), len(ck) - 1)
                ok &= ck[j] == tk
                dx, dy, dz = pp[:, 0] - cx[j], pp[:, 1] - cy[j], pp[:, 2] - cz[j]
                d2 = (dx * dx + dy * dy) + dz * dz
                ok &= d2 <= md2
                less = ok & (d2 < best_d2)
                n_best = np.where(less, 1, n_best + (ok & (d2 == best_d2)))
                best_d2 = np.where(less, d2, best_d2)
    assert (n_best >= 1).all(), "a found point without a candidate"
    tied[idx] = n_best >= 2
    return tied


def brute_force(rows, occupied, points, pose, bbox, res, z_clip=(0.28, 0.6), radius=1, min_count=0.0, max_distance=np.inf, zclip=False):
    """The same by an O(N * M) scan of every candidate row per point (tests of query() itself)."""
    hits, p, v, ib = _finish(points, pose, bbox, res, occupied, z_clip, zclip)
    out = empty_rows(len(hits), rows.dtype)
    cand = candidates(rows, min_count)
    cv = np.stack([cand["ix"], cand["iy"], cand["iz"]], axis=1).astype(np.int64)
    cxyz = np.stack([cand["x"], cand["y"], cand["z"]], axis=1).astype(np.float64)
    md2 = float(max_distance) * float(max_distance)
    for i in np.flatnonzero(ib):
        cheb = np.abs(cv - v[i].astype(np.int64)).max(axis=1) if len(cand) else np.zeros(0, np.int64)
        near = cheb <= radius
        if (near & (cheb == 0)).any():
            hits["flags"][i] |= HAS_ROW
        d = p[i].astype(np.float64) - cxyz
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        ok = np.flatnonzero(near & (d2 <= md2))
        if not len(ok):
            continue
        order = np.lexsort((cv[ok, 2], cv[ok, 1], cv[ok, 0], d2[ok]))  # d2 first, then (ix, iy, iz)
        j = ok[order[0]]
        w = cand[j]
        hits["flags"][i] |= FOUND
        hits["row_voxel"][i] = (w["ix"], w["iy"], w["iz"])
        hits["row_count"][i] = w["count"]
        hits["distance"][i] = np.float32(np.sqrt(d2[j]))
        dj = d[j]
        hits["signed_distance"][i] = np.float32((float(w["nx"]) * dj[0] + float(w["ny"]) * dj[1]) + float(w["nz"]) * dj[2])
        out[i] = w
    return hits, out
