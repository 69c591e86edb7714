"""The depth-consistency contract of include/hfpf.h restated in numpy (imported by tests only): extracted rows + depth frames with their
poses -> the per-row records hfpf_depth_consistency returns, the summary and the kept rows.  Every operation f64, left to right, one
rounding each, as the engine evaluates it; the depth sample of a U16 frame is the f32 product of the depth-frame contract.  consistency()
is vectorised over the rows, one frame at a time; scalar_records() is the same contract as a plain double loop."""
import math

import numpy as np

DROP = 1
SEEN, SUPPORTED, CONTRADICTED = 1, 2, 4
NONE = 0xFFFFFFFF
IN_VIEW, TESTED, SUPPORT, NO_DEPTH, OCCLUDED, THROUGH = 1, 2, 3, 4, 5, 6  # classes of a (row, frame): IN_VIEW = in view, not tested
DTYPE = np.dtype([(k, "<u4") for k in ("n_in_view", "n_tested", "n_support", "n_through", "n_occluded", "first_through", "flags", "reserved")])
SUMMARY_KEYS = ("n_rows", "n_seen", "n_supported", "n_contradicted", "n_kept", "pairs_tested", "pairs_support", "pairs_through")
DEFAULTS = dict(window=0, min_through=1, min_count=0.0, z_range=(0.01, 100.0), tolerance=0.004, slope=0.0, min_cos=0.3, through_ratio=1.0, drop=False)


def row_set(rows, min_count=0.0):
    """The row set: hfpf_extract_filtered's compare, rows with (double)(int)count < min_count dropped."""
    c = rows["count"].astype(np.int64).astype(np.int32).astype(np.float64)
    return rows[~(c < float(min_count))]


def samples(frame, depth_scale):
    """(zd as f64, valid) of every pixel of one frame (uint16 counts or float32 metres)."""
    frame = np.asarray(frame)
    if frame.dtype == np.uint16:
        zd = (frame.astype(np.float32) * np.float32(depth_scale)).astype(np.float64)
        return zd, frame != 0
    assert frame.dtype == np.float32, frame.dtype
    return frame.astype(np.float64), np.isfinite(frame)


def as_f32(frame, depth_scale):
    """A U16 frame as the F32 frame with the same samples: invalid pixels NaN."""
    zd, valid = samples(frame, depth_scale)
    return np.where(valid, zd, np.nan).astype(np.float32)


def classify(rows, frame, pose, K, depth_scale=0.001, window=0, z_range=(0.01, 100.0), tolerance=0.004, slope=0.0, min_cos=0.3):
    """The class of every row of the row set against one frame: 0 (not in view), IN_VIEW (gated out), SUPPORT, NO_DEPTH, OCCLUDED, THROUGH."""
    T = np.asarray(pose, dtype=np.float64).reshape(12)
    fx, fy, cx, cy = (float(k) for k in K)
    H, W = frame.shape
    x, y, z = (rows[k].astype(np.float64) for k in ("x", "y", "z"))
    nx, ny, nz = (rows[k].astype(np.float64) for k in ("nx", "ny", "nz"))
    dx, dy, dz = x - T[3], y - T[7], z - T[11]
    xc = (T[0] * dx + T[4] * dy) + T[8] * dz
    yc = (T[1] * dx + T[5] * dy) + T[9] * dz
    zc = (T[2] * dx + T[6] * dy) + T[10] * dz
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = (float(z_range[0]) < zc) & (zc < float(z_range[1]))
        u = (xc / zc) * fx + cx
        v = (yc / zc) * fy + cy
        ok &= (np.abs(u) < 2.0 ** 30) & (np.abs(v) < 2.0 ** 30)
        pu = np.where(ok, np.floor(u + 0.5), -1.0).astype(np.int64)
        pv = np.where(ok, np.floor(v + 0.5), -1.0).astype(np.int64)
        ok &= (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
        tested = ok.copy()
        if min_cos >= 0:
            c = -((nx * dx + ny * dy) + nz * dz)
            d2 = (dx * dx + dy * dy) + dz * dz
            tested &= (c > 0.0) & (c * c >= (float(min_cos) * float(min_cos)) * d2)
        tol = float(tolerance) + float(slope) * zc
    cls = np.zeros(len(rows), np.int64)
    cls[ok] = IN_VIEW
    idx = np.flatnonzero(tested)
    if idx.size == 0:
        return cls
    zd, valid = samples(frame, depth_scale)
    off = np.arange(-int(window), int(window) + 1, dtype=np.int64)
    px = pu[idx][:, None, None] + off[None, None, :] + 0 * off[None, :, None]
    py = pv[idx][:, None, None] + off[None, :, None] + 0 * off[None, None, :]
    inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
    pxc, pyc = np.clip(px, 0, W - 1), np.clip(py, 0, H - 1)
    val = inside & valid[pyc, pxc]
    g = zd[pyc, pxc] - zc[idx][:, None, None]
    t = tol[idx][:, None, None]
    with np.errstate(invalid="ignore"):
        support = (val & (np.abs(g) <= t)).any(axis=(1, 2))
        occluded = (val & (g < -t)).any(axis=(1, 2))
    any_valid = val.any(axis=(1, 2))
    cls[idx] = np.where(support, SUPPORT, np.where(~any_valid, NO_DEPTH, np.where(occluded, OCCLUDED, THROUGH)))
    return cls


def records_of(classes):
    """The records of the (n_frames, n_rows) class matrix, flags still 0."""
    classes = np.asarray(classes)
    assert classes.ndim == 2, classes.shape
    rec = np.zeros(classes.shape[1], DTYPE)
    rec["first_through"] = NONE
    for f, cls in enumerate(classes):
        rec["n_in_view"] += (cls != 0).astype(np.uint32)
        rec["n_tested"] += (cls >= SUPPORT).astype(np.uint32)
        rec["n_support"] += (cls == SUPPORT).astype(np.uint32)
        rec["n_through"] += (cls == THROUGH).astype(np.uint32)
        rec["n_occluded"] += (cls == OCCLUDED).astype(np.uint32)
        rec["first_through"] = np.where((cls == THROUGH) & (rec["first_through"] == NONE), f, rec["first_through"]).astype(np.uint32)
    return rec


def finish(rec, min_through=1, through_ratio=1.0):
    """Sets the flags of rec in place; returns (contradicted mask, summary dict)."""
    nt, ns = rec["n_through"], rec["n_support"]
    contra = (nt >= max(1, int(min_through))) & (nt.astype(np.float64) > float(through_ratio) * ns.astype(np.float64))
    rec["flags"] = (np.where(rec["n_tested"] > 0, SEEN, 0) | np.where(ns > 0, SUPPORTED, 0) | np.where(contra, CONTRADICTED, 0)).astype(np.uint32)
    s = dict(n_rows=len(rec), n_seen=int((rec["n_tested"] > 0).sum()), n_supported=int((ns > 0).sum()), n_contradicted=int(contra.sum()),
             n_kept=len(rec) - int(contra.sum()), pairs_tested=int(rec["n_tested"].astype(np.uint64).sum()),
             pairs_support=int(ns.astype(np.uint64).sum()), pairs_through=int(nt.astype(np.uint64).sum()))
    return contra, s


def consistency(rows, frames, poses, K, depth_scale=0.001, **kw):
    """(output rows, records, summary) of hfpf_depth_consistency on hfpf_extract's rows; keywords as hfpf.consistency_opts()."""
    o = dict(DEFAULTS, **kw)
    rows = row_set(rows, o["min_count"])
    ck = dict(depth_scale=depth_scale, window=o["window"], z_range=o["z_range"], tolerance=o["tolerance"], slope=o["slope"], min_cos=o["min_cos"])
    classes = np.zeros((len(frames), len(rows)), np.int8)
    for f in range(len(frames)):
        classes[f] = classify(rows, np.asarray(frames[f]), poses[f], K, **ck)
    rec = records_of(classes)
    contra, s = finish(rec, o["min_through"], o["through_ratio"])
    if o["drop"]:
        return rows[~contra], rec[~contra], s
    return rows, rec, s


def scalar_class(row, frame, pose, K, depth_scale=0.001, window=0, z_range=(0.01, 100.0), tolerance=0.004, slope=0.0, min_cos=0.3):
    """classify() for one row as plain Python floats (IEEE doubles), pixel by pixel."""
    T = [float(t) for t in np.asarray(pose, np.float64).reshape(12)]
    fx, fy, cx, cy = (float(k) for k in K)
    H, W = frame.shape
    x, y, z, nx, ny, nz = (float(np.float64(row[k])) for k in ("x", "y", "z", "nx", "ny", "nz"))
    dx, dy, dz = x - T[3], y - T[7], z - T[11]
    xc = (T[0] * dx + T[4] * dy) + T[8] * dz
    yc = (T[1] * dx + T[5] * dy) + T[9] * dz
    zc = (T[2] * dx + T[6] * dy) + T[10] * dz
    if not (z_range[0] < zc < z_range[1]):
        return 0
    u = (xc / zc) * fx + cx
    v = (yc / zc) * fy + cy
    if not (abs(u) < 2.0 ** 30 and abs(v) < 2.0 ** 30):
        return 0
    pu, pv = int(math.floor(u + 0.5)), int(math.floor(v + 0.5))
    if not (0 <= pu < W and 0 <= pv < H):
        return 0
    if min_cos >= 0:
        c = -((nx * dx + ny * dy) + nz * dz)
        d2 = (dx * dx + dy * dy) + dz * dz
        if not (c > 0.0 and c * c >= (min_cos * min_cos) * d2):
            return IN_VIEW
    tol = tolerance + slope * zc
    any_valid = occluded = False
    for j in range(-window, window + 1):
        for i in range(-window, window + 1):
            px, py = pu + i, pv + j
            if not (0 <= px < W and 0 <= py < H):
                continue
            d = frame[py, px]
            if frame.dtype == np.uint16:
                if d == 0:
                    continue
                zd = float(np.float32(d) * np.float32(depth_scale))
            else:
                if not np.isfinite(d):
                    continue
                zd = float(d)
            g = zd - zc
            if abs(g) <= tol:
                return SUPPORT
            any_valid = True
            occluded = occluded or g < -tol
    return NO_DEPTH if not any_valid else OCCLUDED if occluded else THROUGH


def scalar_records(rows, frames, poses, K, depth_scale=0.001, **kw):
    """records (flags 0) by the scalar double loop over rows and frames."""
    return records_of([[scalar_class(r, np.asarray(frames[f]), poses[f], K, depth_scale, **kw) for r in rows] for f in range(len(frames))])


# ---- the scene of the GPU tests ---------------------------------------------------------------------------------------------------

GHOST_SIDE, GHOST_DEPTH = 0.032, 0.30  # metres: the side of the ghost square and its camera-frame z (inside the z-clip 0.28 .. 0.6)


def ghost_cloud(res, per_edge=3):
    """Something that crossed the view once: a GHOST_SIDE square of points, per_edge per voxel edge, at camera-frame z = GHOST_DEPTH on
    the optical axis, as packed 16-byte x, y, z, rgb records (to be integrated at the pose of a frame that later looks through it)."""
    n = int(round(GHOST_SIDE / res)) * per_edge
    t = ((np.arange(n) + 0.5) / n - 0.5) * GHOST_SIDE
    u, v = np.meshgrid(t, t, indexing="ij")
    rec = np.zeros((u.size, 4), np.float32)
    rec[:, 0], rec[:, 1], rec[:, 2] = u.ravel(), v.ravel(), GHOST_DEPTH
    rec[:, 3] = np.array([0x00FF00FF], np.uint32).view(np.float32)[0]
    return np.ascontiguousarray(rec)


def tampered(frame):
    """A U16 frame with three rectangles changed (valid pixels only): 50 counts farther in [20:50, 20:60] (the model in front of it is
    seen THROUGH), 50 counts nearer in [70:100, 20:60] (OCCLUDED), no reading in [40:80, 100:140] (NO_DEPTH)."""
    t = np.array(frame, np.uint16, copy=True)
    far, near = t[20:50, 20:60], t[70:100, 20:60]
    far[far != 0] += 50
    near[near > 50] -= 50
    t[40:80, 100:140] = 0
    return t


def voxel_keys(rows):
    return (rows["ix"].astype(np.int64) << 42) | (rows["iy"].astype(np.int64) << 21) | rows["iz"].astype(np.int64)


def csv(rows, rec):
    """consistency.csv of the node shell."""
    lines = ["ix,iy,iz,n_in_view,n_tested,n_support,n_through,n_occluded,first_through,flags"]
    for r, c in zip(rows, rec):
        lines.append("%d,%d,%d,%d,%d,%d,%d,%d,%d,%d" % (r["ix"], r["iy"], r["iz"], c["n_in_view"], c["n_tested"], c["n_support"], c["n_through"],
                                                       c["n_occluded"], c["first_through"], c["flags"]))
    return "\n".join(lines) + "\n"


def summary_csv(s):
    return ",".join(SUMMARY_KEYS) + "\n" + ",".join("%d" % s[k] for k in SUMMARY_KEYS) + "\n"
