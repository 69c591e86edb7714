#!/usr/bin/env python3
"""Align rates on a full-size model: the 1 mm session of 120 synthetic 640x480 depth + colour frames tools/deviation_rate.py builds,
then the model's own mesh, left in HBM (hfpf_extract_mesh_device), best-fitted to the model from a pose a small rigid motion away
(--degrees about the bounding box's centre, --shift voxels of translation): hfpf_align_mesh_device at max_distance = --voxels voxels,
stride 1 and stride 4, with hfpf_compare_mesh_device of the same session at the same max_distance (at the start pose) beside it.

Every call returns when its result is complete, so wall time around the call is the call's time.  Median and min of --reps calls
after one warm-up call; ms_per_iteration divides by the iterations the call reports.  compare_kernels_ms is the engine's own event
timing of the compare (hfpf_get_kernel_time id 7), the mean over the timed calls; an align has no id.  The fit itself is recorded too:
iterations, flags, inliers, rms, and how far a corner of the bounding box is from where the true pose (the identity) puts it, before
and after.

usage: python3 tools/align_rate.py [--frames 120] [--resolution 0.001] [--reps 3] [--voxels 3] [--out profiles/align_rate.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "high-fidelity-pointcloud-fusion_amd", "python"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import hfpf  # noqa: E402
import hfpf_synth as S  # noqa: E402

W, H = 640, 480
BBOX = (-0.5, 0.5, -0.5, 0.5, 0.0, 1.0)
SEED, POSE_SEED = 0xD3F7, 0x5E3


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(fn, reps, after=lambda r: None):
    ts, r = [], None
    for i in range(reps + 1):  # the first call warms up
        t0 = time.perf_counter()
        r = fn()
        ms = (time.perf_counter() - t0) * 1e3
        after(r)
        if i:
            ts.append(ms)
    return [float(np.median(ts)), float(min(ts))], r


def rigid(deg, axis, t, c):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.radians(deg)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    c = np.asarray(c, np.float64)
    return np.hstack([R, (c - R @ c + np.asarray(t, np.float64)).reshape(3, 1)])


def corner_displacement(pose):
    corners = np.array([[BBOX[i], BBOX[2 + j], BBOX[4 + k], 1.0] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    return float(np.linalg.norm(corners @ np.asarray(pose).T - corners[:, :3], axis=1).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--resolution", type=float, default=0.001)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--voxels", type=float, default=3.0)
    ap.add_argument("--degrees", type=float, default=0.05)
    ap.add_argument("--shift", type=float, default=1.0)
    ap.add_argument("--max-iterations", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_rate.json"))
    a = ap.parse_args()

    poses = [S.pose(POSE_SEED, f) for f in range(a.frames)]
    g = hfpf.OccupancyGrid(resolution=a.resolution, bbox=BBOX, fuse_color=True, max_bricks=400000, max_log_points=a.frames * W * H,
                           max_normals=24 << 20, max_frames=4096, frame_width=W)
    t0 = time.perf_counter()
    for f in range(a.frames):
        depth, rgb, K = S.depth_frame(SEED, f, W, H, poses[f])
        g.integrate_depth(depth, poses[f], K, color=rgb)
        if (f + 1) % 30 == 0:
            g.clean()
    g.clean()
    g.sync()
    log("session: %d frames in %.1f s" % (a.frames, time.perf_counter() - t0))
    n_rows = len(g.extract())
    dv, nv, dt, nt = g.extract_mesh_device()
    md = a.voxels * a.resolution
    c = [(BBOX[0] + BBOX[1]) * 0.5, (BBOX[2] + BBOX[3]) * 0.5, (BBOX[4] + BBOX[5]) * 0.5]
    s = a.shift * a.resolution
    start = rigid(a.degrees, (0.5, 1.0, -0.4), (0.6 * s, -0.64 * s, 0.48 * s), c)
    out = {"what": "hfpf_align_mesh_device of a %g m model of %d synthetic 640x480 depth frames against its own mesh in HBM, started %g degrees "
                   "and %g voxels off" % (a.resolution, a.frames, a.degrees, a.shift),
           "rows": int(n_rows), "vertices": int(nv), "triangles": int(nt), "reps": a.reps, "stat": "[median ms, min ms] per call",
           "max_distance": md, "max_iterations": a.max_iterations, "start_corner_displacement": corner_displacement(start)}

    def free(r):
        for p in (r[0], r[1]):
            if p:
                g.device_free(p)

    g.kernel_timing(1)
    out["compare_device_ms"], r = timed(lambda: g.compare_mesh(dv, dt, start, device=True, n_verts=nv, vertex_stride=32, n_tris=nt, max_distance=md),
                                        a.reps, free)
    ms, n = g.kernel_time(7)
    g.kernel_timing(0)
    out["compare_kernels_ms"] = ms / max(n, 1)
    out["compare_found_fraction_at_start"] = r[3]["n_found"] / max(1, r[3]["n_rows"])
    log("compare at the start pose: %s ms, found %.3f" % (out["compare_device_ms"], out["compare_found_fraction_at_start"]))
    for stride in (1, 4):
        t, r = timed(lambda: g.align_mesh(dv, dt, start, device=True, n_verts=nv, vertex_stride=32, n_tris=nt, max_distance=md, stride=stride,
                                          max_iterations=a.max_iterations, eps_rotation=1e-5, eps_translation=0.01 * a.resolution), a.reps)
        e = {"align_device_ms": t, "ms_per_iteration": t[0] / max(1, r["iterations"]), "iterations": r["iterations"],
             "flags": r["flags"], "rows_sampled": r["rows_sampled"], "inliers": r["inliers"], "rms": r["rms"],
             "corner_displacement": corner_displacement(r["pose"]), "iterations_x_compare_ms": r["iterations"] * out["compare_device_ms"][0]}
        out["stride_%d" % stride] = e
        log("stride %d: %s" % (stride, e))
    g.device_free(dv), g.device_free(dt)
    out["device_bytes"] = int(g.counters()["device_bytes"])
    g.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
