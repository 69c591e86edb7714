#!/usr/bin/env python3
"""Track rates on a full-size model: a 1 mm session of 120 synthetic 640x480 depth + colour frames (1 m^3, colour fusion on,
a clean pass every 30 frames), then a held-out 640x480 uint16 depth frame tracked from a 1 cm / 2 degree guess:

  call      hfpf_track_depth as a user calls it (eps 1e-6, at most 30 iterations): ms per call and the iterations it took
  split     the same call with eps = 0 (it never converges) and max_iterations 1 and 11: per iteration = (t11 - t1) / 10,
            model view (row set + splat + the frame's upload) = t1 - one iteration
  ... at stride 1, 2 and 4.

Every call returns when its result is complete, so wall time around the call is the call's time.  Median of --reps calls after
one warm-up call.  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats`: --kernel-stats names its
kernel_stats.csv, whose rows for the track and render kernels are copied into the output.

usage: python3 tools/track_rate.py [--frames 120] [--reps 7] [--kernel-stats stats.csv] [--out profiles/track_rate.json]
"""
import argparse
import csv
import json
import math
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
SEED, POSE_SEED, HELD_OUT = 0xD3F7, 0x5E3, 40
OPTS = dict(max_distance=0.03, damping=1e-6, z_range=(0.05, 3.0), splat_radius=-1, max_splat_radius=4, cull_backfaces=True)
KERNELS = ("k_track_reduce", "k_render_splat", "k_extract_keys", "k_extract_rows")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts))


def perturbed(pose, deg, shift):
    a = np.array([1.0, -0.5, 0.3]) / math.sqrt(1.34)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    return np.hstack([R @ pose[:, :3], (pose[:, 3] + np.asarray(shift)).reshape(3, 1)])


def kernel_stats(path):
    """{kernel: {calls, mean_us, total_ms}} of the rocprofv3 kernel_stats.csv rows whose name starts with one of KERNELS."""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            short = name.split("(")[0].split("<")[0].split("::")[-1]
            if short in KERNELS:
                e = out.setdefault(short, {"calls": 0, "total_ns": 0.0})
                e["calls"] += int(row["Calls"])
                e["total_ns"] += float(row["TotalDurationNs"])
    return {k: {"calls": v["calls"], "mean_us": v["total_ns"] / v["calls"] / 1e3, "total_ms": v["total_ns"] / 1e6} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_rate.json"))
    a = ap.parse_args()

    poses = [S.pose(POSE_SEED, f) for f in range(a.frames)]
    g = hfpf.OccupancyGrid(resolution=0.001, bbox=BBOX, fuse_color=True, max_bricks=400000, max_log_points=a.frames * W * H,
                           max_normals=24 << 20, max_frames=4096, frame_width=W)
    K = None
    t0 = time.perf_counter()
    for f in range(a.frames):
        depth, rgb, K = S.depth_frame(SEED, f, W, H, poses[f])
        g.integrate_depth(depth, poses[f], K, color=rgb)
        if (f + 1) % 30 == 0:
            g.clean()
    g.clean()
    g.sync()
    log("session: %d frames in %.1f s" % (a.frames, time.perf_counter() - t0))
    n_rows = int(len(g.extract()))
    true = S.pose(POSE_SEED, HELD_OUT)
    depth, _, K = S.depth_frame(SEED, HELD_OUT, W, H, true)
    guess = perturbed(true, 2.0, (0.006, -0.005, 0.006))

    out = {"what": "hfpf_track_depth of a held-out 640x480 uint16 frame on a 1 mm model of %d synthetic 640x480 depth frames" % a.frames,
           "rows": n_rows, "image": [W, H], "reps": a.reps, "start_error": "1 cm / 2 deg", "options": OPTS,
           "stat": "median ms (min ms) per call"}
    for stride in (1, 2, 4):
        pose, r = g.track_depth(depth, guess, K, stride=stride, max_iterations=30, eps_rotation=1e-6, eps_translation=1e-6, **OPTS)
        dR = pose[:, :3] @ true[:, :3].T
        err = (float(np.linalg.norm(pose[:, 3] - true[:, 3])), math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1) / 2)))))
        med, mn = timed(lambda: g.track_depth(depth, guess, K, stride=stride, max_iterations=30, eps_rotation=1e-6,
                                              eps_translation=1e-6, **OPTS), a.reps)
        t1, _ = timed(lambda: g.track_depth(depth, guess, K, stride=stride, max_iterations=1, eps_rotation=0.0, eps_translation=0.0,
                                            **OPTS), a.reps)
        t11, _ = timed(lambda: g.track_depth(depth, guess, K, stride=stride, max_iterations=11, eps_rotation=0.0, eps_translation=0.0,
                                             **OPTS), a.reps)
        per_it = (t11 - t1) / 10
        out["stride%d" % stride] = {"call_ms": med, "call_min_ms": mn, "iterations": r["iterations"], "flags": r["flags"],
                                    "points_used": r["points_used"], "inliers": r["inliers"], "end_error_m_deg": err,
                                    "one_iteration_call_ms": t1, "eleven_iteration_call_ms": t11, "ms_per_iteration": per_it,
                                    "view_and_upload_ms": t1 - per_it}
        log("stride %d: %.3f ms/call, %d iterations, %.4f ms/iteration, view + upload %.3f ms, end error %.2e m / %.4f deg" % (
            stride, med, r["iterations"], per_it, t1 - per_it, *err))
    g.close()
    if a.kernel_stats:
        out["kernels"] = kernel_stats(a.kernel_stats)
        out["kernels_note"] = "from a separate run of this tool under rocprofv3 --kernel-trace --stats (all of its calls)"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
