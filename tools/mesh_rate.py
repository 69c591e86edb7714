#!/usr/bin/env python3
"""Mesh rates on a full-size model: a 1 mm session of 120 synthetic 640x480 depth + colour frames (1 m^3, colour fusion on, a clean
pass every 30 frames; the model tools/query_rate.py builds), then the model meshed in two forms:

  host     hfpf_extract_mesh: vertices and triangles downloaded to pageable host arrays
  device   hfpf_extract_mesh_device: vertices and triangles left in fresh HBM arrays (freed after each call, outside the timing)
  ... at radius 1, 2 and 4; and hfpf_extract on the same model (what a user calls today before a CPU mesher).

Every call returns when its outputs are complete, so wall time around the call is the call's time.  Median and min of --reps calls
after one warm-up call.  The cube and corner counts are the contract's sets, counted here in numpy from the extracted rows.  Kernel
times come from a separate run under `rocprofv3 --kernel-trace --stats`: --kernel-stats names its kernel_stats.csv, whose rows for the
mesh, rocPRIM and extract kernels are copied into the output.

usage: python3 tools/mesh_rate.py [--frames 120] [--reps 7] [--kernel-stats stats.csv] [--out profiles/mesh_rate.json]
"""
import argparse
import csv
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
import mesh_ref  # noqa: E402

W, H = 640, 480
BBOX = (-0.5, 0.5, -0.5, 0.5, 0.0, 1.0)
SEED, POSE_SEED = 0xD3F7, 0x5E3
RADII = (1, 2, 4)


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


def kernel_stats(path):
    """{kernel: {calls, mean_us, total_ms}} of the rocprofv3 kernel_stats.csv rows of the mesh call's kernels."""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            short = name.split("(")[0].split("<")[0].split("::")[-1]
            if "rocprim" in name:
                short = "rocprim " + ("lookback init" if "lookback_scan_state" in name else "sort" if "sort" in name else
                                      "unique" if "select" in name or "unique" in name else "scan" if "scan" in name else "other")
            elif "fillBuffer" in name:
                short = "buffer fill"
            elif not (short.startswith("k_mesh") or short.startswith("k_extract")):
                continue
            e = out.setdefault(short, {"calls": 0, "total_ns": 0.0})
            e["calls"] += int(row["Calls"])
            e["total_ns"] += float(row["TotalDurationNs"])
    return {k: {"calls": v["calls"], "mean_us": v["total_ns"] / v["calls"] / 1e3, "total_ms": v["total_ns"] / 1e6} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_rate.json"))
    a = ap.parse_args()

    poses = [S.pose(POSE_SEED, f) for f in range(a.frames)]
    g = hfpf.OccupancyGrid(resolution=0.001, bbox=BBOX, fuse_color=True, max_bricks=400000, max_log_points=a.frames * W * H,
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
    rows = g.extract().copy()
    dims, res = g.dims
    cubes = mesh_ref.cube_set(rows, dims)
    out = {"what": "hfpf_extract_mesh* of a 1 mm model of %d synthetic 640x480 depth frames" % a.frames, "rows": int(len(rows)),
           "cubes": int(len(cubes)), "corners": int(len(mesh_ref.corner_set(cubes))), "reps": a.reps,
           "stat": "[median ms, min ms] per call"}
    del cubes
    out["extract_ms"] = timed(lambda: g.extract(), a.reps)
    log("extract: %s ms (%d rows)" % (out["extract_ms"], len(rows)))

    def device(r):
        dv, nv, dt, nt = g.extract_mesh_device(radius=r)
        return dv, dt

    for r in RADII:
        v, t = g.extract_mesh(radius=r)
        e = {"vertices": int(len(v)), "triangles": int(len(t))}
        del v, t
        e["host_ms"] = timed(lambda: g.extract_mesh(radius=r), a.reps)
        ts = []
        for i in range(a.reps + 1):
            t0 = time.perf_counter()
            dv, dt = device(r)
            ms = (time.perf_counter() - t0) * 1e3
            g.device_free(dv)
            g.device_free(dt)
            if i:
                ts.append(ms)
        e["device_ms"] = (float(np.median(ts)), float(min(ts)))
        out["radius%d" % r] = e
        log("radius %d: %s" % (r, e))
    out["device_bytes"] = int(g.counters()["device_bytes"])
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
