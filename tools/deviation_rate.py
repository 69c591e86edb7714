#!/usr/bin/env python3
"""Deviation rates on a full-size model: a 1 mm session of 120 synthetic 640x480 depth + colour frames (1 m^3, colour fusion on, a
clean pass every 30 frames; the model tools/mesh_rate.py builds), then the model measured against its own mesh in two forms:

  host     hfpf_compare_mesh: the mesh uploaded from pageable host arrays, the records downloaded
  device   hfpf_compare_mesh_device: the mesh of hfpf_extract_mesh_device read in place, the records left in a fresh HBM array

at max_distance = 3 and 20 voxels, with hfpf_extract and hfpf_extract_mesh_device of the same session beside them.  Every call
returns when its outputs are complete, so wall time around the call is the call's time.  Median and min of --reps calls after one
warm-up call.  kernels_ms is the engine's own event timing of the compare kernels of a call (hfpf_get_kernel_time id 7: binning to the
row kernel, without the row set and the copies), the mean over the timed calls of the case.  The fidelity figures (n_found / n_rows,
RMS from sum_sq_q30, max_abs) of each case are recorded too.

usage: python3 tools/deviation_rate.py [--frames 120] [--resolution 0.001] [--reps 5] [--out profiles/deviation_rate.json]
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
    ts = []
    for i in range(reps + 1):  # the first call warms up
        t0 = time.perf_counter()
        r = fn()
        ms = (time.perf_counter() - t0) * 1e3
        after(r)
        if i:
            ts.append(ms)
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--resolution", type=float, default=0.001)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deviation_rate.json"))
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
    verts, tris = g.extract_mesh()
    out = {"what": "hfpf_compare_mesh* of a %g m model of %d synthetic 640x480 depth frames against its own mesh" % (a.resolution, a.frames),
           "rows": int(n_rows), "vertices": int(len(verts)), "triangles": int(len(tris)), "reps": a.reps, "stat": "[median ms, min ms] per call"}
    out["extract_ms"] = timed(lambda: g.extract(), a.reps)

    def free_mesh(r):
        g.device_free(r[0]), g.device_free(r[2])

    out["extract_mesh_device_ms"] = timed(lambda: g.extract_mesh_device(), a.reps, free_mesh)
    dv, nv, dt, nt = g.extract_mesh_device()

    def free(r):
        for p in (r[0], r[1]):
            if p:
                g.device_free(p)

    ident = np.eye(4)[:3]
    for voxels in (3, 20):
        md = voxels * a.resolution
        dev, s = g.compare_mesh(verts, tris, ident, max_distance=md)
        e = {"max_distance": md, "summary": s, "found_fraction": s["n_found"] / max(1, s["n_rows"]),
             "rms": float((s["sum_sq_q30"] / 2.0 ** 30 / max(1, s["n_found"])) ** 0.5),
             "mean_abs": float(s["sum_abs_q30"] / 2.0 ** 30 / max(1, s["n_found"]))}
        del dev
        g.kernel_timing(1)
        e["host_ms"] = timed(lambda: g.compare_mesh(verts, tris, ident, max_distance=md), a.reps)
        e["device_ms"] = timed(lambda: g.compare_mesh(dv, dt, ident, device=True, n_verts=nv, vertex_stride=32, n_tris=nt, max_distance=md), a.reps, free)
        ms, n = g.kernel_time(7)
        g.kernel_timing(0)
        e["kernels_ms"] = ms / max(n, 1)
        e["rows_per_s_device"] = n_rows / (e["device_ms"][0] * 1e-3)
        out["voxels_%d" % voxels] = e
        log("%d voxels: %s" % (voxels, e))
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
