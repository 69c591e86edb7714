#!/usr/bin/env python3
"""Render rates on a full-size model: a 1 mm session of 120 synthetic 640x480 depth + colour frames (1 m^3, colour fusion on,
a clean pass every 30 frames), then, one measurement at a time on the engine's stream:

  rowset   a 1x1 render: the row set (k_extract_keys -> sort -> k_extract_rows) plus one tiny splat and resolve
  device   hfpf_render_device of 1, 16 and 64 views at 640x480 into device planes (all five planes), radius 0 and auto (max 4)
  host     hfpf_render of one 640x480 view into pageable numpy planes (all five planes), radius 0 and auto

Every call returns when its planes are complete, so wall time around the call is the call's time.  Median of --reps calls after
one warm-up call.

usage: python3 tools/render_rate.py [--frames 120] [--reps 7] [--out profiles/render_rate.json]
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
Z_RANGE = (0.05, 3.0)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_rate.json"))
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
    rows = g.extract()
    n_rows = int(len(rows))
    n_drawable = int((rows["count"] > 0).sum())
    del rows
    log("rows %d (count > 0: %d)" % (n_rows, n_drawable))

    out = {"what": "hfpf_render / hfpf_render_device on a 1 mm model of %d synthetic 640x480 depth frames" % a.frames,
           "rows": n_rows, "rows_drawable": n_drawable, "image": [W, H], "reps": a.reps, "stat": "median ms (min ms) per call"}

    med, mn = timed(lambda: g.render(poses[0], K, 1, 1, planes=("depth",), z_range=Z_RANGE), a.reps)
    out["rowset_ms"] = {"median": med, "min": mn, "note": "a 1x1 single-plane render: row set build + one splat/resolve of 1 pixel"}
    log("rowset %.3f ms" % med)

    n_max = 64
    WH = W * H
    planes = {"depth": 4, "normal": 12, "rgb": 4, "count": 4, "voxel": 12}
    ptrs = {p: g.device_alloc(n_max * WH * b) for p, b in planes.items()}
    view_poses = np.stack([poses[(7 * i) % a.frames] for i in range(n_max)])
    dev = {}
    for label, kw in (("radius0", dict(splat_radius=0)), ("auto", dict(splat_radius=-1, max_splat_radius=4))):
        for n in (1, 16, 64):
            med, mn = timed(lambda: g.render_device(view_poses[:n], K, W, H, ptrs, z_range=Z_RANGE, **kw), a.reps)
            dev["%s_n%d" % (label, n)] = {"call_ms": med, "call_min_ms": mn, "ms_per_view": med / n,
                                         "ms_per_view_after_rowset": (med - out["rowset_ms"]["median"]) / n}
            log("device %s n=%d: %.3f ms/call, %.3f ms/view" % (label, n, med, med / n))
    for p in ptrs.values():
        g.device_free(p)
    out["device"] = dev

    host = {}
    for label, kw in (("radius0", dict(splat_radius=0)), ("auto", dict(splat_radius=-1, max_splat_radius=4))):
        med, mn = timed(lambda: g.render(poses[0], K, W, H, z_range=Z_RANGE, **kw), a.reps)
        host[label] = {"call_ms": med, "call_min_ms": mn}
        log("host %s: %.3f ms" % (label, med))
    out["host"] = host
    img = g.render(poses[0], K, W, H, z_range=Z_RANGE, splat_radius=-1, max_splat_radius=4)
    out["coverage_pose0_auto"] = float((~np.isnan(img["depth"])).mean())
    g.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
