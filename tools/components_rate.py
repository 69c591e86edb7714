#!/usr/bin/env python3
"""Connected-component rates on a full-size model: a 1 mm session of 120 synthetic 640x480 depth + colour frames (1 m^3, colour fusion
on, a clean pass every 30 frames; the model tools/mesh_rate.py builds), then the model labelled in two forms:

  host     hfpf_extract_components: rows, labels and component records downloaded to pageable host arrays
  device   hfpf_extract_components_device: the same left in fresh HBM arrays (freed after each call, outside the timing)
  ... at reach 1 and 2, without (min_normal_dot = -2) and with (0.9) the normal gate, every keep test off; one more case with the
  keep tests on (min_rows, keep_largest); and hfpf_extract on the same model (what a user calls today before a CPU labelling).

Every call returns when its outputs are complete, so wall time around the call is the call's time.  Median and min of --reps calls
after one warm-up call.  kernels_ms is the engine's own event timing of the component kernels of a call (hfpf_get_kernel_time id 6:
index to compaction, without the row set and the copies), the mean over the timed host and device calls of the case.

usage: python3 tools/components_rate.py [--frames 120] [--reps 7] [--out profiles/components_rate.json]
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
CASES = [("reach1", dict(reach=1)), ("reach1_dot0.9", dict(reach=1, min_normal_dot=0.9)), ("reach2", dict(reach=2)),
         ("reach2_dot0.9", dict(reach=2, min_normal_dot=0.9)), ("reach1_min_rows100_keep8", dict(reach=1, min_rows=100, keep_largest=8))]
LINK_KERNEL = "row order (one lane per row in lexicographic order, union-find in HBM)"


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_rate.json"))
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
    n_rows = len(g.extract())
    out = {"what": "hfpf_extract_components* of a 1 mm model of %d synthetic 640x480 depth frames" % a.frames, "rows": int(n_rows),
           "reps": a.reps, "stat": "[median ms, min ms] per call", "link_kernel": LINK_KERNEL}
    out["extract_ms"] = timed(lambda: g.extract(), a.reps)
    log("extract: %s ms (%d rows)" % (out["extract_ms"], n_rows))

    def free(r):
        for p in (r[0], r[1], r[3]):
            if p:
                g.device_free(p)

    for name, kw in CASES:
        rows, labels, comps = g.extract_components(**kw)
        e = {"opts": kw, "rows_kept": int(len(rows)), "components": int(len(comps)),
             "largest": int(comps["n_rows"].max()) if len(comps) else 0}
        del rows, labels, comps
        g.kernel_timing(1)
        e["host_ms"] = timed(lambda: g.extract_components(**kw), a.reps)
        e["host_labels_only_ms"] = timed(lambda: g.extract_components(rows=False, **kw), a.reps)
        e["device_ms"] = timed(lambda: g.extract_components(device=True, **kw), a.reps, free)
        ms, n = g.kernel_time(6)
        g.kernel_timing(0)
        e["kernels_ms"] = ms / max(n, 1)
        e["rows_per_s_host"] = n_rows / (e["host_ms"][0] * 1e-3)
        e["rows_per_s_device"] = n_rows / (e["device_ms"][0] * 1e-3)
        out[name] = e
        log("%s: %s" % (name, e))
    out["device_bytes"] = int(g.counters()["device_bytes"])
    g.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
