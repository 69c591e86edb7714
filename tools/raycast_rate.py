#!/usr/bin/env python3
"""Raycast rates on a full-size model: the 1 mm session of 120 synthetic 640x480 depth + colour frames tools/query_rate.py builds,
then the 640x480 view of the held-out frame's pose:

  raycast        hfpf_raycast_view_device into HBM at radius 1, 2 and 4, step 0.5
  kernel         k_raycast_view alone (hfpf_get_kernel_time id 5, HIP events on the engine's stream)
  naive          the same contract without skipping: hfpf_query_device over ALL n samples of --naive-rays randomly chosen rays of
                 the view (points resident in HBM, hits left in HBM), scaled to the whole view by width * height / --naive-rays
  render         hfpf_render of the same view (depth plane, splat radius 0 and 2)
  mesh           hfpf_extract_mesh_device of the same model

and, for the view at an INTEGRATED frame's pose, t against that frame's depth image and the count of valid pixels against hfpf_render
at splat radius 0.  Every call returns when its outputs are complete, so wall time around the call is the call's time.  Median of
--reps calls after one warm-up call.  Kernel times of a separate run under `rocprofv3 --kernel-trace --stats` are copied in with
--kernel-stats.

usage: python3 tools/raycast_rate.py [--frames 120] [--reps 7] [--naive-rays 4096] [--kernel-stats stats.csv] [--out profiles/raycast_rate.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "high-fidelity-pointcloud-fusion_amd", "python"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import hfpf  # noqa: E402
import hfpf_synth as S  # noqa: E402
import raycast_ref as RC  # noqa: E402
from query_rate import BBOX, H, HELD_OUT, POSE_SEED, SEED, W, log, timed  # noqa: E402
import query_rate  # noqa: E402

Z = (0.25, 0.65)
STEP = 0.5
RADII = (1, 2, 4)
SEEN = 60  # the integrated frame whose pose and depth image the agreement figures use


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--naive-rays", type=int, default=4096)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast_rate.json"))
    a = ap.parse_args()

    poses = [S.pose(POSE_SEED, f) for f in range(a.frames)]
    g = hfpf.OccupancyGrid(resolution=0.001, bbox=BBOX, fuse_color=True, max_bricks=400000, max_log_points=a.frames * W * H,
                           max_normals=24 << 20, max_frames=4096, frame_width=W)
    K = None
    seen_depth = None
    for f in range(a.frames):
        depth, rgb, K = S.depth_frame(SEED, f, W, H, poses[f])
        if f == min(SEEN, a.frames - 1):
            seen_depth, seen_pose = depth.copy(), poses[f]
        g.integrate_depth(depth, poses[f], K, color=rgb)
        if (f + 1) % 30 == 0:
            g.clean()
    g.clean()
    g.sync()
    n_rows = int(len(g.extract()))
    res = g.dims[1]
    pose = np.asarray(S.pose(POSE_SEED, HELD_OUT), np.float64).reshape(3, 4)
    n = RC.n_samples(Z[0], Z[1], STEP, res)
    out = {"what": "hfpf_raycast_view_device of the %dx%d view at a held-out pose on a 1 mm model of %d synthetic depth frames, z %g..%g m, "
                   "step %g voxels (%d samples a ray)" % (W, H, a.frames, Z[0], Z[1], STEP, n),
           "rows": n_rows, "image": [W, H], "reps": a.reps, "stat": "median ms (min ms) per call", "samples_per_ray": n}
    dev_hits = g.device_alloc(W * H * 64)
    O, D, _ = RC.view_rays(pose, K, W, H)
    pick = np.sort(np.random.default_rng(0xACE).choice(W * H, a.naive_rays, replace=False))
    tk = Z[0] + np.arange(n, dtype=np.float64) * (STEP * res)
    pts = np.ascontiguousarray((O[pick][:, None, :] + tk[None, :, None] * D[pick][:, None, :]).astype(np.float32).reshape(-1, 3))
    dev_pts = g.device_alloc(pts.nbytes)
    dev_qhits = g.device_alloc(len(pts) * 64)
    g.device_upload(dev_pts, pts)
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    for r in RADII:
        kw = dict(radius=r, step=STEP, t_range=Z)
        hits = g.raycast_view(pose, K, W, H, **kw)
        fl = hits["flags"]
        e = {"hit": int((fl & hfpf.RAY_HIT != 0).sum()), "near_without_hit": int(((fl & hfpf.RAY_NEAR != 0) & (fl & hfpf.RAY_HIT == 0)).sum())}
        e["raycast_view_device"] = timed(lambda: g.raycast_views_device([pose], K, W, H, dev_hits=dev_hits, **kw), a.reps)
        g.kernel_timing(1)
        for _ in range(a.reps):
            g.raycast_views_device([pose], K, W, H, dev_hits=dev_hits, **kw)
        ms, launches = g.kernel_time(5)
        g.kernel_timing(0)
        e["k_raycast_view_mean_ms"] = ms / max(1, launches)
        med, mn = timed(lambda: g.query_device(dev_pts, len(pts), ident, dev_hits=dev_qhits, dev_rows=0, radius=r), a.reps)
        scale = W * H / float(a.naive_rays)
        e["naive_query_device_subset"] = (med, mn)
        e["naive_query_device_scaled_to_view"] = (med * scale, mn * scale)
        e["naive_rays"], e["naive_points"] = a.naive_rays, len(pts)
        e["speedup_over_naive"] = med * scale / e["raycast_view_device"][0]
        out["radius%d" % r] = e
        log("radius %d: %s" % (r, e))
    for sr in (0, 2):
        out["render_depth_splat%d" % sr] = timed(lambda: g.render(pose, K, W, H, planes=("depth",), z_range=Z, splat_radius=sr), a.reps)

    def mesh():
        v, nv, t, nt = g.extract_mesh_device(radius=2)
        for p in (v, t):
            if p:
                g.device_free(p)
        return nv, nt

    out["mesh_counts"] = list(mesh())
    out["extract_mesh_device"] = timed(mesh, a.reps)
    # agreement with the sensor: the view at an integrated frame's pose against that frame's depth image
    K_seen = K
    hv = g.raycast_view(seen_pose, K_seen, W, H, radius=2, step=STEP, t_range=Z)
    valid_ray = hv["flags"] & hfpf.RAY_HIT != 0
    sensor = seen_depth.astype(np.float64) * 0.001
    both = valid_ray & (seen_depth != 0)
    d = (hv["t"].astype(np.float64) - sensor)[both]
    img = g.render(seen_pose, K_seen, W, H, planes=("depth",), z_range=Z, splat_radius=0)["depth"]
    out["agreement"] = {"frame": min(SEEN, a.frames - 1), "sensor_valid": int((seen_depth != 0).sum()), "raycast_valid": int(valid_ray.sum()),
                        "both_valid": int(both.sum()), "render_splat0_valid": int(np.isfinite(img).sum()),
                        "t_minus_depth_m": {"mean": float(d.mean()), "std": float(d.std()),
                                            "percentiles_1_5_25_50_75_95_99": [float(x) for x in np.percentile(d, [1, 5, 25, 50, 75, 95, 99])],
                                            "abs_le_1mm": float((np.abs(d) <= 0.001).mean()), "abs_le_2mm": float((np.abs(d) <= 0.002).mean())}}
    log("agreement: %s" % out["agreement"])
    for p in (dev_hits, dev_pts, dev_qhits):
        g.device_free(p)
    g.close()
    if a.kernel_stats:
        query_rate.KERNELS = ("k_raycast_view", "k_raycast", "k_ray_map_bricks", "k_ray_map_dilate", "k_ray_map_up", "k_query")
        out["kernels"] = query_rate.kernel_stats(a.kernel_stats)
        out["kernels_note"] = "from a separate run of this tool under rocprofv3 --kernel-trace --stats (all of its calls)"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
