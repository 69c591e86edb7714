#!/usr/bin/env python3
"""Coverage rates on a full-size model: the 1 mm session of 120 synthetic 640x480 depth + colour frames tools/deviation_rate.py builds,
then how much of the model's own mesh the model covers, in two forms:

  host     hfpf_cover_mesh: the mesh uploaded from pageable host arrays, the records downloaded
  device   hfpf_cover_mesh_device: the mesh of hfpf_extract_mesh_device read in place, the records left in a fresh HBM array

at spacing = 1 and 4 voxels (window 2 voxels, max_distance 2 voxels, gate off), with two calls of the same session beside each case:
hfpf_compare_mesh_device at max_distance = 3 voxels, and hfpf_query_device (hits only, the same window and max_distance) of as many
points as the cover has samples, the mesh's vertices repeated to that count.  Every call returns when its outputs are complete, so
wall time around the call is the call's time: a cover has no kernel timing id.  Median and min of --reps calls after one warm-up call.
The coverage figures of each case (samples, covered share of samples and of area) are recorded too.

usage: python3 tools/cover_rate.py [--frames 120] [--resolution 0.001] [--reps 5] [--out profiles/cover_rate.json]
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
    return [float(np.median(ts)), float(min(ts))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--resolution", type=float, default=0.001)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cover_rate.json"))
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
    out = {"what": "hfpf_cover_mesh* of the own mesh of a %g m model of %d synthetic 640x480 depth frames" % (a.resolution, a.frames),
           "rows": int(n_rows), "vertices": int(len(verts)), "triangles": int(len(tris)), "reps": a.reps, "stat": "[median ms, min ms] per call"}
    dv, nv, dt, nt = g.extract_mesh_device()
    ident = np.eye(4)[:3]
    res = a.resolution

    def free_compare(r):
        for p in (r[0], r[1]):
            if p:
                g.device_free(p)

    out["compare_mesh_device_3_voxels_ms"] = timed(
        lambda: g.compare_mesh(dv, dt, ident, device=True, n_verts=nv, vertex_stride=32, n_tris=nt, max_distance=3 * res), a.reps, free_compare)
    xyz = np.stack([verts["x"], verts["y"], verts["z"]], axis=1)
    for voxels in (1, 4):
        kw = dict(radius=2, max_distance=2 * res, spacing=voxels * res)
        cov, s = g.cover_mesh(verts, tris, ident, **kw)
        n = s["n_samples"]
        e = {"spacing": voxels * res, "summary": s, "covered_fraction_of_samples": s["n_covered"] / max(1, n),
             "covered_fraction_of_area": s["covered_area"] / s["area"] if s["area"] else 0.0,
             "mean_distance": float(s["sum_dist_q30"] / 2.0 ** 30 / max(1, s["n_covered"])),
             "triangles_subdivided": int((cov["n_samples"] > 1).sum())}
        del cov
        e["host_ms"] = timed(lambda: g.cover_mesh(verts, tris, ident, **kw), a.reps)
        e["device_ms"] = timed(lambda: g.cover_mesh(dv, dt, ident, device=True, n_verts=nv, vertex_stride=32, n_tris=nt, **kw), a.reps,
                               lambda r: g.device_free(r[0]) if r[0] else None)
        e["samples_per_s_device"] = n / (e["device_ms"][0] * 1e-3)
        pts = np.ascontiguousarray(np.resize(xyz, (n, 3)), np.float32)  # as many points as samples: the vertices, repeated
        dp, dh = g.device_alloc(pts.nbytes), g.device_alloc(n * hfpf.QUERY_HIT_DTYPE.itemsize)
        try:
            g.device_upload(dp, pts)
            e["query_device_hits_only_ms"] = timed(lambda: g.query_device(dp, n, ident, dev_hits=dh, dev_rows=0, radius=2, max_distance=2 * res), a.reps)
        finally:
            g.device_free(dp), g.device_free(dh)
        e["points_per_s_query_device"] = n / (e["query_device_hits_only_ms"][0] * 1e-3)
        out["spacing_%d_voxels" % voxels] = e
        log("spacing %d voxels: %s" % (voxels, e))
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
