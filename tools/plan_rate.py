#!/usr/bin/env python3
"""View-planning rates on a full-size model: the 1 mm session of 120 synthetic 640x480 depth + colour frames tools/cover_rate.py
builds, then hfpf_plan_views_device of the model's own mesh (read in place from HBM, spacing one voxel, window 2 voxels, max_distance
2 voxels) for 16, 64 and 256 candidate 640x480 views on three rings around the scene, with two calls of the same session beside each
case: hfpf_cover_mesh_device with the same cover options, and hfpf_render_device (depth plane, radius 0) of as many views.  Every call
returns when its outputs are complete, so wall time around the call is the call's time.  Median and min of --reps calls after one
warm-up call.  The plan's figures (targets, reachable, planned, selected) are recorded too.

With --parent TREE (a built checkout of the parent commit) tools/cover_rate.py is run in child processes, alternating this tree and
the parent's, --rounds times each: the JSON holds both sets of hfpf_cover_mesh_device figures and the spread of the parent's own
repeated runs, inside which this tree's must lie.

usage: python3 tools/plan_rate.py [--frames 120] [--resolution 0.001] [--reps 3] [--parent TREE [--rounds 2]] [--out profiles/plan_rate.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "high-fidelity-pointcloud-fusion_amd", "python"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import hfpf  # noqa: E402
import hfpf_synth as S  # noqa: E402

W, H = 640, 480
K = (525.0, 525.0, 319.5, 239.5)
BBOX = (-0.5, 0.5, -0.5, 0.5, 0.0, 1.0)
SEED, POSE_SEED = 0xD3F7, 0x5E3
LOOK_AT = np.array([0.0, 0.0, 0.47])


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


def look_at(eye, target=LOOK_AT):
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    return np.hstack([np.stack([x, np.cross(z, x), z], axis=1), eye.reshape(3, 1)])


def candidates(n):
    """n poses on three rings (radius 0.45 m, at y = -0.2, 0 and 0.2 m) around the scene, all looking at its middle."""
    out = []
    for i in range(n):
        t = 2 * np.pi * (i // 3) / ((n + 2) // 3)
        out.append(look_at(LOOK_AT + np.array([0.45 * np.sin(t), 0.2 * (i % 3 - 1), -0.45 * np.cos(t)])))
    return np.stack(out)


def cover_runs(tree, frames, resolution, reps):
    """tools/cover_rate.py of `tree` in a child process: its device_ms at a spacing of one voxel."""
    with tempfile.NamedTemporaryFile(suffix=".json") as f:
        subprocess.check_call([sys.executable, os.path.join(tree, "tools", "cover_rate.py"), "--frames", str(frames), "--resolution", str(resolution),
                               "--reps", str(reps), "--out", f.name], stdout=subprocess.DEVNULL, cwd=tree)
        return json.load(open(f.name))["spacing_1_voxels"]["device_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--resolution", type=float, default=0.001)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_rate.json"))
    a = ap.parse_args()

    poses = [S.pose(POSE_SEED, f) for f in range(a.frames)]
    g = hfpf.OccupancyGrid(resolution=a.resolution, bbox=BBOX, fuse_color=True, max_bricks=400000, max_log_points=a.frames * W * H,
                           max_normals=24 << 20, max_frames=4096, frame_width=W)
    t0 = time.perf_counter()
    for f in range(a.frames):
        depth, rgb, Kf = S.depth_frame(SEED, f, W, H, poses[f])
        g.integrate_depth(depth, poses[f], Kf, color=rgb)
        if (f + 1) % 30 == 0:
            g.clean()
    g.clean()
    g.sync()
    log("session: %d frames in %.1f s" % (a.frames, time.perf_counter() - t0))
    n_rows = len(g.extract())
    dv, nv, dt, nt = g.extract_mesh_device()
    out = {"what": "hfpf_plan_views_device of the own mesh of a %g m model of %d synthetic 640x480 depth frames" % (a.resolution, a.frames),
           "rows": int(n_rows), "vertices": int(nv), "triangles": int(nt), "reps": a.reps, "stat": "[median ms, min ms] per call"}
    ident = np.eye(4)[:3]
    res = a.resolution
    cover = dict(radius=2, max_distance=2 * res, spacing=res)
    mesh = dict(device=True, n_verts=nv, vertex_stride=32, n_tris=nt)
    free = lambda r: g.device_free(r[-2]) if r[-2] else None  # noqa: E731  (records pointer, summary)
    out["cover_mesh_device_ms"] = timed(lambda: g.cover_mesh(dv, dt, ident, **mesh, **cover), a.reps, free)
    plan = dict(cover, z_range=(0.3, 3.0), splat_radius=-1, max_splat_radius=4, occluder_near=0.01, min_cos=0.2, tolerance=2 * res, max_views=8)
    for n in (16, 64, 256):
        cand = candidates(n)
        scores, ptr, s = g.plan_views(dv, dt, cand, ident, K=K, width=W, height=H, **mesh, **plan)
        if ptr:
            g.device_free(ptr)
        e = {"summary": {k: s[k] for k in s if k != "coverage"}, "samples": s["coverage"]["n_samples"],
             "selected_views": [int(v) for v in np.argsort(np.where(scores["rank"] < 0, 1 << 30, scores["rank"]))[:s["n_selected"]]]}
        e["plan_views_device_ms"] = timed(lambda: g.plan_views(dv, dt, cand, ident, K=K, width=W, height=H, **mesh, **plan), a.reps, free)
        e["plan_views_device_without_records_ms"] = timed(
            lambda: g.plan_views(dv, dt, cand, ident, K=K, width=W, height=H, tri_plan=False, **mesh, **plan), a.reps)
        e["plan_views_device_model_occludes_ms"] = timed(
            lambda: g.plan_views(dv, dt, cand, ident, K=K, width=W, height=H, tri_plan=False, model_occludes=True, **mesh, **plan), a.reps)
        dd = g.device_alloc(n * W * H * 4)
        try:
            e["render_device_depth_ms"] = timed(lambda: g.render_device(cand, K, W, H, {"depth": dd}, z_range=(0.3, 3.0)), a.reps)
        finally:
            g.device_free(dd)
        out["views_%d" % n] = e
        log("%d views: %s" % (n, e))
    g.device_free(dv), g.device_free(dt)
    out["device_bytes"] = int(g.counters()["device_bytes"])
    g.close()
    if a.parent:
        runs = {"this": [], "parent": []}
        for _ in range(a.rounds):
            for name, tree in (("parent", os.path.abspath(a.parent)), ("this", ROOT)):
                runs[name].append(cover_runs(tree, a.frames, a.resolution, a.reps))
                log("cover_rate.py, %s: %r" % (name, runs[name][-1]))
        med = {k: [r[0] for r in v] for k, v in runs.items()}
        out["cover_rate_against_parent"] = dict(
            what="tools/cover_rate.py, hfpf_cover_mesh_device at a spacing of one voxel, [median ms, min ms] per run, runs alternating",
            this=runs["this"], parent=runs["parent"], parent_spread_ms=[min(med["parent"]), max(med["parent"])],
            this_inside_parent_spread=bool(min(med["parent"]) <= min(med["this"]) and max(med["this"]) <= max(med["parent"])),
            this_not_above_parent_spread=bool(max(med["this"]) <= max(med["parent"])))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
