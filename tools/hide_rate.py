#!/usr/bin/env python3
"""Hidden-row rates on a full-size model: the 1 mm session of 120 synthetic 640x480 depth + colour frames the other rate tools
build, then

  hide_device_list   hfpf_hide_voxels_device of ALL rows (an hfpf_row array in HBM, stride 64) with a selector word per row that
                     selects every tenth (HFPF_HIDE; hfpf_show_all between the calls, outside the timed window)
  hide_box           hfpf_hide_box of the middle third of the rows' x range
  get_hidden         hfpf_get_hidden with 10 % of the rows hidden
  read-outs          hfpf_extract, hfpf_query_device (the rows' own centroids, radius 1), hfpf_raycast_view_device (one 640x480 view) and
                     hfpf_extract_mesh_device (radius 2), with H empty and with 10 % of the rows hidden

The guard that matters is that H empty costs nothing.  With --parent TREE (a built checkout of the parent commit) the four read-outs
with H empty are measured in child processes of this tool, alternating this tree and the parent's, --rounds times each: the JSON holds
both sets of numbers and the spread the parent's own repeated runs show.  --bench-steps K also runs `bench.py --gpus 1 --steps K
--warmup W` in both trees the same way and records the headline values.  Every call returns when its outputs are complete, so wall
time around the call is the call's time.  Median and min of --reps calls after one warm-up call.

usage: python3 tools/hide_rate.py [--frames 120] [--reps 5] [--parent TREE [--rounds 2] [--bench-steps 4 --bench-warmup 2]]
                                  [--out profiles/hide_rate.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 640, 480
BBOX = (-0.5, 0.5, -0.5, 0.5, 0.0, 1.0)
SEED, POSE_SEED = 0xD3F7, 0x5E3


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(fn, reps, after=lambda r: None, before=lambda: None):
    import numpy as np
    ts = []
    for i in range(reps + 1):  # the first call warms up
        before()
        t0 = time.perf_counter()
        r = fn()
        ms = (time.perf_counter() - t0) * 1e3
        after(r)
        if i:
            ts.append(ms)
    return [float(np.median(ts)), float(min(ts))]


def session(tree, frames):
    """(hfpf module, grid, rows, K, poses) of the model, with the binding and the library of `tree`."""
    for p in (os.path.join(tree, "high-fidelity-pointcloud-fusion_amd", "python"), os.path.join(tree, "tests")):
        sys.path.insert(0, p)
    import numpy as np
    import hfpf
    import hfpf_synth as S
    poses = np.stack([S.pose(POSE_SEED, f) for f in range(frames)])
    g = hfpf.OccupancyGrid(resolution=0.001, bbox=BBOX, fuse_color=True, max_bricks=400000, max_log_points=frames * W * H, max_normals=24 << 20,
                           max_frames=4096, frame_width=W)
    K = None
    t0 = time.perf_counter()
    for f in range(frames):
        depth, rgb, K = S.depth_frame(SEED, f, W, H, poses[f])
        g.integrate_depth(depth, poses[f], K, color=rgb)
        if (f + 1) % 30 == 0:
            g.clean()
    g.clean()
    g.sync()
    log("session: %d frames in %.1f s" % (frames, time.perf_counter() - t0))
    return hfpf, g, g.extract().copy(), K, poses


def readouts(hfpf, g, rows, K, poses, reps):
    """[median ms, min ms] of the four read-outs on g as it stands."""
    import numpy as np
    pts = np.ascontiguousarray(np.stack([rows["x"], rows["y"], rows["z"]], axis=1))
    d_pts = g.device_alloc(pts.nbytes)
    g.device_upload(d_pts, pts)
    d_hits, d_rows = g.device_alloc(len(pts) * 64), g.device_alloc(len(pts) * 64)
    d_view = g.device_alloc(W * H * 64)
    ident = np.eye(4)[:3]

    def free_mesh(r):
        for p in (r[0], r[2]):
            if p:
                g.device_free(p)

    out = {"extract_ms": timed(lambda: g.extract(), reps),
           "query_device_ms": timed(lambda: g.query_device(d_pts, len(pts), ident, dev_hits=d_hits, dev_rows=d_rows, radius=1), reps),
           "raycast_view_device_ms": timed(lambda: g.raycast_views_device(poses[:1], K, W, H, dev_hits=d_view, radius=2, step=0.5, t_range=(0.05, 3.0)), reps),
           "extract_mesh_device_ms": timed(lambda: g.extract_mesh_device(radius=2), reps, free_mesh)}
    for p in (d_pts, d_hits, d_rows, d_view):
        g.device_free(p)
    return out


def child(tree, frames, reps):
    """The four read-outs with nothing hidden, with the binding and library of `tree`: one JSON line on stdout."""
    hfpf, g, rows, K, poses = session(tree, frames)
    out = readouts(hfpf, g, rows, K, poses, reps)
    out["rows"] = int(len(rows))
    g.close()
    print(json.dumps(out))


def run_child(tree, frames, reps):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, "--frames", str(frames), "--reps", str(reps)], stdout=subprocess.PIPE, text=True,
                       check=True, timeout=900)
    return json.loads(r.stdout.strip().splitlines()[-1])


def run_bench(tree, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], stdout=subprocess.PIPE,
                       text=True, check=True, timeout=1500, cwd=tree)
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return {k: line[k] for k in ("value", "unit") if k in line}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--bench-steps", type=int, default=0)
    ap.add_argument("--bench-warmup", type=int, default=2)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "hide_rate.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.frames, a.reps)
    if a.parent:
        a.parent = os.path.abspath(a.parent)

    import numpy as np
    hfpf, g, rows, K, poses = session(HERE, a.frames)
    n = len(rows)
    out = {"what": "hfpf_hide_* on a 1 mm model of %d synthetic 640x480 depth frames" % a.frames, "rows": int(n), "image": [W, H], "reps": a.reps,
           "stat": "[median ms, min ms] per call"}
    out["H_empty"] = readouts(hfpf, g, rows, K, poses, a.reps)
    log("H empty: %s" % out["H_empty"])

    words = (np.arange(n) % 10 == 0).astype(np.uint32)
    d_rows, d_words = g.device_alloc(rows.nbytes), g.device_alloc(words.nbytes)
    g.device_upload(d_rows, rows), g.device_upload(d_words, words)
    hide = lambda: g.hide_voxels(d_rows, "hide", select=d_words, select_mask=1, select_value=1, device=True, n=n, voxel_stride=64, select_stride=4)
    out["hide_device_list_ms"] = timed(hide, a.reps, before=g.show_all)
    x0, x1 = int(rows["ix"].min()), int(rows["ix"].max())
    third = (x1 - x0 + 1) // 3
    big = 2 ** 31 - 1
    out["hide_box_ms"] = timed(lambda: g.hide_box((x0 + third, -big, -big), (x0 + 2 * third - 1, big, big)), a.reps, before=g.show_all)
    g.show_all()
    out["hidden_10_percent"] = dict(counts=hide())
    out["get_hidden_ms"] = timed(lambda: g.hidden(), a.reps)
    out["hidden_10_percent"].update(readouts(hfpf, g, rows, K, poses, a.reps))
    log("10 %% hidden: %s" % out["hidden_10_percent"])
    g.show_all()
    g.device_free(d_rows), g.device_free(d_words)
    out["device_bytes"] = int(g.counters()["device_bytes"])
    g.close()

    if a.parent:
        runs = {"this": [], "parent": []}
        for _ in range(a.rounds):  # alternating: other people's work shares the host
            for name, tree in (("parent", a.parent), ("this", HERE)):
                runs[name].append(run_child(tree, a.frames, a.reps))
                log("%s: %s" % (name, runs[name][-1]))
        keys = ("extract_ms", "query_device_ms", "raycast_view_device_ms", "extract_mesh_device_ms")
        med = lambda name, k: [r[k][0] for r in runs[name]]
        out["against_parent"] = {k: dict(this_median_ms=med("this", k), parent_median_ms=med("parent", k),
                                         parent_spread_ms=max(med("parent", k)) - min(med("parent", k))) for k in keys}
        if a.bench_steps:
            bench = {"this": [], "parent": []}
            for _ in range(a.rounds):
                for name, tree in (("parent", a.parent), ("this", HERE)):
                    bench[name].append(run_bench(tree, a.bench_steps, a.bench_warmup))
                    log("bench %s: %s" % (name, bench[name][-1]))
            out["bench_against_parent"] = dict(command="bench.py --gpus 1 --steps %d --warmup %d" % (a.bench_steps, a.bench_warmup), **bench)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
