#!/usr/bin/env python3
"""Topology rates on a full-size model: the 1 mm session of 120 synthetic 640x480 depth + colour frames tools/section_rate.py builds,
then hfpf_mesh_topology* of the model's own mesh, in two forms:

  device   hfpf_mesh_topology_device: the mesh of hfpf_extract_mesh_device read in place, the arrays left in fresh HBM arrays
  host     hfpf_mesh_topology: the mesh uploaded from pageable host arrays, the arrays downloaded

beside hfpf_extract_mesh_device and hfpf_section_mesh_device (64 parallel planes) of the same session.  Every call returns when its
outputs are complete, so wall time around the call is the call's time: the call has no kernel timing id.  Median and min of --reps
calls after one warm-up call.  The counts (edges, boundary edges, loops, shells) are recorded.  One more device call runs with
HFPF_TRACE_TOPOLOGY=1: the engine then prints its own wall time between the read-backs that end each stage, and the line is recorded
("stages_ms"; the traced call drains the stream twice more than an untraced one and is not among the timed ones).

With --parent (a built checkout of the parent commit) bench.py's headline is also run on both trees, --rounds alternating runs each
in this one session.

usage: python3 tools/topology_rate.py [--frames 120] [--resolution 0.001] [--reps 5] [--parent DIR [--bench-steps 4]] [--out profiles/topology_rate.json]
"""
import argparse
import json
import os
import re
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
BBOX = (-0.5, 0.5, -0.5, 0.5, 0.0, 1.0)
SEED, POSE_SEED = 0xD3F7, 0x5E3
STAGES = ("vertices_emit_shells", "sort", "run_walk_listed_scan", "loops", "allocation_reductions_finish")


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


def parallel(n):
    """n planes normal to x, evenly across the box."""
    p = np.zeros((n, 4))
    p[:, 0], p[:, 3] = 1.0, BBOX[0] + (BBOX[1] - BBOX[0]) * (np.arange(n) + 0.5) / n
    return p


def traced(fn):
    """fn() with HFPF_TRACE_TOPOLOGY=1 and the process's stderr in a file: (fn's result, the stage times the engine printed)."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["HFPF_TRACE_TOPOLOGY"] = "1"
        try:
            r = fn()
        finally:
            del os.environ["HFPF_TRACE_TOPOLOGY"]
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        text = tmp.read().decode()
    line = [x for x in text.splitlines() if x.startswith("hfpf: topology:")][-1]
    return r, dict(zip(STAGES, (float(v) for v in re.findall(r"([0-9.]+) ms", line))))


def run_bench(tree, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], stdout=subprocess.PIPE,
                       text=True, check=True, timeout=1500, cwd=tree)
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return {k: line[k] for k in ("value", "unit") if k in line}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--resolution", type=float, default=0.001)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--bench-steps", type=int, default=4)
    ap.add_argument("--bench-warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topology_rate.json"))
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
    out = {"what": "hfpf_mesh_topology* of the own mesh of a %g m model of %d synthetic 640x480 depth frames" % (a.resolution, a.frames),
           "rows": int(n_rows), "vertices": int(len(verts)), "triangles": int(len(tris)), "reps": a.reps, "stat": "[median ms, min ms] per call"}

    def free_mesh(r):
        for p in (r[0], r[2]):
            if p:
                g.device_free(p)

    def free_pairs(r):
        for x in r[:4]:
            p = x[0] if isinstance(x, tuple) else x
            if p:
                g.device_free(p)

    out["extract_mesh_device_ms"] = timed(lambda: g.extract_mesh_device(), a.reps, free_mesh)
    dv, nv, dt, nt = g.extract_mesh_device()
    ident = np.eye(4)[:3]
    planes = parallel(64)
    out["section_64_planes_device_ms"] = timed(lambda: g.section_mesh_device(dv, nv, 32, dt, nt, ident, planes), a.reps, lambda r: free_pairs(r[:3]))

    edges, loops, shells, tri_shell, s = g.mesh_topology(verts, tris)
    closed = (loops["flags"] & hfpf.TOPOLOGY_LOOP_CLOSED) != 0
    longest = np.argsort(loops["length_q32"])[::-1][:5]
    out["summary"] = s
    out["counts"] = {"edges": s["n_edges"], "boundary_edges": s["n_boundary"], "loops": s["n_loops"], "closed_loops": int(closed.sum()),
                     "shells": s["n_shells"], "largest_shell_triangles": int(shells["n_tris"].max()) if len(shells) else 0,
                     "longest_loops_m": [float(loops["length_q32"][i]) / 2.0 ** 32 for i in longest],
                     "longest_loops_edges": [int(loops["n_edges"][i]) for i in longest]}
    del edges, loops, shells, tri_shell
    out["device_ms"] = timed(lambda: g.mesh_topology_device(dv, nv, 32, dt, nt), a.reps, free_pairs)
    out["device_without_tri_shell_ms"] = timed(lambda: g.mesh_topology_device(dv, nv, 32, dt, nt, tri_shell=False), a.reps, free_pairs)
    out["host_ms"] = timed(lambda: g.mesh_topology(verts, tris), a.reps)
    r, out["stages_ms"] = traced(lambda: g.mesh_topology_device(dv, nv, 32, dt, nt))
    free_pairs(r)
    log("topology: %s" % {k: out[k] for k in ("counts", "device_ms", "host_ms", "stages_ms", "section_64_planes_device_ms", "extract_mesh_device_ms")})
    g.device_free(dv), g.device_free(dt)
    out["device_bytes"] = int(g.counters()["device_bytes"])
    g.close()

    if a.parent:
        parent = os.path.abspath(a.parent)
        bench = {"this": [], "parent": []}
        for _ in range(a.rounds):  # alternating: other people's work shares the host
            for name, tree in (("parent", parent), ("this", ROOT)):
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
