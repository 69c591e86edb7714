"""CPU: the pinhole view of csrc/view.hpp at the edges where the rule can go wrong, against its numpy restatements.
tests/view_check.cpp is a program of its own: it includes only that header, is built with -ffp-contract=off and the address and
undefined-behaviour sanitizers (their runtime linked into the executable) and run as an ordinary process in the environment as it
is.  It evaluates the header on the table of cases below and prints bit patterns; render_ref.project / auto_radius,
plan_ref.project and track_ref.associate say what they must be."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np

import hfpf
import plan_ref
import render_ref
import track_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "high-fidelity-pointcloud-fusion_amd", "csrc")

IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
P30 = 2.0 ** 30
BELOW_HALF = 0.49999999999999994  # the largest double below 0.5: u + 0.5 rounds up to 1
NAN, INF = float("nan"), float("inf")


def f32(v):
    return float(np.float32(v))


def rotated_pose():
    """A rotation about (1, 2, 3) by 0.7 rad (Rodrigues) and a translation: no entry of T is 0 or 1."""
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    R = np.eye(3) + np.sin(0.7) * K + (1.0 - np.cos(0.7)) * (K @ K)
    return tuple(np.concatenate([R, np.array([[0.3], [-0.2], [0.1]])], axis=1).reshape(12))


def case(p, pose=IDENTITY, K=(1.0, 1.0, 0.0, 0.0), z=(0.01, 100.0), size=(640, 480), radius=0, max_radius=4, res=0.0078125):
    return dict(p=tuple(f32(c) for c in p), pose=pose, K=K, z=z, size=size, radius=radius, max_radius=max_radius, res=res)


def cases():
    c = []
    # zc equal to z_near and to z_far (strict compares reject both) and their neighbours inside
    for z in ((0.5, 100.0), (np.nextafter(0.5, 0.0), 100.0), (0.01, 0.5), (0.01, np.nextafter(0.5, 1.0))):
        c.append(case((0.0, 0.0, 0.5), z=z))
    # u or v equal to +-2^30 (rejected) and the neighbour below in magnitude: 2^30 - 2^-22 is a double
    for s in (1.0, -1.0):
        for cxy in (0.0, -s * 2.0 ** -22):
            c.append(case((s * P30, 0.0, 1.0), K=(1.0, 1.0, cxy, 0.0)))
            c.append(case((0.0, s * P30, 1.0), K=(1.0, 1.0, 0.0, cxy)))
    # half-pixel ties u = k - 0.5, v = k - 0.5 for negative and positive k: floor(u + 0.5) takes them up
    for k in (-3, -1, 0, 1, 4, 640, 641):
        c.append(case((k - 0.5, 0.0, 1.0)))
        c.append(case((0.0, k - 0.5, 1.0)))
    c.append(case((0.0, 0.0, 1.0), K=(1.0, 1.0, BELOW_HALF, 0.0)))
    c.append(case((0.0, 0.0, 1.0), K=(1.0, 1.0, 0.0, BELOW_HALF)))
    # NaN and +-inf coordinates
    for bad in (NAN, INF, -INF):
        for axis in range(3):
            p = [0.25, -0.25, 1.0]
            p[axis] = bad
            c.append(case(p))
            c.append(case(p, pose=rotated_pose()))
    # a tiny zc (a subnormal: the camera 1e-310 m behind the point) drives u to inf
    behind = IDENTITY[:11] + (-1e-310,)
    c.append(case((1.0, 0.0, 0.0), pose=behind, z=(0.0, 100.0)))
    c.append(case((0.0, -1.0, 0.0), pose=behind, z=(1e-320, 100.0)))
    c.append(case((0.0, 0.0, 0.0), pose=behind, z=(0.0, 100.0)))  # ... and on the axis it is drawn, at pixel (0, 0)
    # a rotated pose: the column-wise indexing of T, and sums whose association shows in the last bit
    rng = np.random.default_rng(20)
    for p in rng.uniform(-1.0, 1.0, (96, 3)) * np.array([1.5, 1.5, 1.5]) + np.array([0.0, 0.0, 1.2]):
        c.append(case(p, pose=rotated_pose(), K=(525.0, 520.0, 319.5, 239.5), radius=-1, max_radius=6, res=0.01))
    # the association of each sum where it decides the pixel: (2^60 - 2^60) + 1 = 1, but 2^60 + (-2^60 + 1) = 0.  (T is no rotation
    # here; the rule is arithmetic and does not ask.)  xc = 1 -> pu = 8, yc = 1 -> pv = 8, zc = 1 or the row is not drawn at all
    big = (2.0 ** 60, -2.0 ** 60, 1.0)
    c.append(case(big, pose=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0), K=(8.0, 8.0, 0.0, 0.0)))
    c.append(case(big, pose=(0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0), K=(8.0, 8.0, 0.0, 0.0)))
    c.append(case(big, pose=(0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0), K=(8.0, 8.0, 0.0, 0.0)))
    # the image's borders through the inside test
    for x, y in ((-0.5, 0.0), (-0.51, 0.0), (639.49, 0.0), (639.5, 0.0), (0.0, -0.51), (0.0, 479.49), (0.0, 479.5)):
        c.append(case((x, y, 1.0)))
    # auto radius: r_num = (0.5 * 2^-7) * 512 = 2.  r_num / zc an exact integer, just below one, above max_radius, max_radius = 0
    for z, mr in ((0.5, 15), (np.nextafter(np.float32(0.5), np.float32(1.0)), 15), (0.25, 15), (0.125, 15), (0.0625, 15), (0.125, 7), (0.5, 0), (0.5, 4),
                  (np.nextafter(np.float32(0.4), np.float32(0.0)), 4)):
        c.append(case((0.0, 0.0, z), K=(512.0, 500.0, 0.0, 0.0), radius=-1, max_radius=mr))
        c.append(case((0.0, 0.0, z), K=(500.0, 512.0, 0.0, 0.0), radius=-1, max_radius=mr))
    c.append(case((0.0, 0.0, 0.5), K=(512.0, 512.0, 0.0, 0.0), radius=3, max_radius=0))  # a fixed radius ignores the cap
    return c


def bits(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def r_num(c):
    return (0.5 * float(c["res"])) * max(float(c["K"][0]), float(c["K"][1]))


def run_header(tmp_path, table):
    cxx = shutil.which("g++")
    assert cxx, "g++ is part of the build of this package"
    exe = os.path.join(tmp_path, "view_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "view_check.cpp")])
    lines = []
    for c in table:
        words = [bits(v) for v in c["pose"] + c["K"] + tuple(c["z"]) + c["p"]]
        lines.append(" ".join(words + ["%d %d %d %d" % (c["size"] + (c["radius"], c["max_radius"])), bits(r_num(c))]))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out and out[-1] == "view ok %d" % len(table), r.stdout[-4000:]
    return [l.split() for l in out[:-1]]


def same_double(got_hex, want):
    """Bit for bit; any NaN equals any NaN (the payload is not part of the contract)."""
    got = struct.unpack("<d", struct.pack("<Q", int(got_hex, 16)))[0]
    return (np.isnan(got) and np.isnan(want)) or got_hex == bits(want)


def test_the_header_agrees_with_the_numpy_restatements_on_every_edge(tmp_path):
    table = cases()
    got = run_header(tmp_path, table)
    seen = dict(rejected_near=0, rejected_far=0, rejected_pixel=0, drawn=0, outside=0, nan_zc=0, capped=0)
    for i, (c, g) in enumerate(zip(table, got)):
        what = "case %d: %r" % (i, c)
        depth_ok, pixel_ok, pu, pv, inside, r = int(g[0]), int(g[1]), int(g[6]), int(g[7]), int(g[8]), int(g[9])
        row = np.zeros(1, dtype=hfpf.ROW_DTYPE)
        row["x"], row["y"], row["z"] = c["p"]
        w, h = c["size"]
        pw = tuple(np.array([v], np.float64) for v in c["p"])
        with np.errstate(all="ignore"):  # the NaN and inf cases
            ok_r, zc_r, pu_r, pv_r = render_ref.project(row, c["pose"], c["K"], c["z"])
            ok_p, dx, dy, dz, zc_p, pu_p, pv_p = plan_ref.project(np.array([c["p"]], np.float32), c["pose"], c["K"], c["z"][0], c["z"][1])
            # the inside test: track's association into a view whose every pixel holds a row
            ok_t, _ = track_ref.associate(pw, c["pose"], np.zeros(w * h, np.uint64), w, h, c["K"], c["z"])
        assert pixel_ok == int(ok_r[0]) == int(ok_p[0]), what
        with np.errstate(invalid="ignore"):
            assert depth_ok == int(float(c["z"][0]) < zc_r[0] < float(c["z"][1])), what
        assert same_double(g[2], dx[0]) and same_double(g[3], dy[0]) and same_double(g[4], dz[0]), what
        assert same_double(g[5], zc_r[0]) and same_double(g[5], zc_p[0]), what
        assert (pu, pv) == (int(pu_r[0]), int(pv_r[0])) == (int(pu_p[0]), int(pv_p[0])), what
        assert inside == int(ok_t[0]), what
        if pixel_ok:
            want_r = c["radius"] if c["radius"] >= 0 else int(render_ref.auto_radius(c["res"], c["K"][0], c["K"][1], zc_r[0], c["max_radius"]))
            assert r == want_r, what
            seen["capped"] += c["radius"] < 0 and r == c["max_radius"]
        seen["rejected_near"] += not depth_ok and zc_r[0] <= c["z"][0]
        seen["rejected_far"] += not depth_ok and zc_r[0] >= c["z"][1]
        seen["rejected_pixel"] += depth_ok and not pixel_ok
        seen["drawn"] += inside
        seen["outside"] += pixel_ok and not inside
        seen["nan_zc"] += bool(np.isnan(zc_r[0]))
    assert all(seen.values()), seen  # the table reaches every branch it is there for


def included_files(path, seen):
    """path and every file it reaches through #include "...", followed transitively (paths relative to the including file)"""
    path = os.path.normpath(path)
    if path in seen:
        return seen
    seen.add(path)
    for rel in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', open(path).read(), re.M):
        included_files(os.path.join(os.path.dirname(path), rel), seen)
    return seen


def test_every_included_file_is_in_the_one_build_list():
    """csrc/Makefile's print-sources is the one list of the files libhfpf.so is built from: it holds everything hfpf.hip includes,
    view.hpp among it, and the two other build paths ask the Makefile instead of naming a header of their own."""
    out = subprocess.run(["make", "-s", "--no-print-directory", "-C", CSRC, "print-sources"], check=True, stdout=subprocess.PIPE, text=True).stdout
    listed = {os.path.normpath(os.path.join(CSRC, f)) for f in out.split()}
    assert all(os.path.isfile(f) for f in listed), sorted(f for f in listed if not os.path.isfile(f))
    reached = included_files(os.path.join(CSRC, "hfpf.hip"), set())
    assert len(reached) > 1 and reached <= listed, sorted(reached - listed)
    assert os.path.join(CSRC, "view.hpp") in reached
    cmake = open(os.path.join(ROOT, "high-fidelity-pointcloud-fusion_amd", "CMakeLists.txt")).read()
    variant = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    # CMake asks the Makefile for the list and its engine target depends on what it was told
    assert re.search(r"print-sources\s+OUTPUT_VARIABLE HFPF_ENGINE_SOURCES\b", cmake) and re.search(r"DEPENDS \$\{HFPF_ENGINE_SOURCES\}", cmake)
    for text in (cmake, variant):
        assert not re.search(r"\.hpp", text), "a build path names a csrc header of its own"
