"""CPU: hfpf_write_ply round-trips through a numpy parser, and the mesh structs of include/hfpf.h have their stated sizes and layout."""
import ctypes as C
import os

import numpy as np

import hfpf
import mesh_ref as M
from pcd_io import read_ply


def test_structs_have_their_stated_sizes():
    assert C.sizeof(hfpf.MeshOpts) == 32
    assert hfpf.MESH_VERTEX_DTYPE.itemsize == 32 and hfpf.MESH_VERTEX_DTYPE == M.VERTEX_DTYPE
    assert [f[0] for f in hfpf.MeshOpts._fields_] == ["struct_size", "radius", "min_count", "max_distance", "flags", "reserved"]
    o = hfpf.mesh_opts()
    assert o.struct_size == 32 and o.radius == 2 and o.min_count == 0.0 and o.max_distance == float("inf") and o.flags == 0


def test_ply_round_trips(tmp_path):
    rng = np.random.default_rng(3)
    v = np.zeros(1000, hfpf.MESH_VERTEX_DTYPE)
    for k in ("x", "y", "z", "nx", "ny", "nz"):
        v[k] = rng.normal(size=len(v)).astype(np.float32)
    v["rgb"] = rng.integers(0, 1 << 24, len(v))
    v["count"] = rng.integers(1, 100, len(v))
    t = rng.integers(0, len(v), (70000, 3)).astype(np.uint32)  # more than one write chunk
    path = os.path.join(tmp_path, "mesh.ply")
    hfpf.write_ply(v, t, path)
    pv, pf = read_ply(path)
    for k in ("x", "y", "z", "nx", "ny", "nz"):
        assert pv[k].tobytes() == v[k].tobytes(), k
    assert (pv["red"] == v["rgb"] >> 16).all() and (pv["green"] == (v["rgb"] >> 8) & 255).all() and (pv["blue"] == v["rgb"] & 255).all()
    assert (pf["n"] == 3).all() and (pf["i"] == t).all()


def test_empty_ply_and_bad_arguments(tmp_path):
    path = os.path.join(tmp_path, "empty.ply")
    hfpf.write_ply(np.zeros(0, hfpf.MESH_VERTEX_DTYPE), np.zeros((0, 3), np.uint32), path)
    v, f = read_ply(path)
    assert len(v) == 0 and len(f) == 0
    L = hfpf.lib()
    assert L.hfpf_write_ply(None, 3, None, 0, path.encode()) == -2
    assert L.hfpf_write_ply(None, 0, None, 0, None) == -2
    assert L.hfpf_write_ply(None, 0, None, 0, os.path.join(tmp_path, "no", "such", "dir.ply").encode()) < 0


def test_the_options_check():
    L = hfpf.lib()
    assert L.hfpf_check_mesh_opts(C.byref(hfpf.mesh_opts())) == 0
    for r in (1, 4):
        assert L.hfpf_check_mesh_opts(C.byref(hfpf.mesh_opts(radius=r, min_count=-1.0, max_distance=1e-6))) == 0
    bad = {"struct_size": 24, "flags": 1, "reserved": 1, "radius": 0, "min_count": float("nan"), "max_distance": 0.0}
    for field, val in list(bad.items()) + [("radius", 5), ("max_distance", -1.0), ("max_distance", float("nan"))]:
        o = hfpf.mesh_opts()
        setattr(o, field, val)
        assert L.hfpf_check_mesh_opts(C.byref(o)) == -2, (field, val)
    assert L.hfpf_check_mesh_opts(None) == -2
