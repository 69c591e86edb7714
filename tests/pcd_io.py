"""Minimal readers for the output files: test_cloud.pcd, meta.csv and the binary PLY of hfpf_write_ply (tests only)."""
import numpy as np


def read_pcd_ascii(path):
    hdr = {}
    with open(path) as f:
        while True:
            line = f.readline()
            if not line:
                raise ValueError("no DATA line")
            if line.startswith("#"):
                continue
            k, _, v = line.strip().partition(" ")
            hdr[k] = v
            if k == "DATA":
                break
        data = np.loadtxt(f, ndmin=2) if int(hdr["POINTS"]) else np.zeros((0, len(hdr["FIELDS"].split())))
    return hdr, data


def read_meta_csv(path):
    with open(path) as f:
        header = f.readline().rstrip("\n")
        rows = np.loadtxt(f, delimiter=",", ndmin=2)
    return header, rows


PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"), ("green", "u1"),
                       ("blue", "u1")])
PLY_FACE = np.dtype([("n", "u1"), ("i", "<u4", (3,))])


def read_ply(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode().splitlines()
    assert head[:2] == ["ply", "format binary_little_endian 1.0"]
    nv = int([h for h in head if h.startswith("element vertex")][0].split()[2])
    nf = int([h for h in head if h.startswith("element face")][0].split()[2])
    assert "property list uchar uint vertex_indices" in head
    assert [h.split()[-1] for h in head if h.startswith("property") and "list" not in h] == list(PLY_VERTEX.names)
    v = np.frombuffer(data, PLY_VERTEX, nv, end)
    f = np.frombuffer(data, PLY_FACE, nf, end + nv * PLY_VERTEX.itemsize)
    assert end + nv * PLY_VERTEX.itemsize + nf * PLY_FACE.itemsize == len(data)
    return v, f
