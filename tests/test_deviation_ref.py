"""CPU: the deviation contract (tests/deviation_ref.py) on hand-computed cases, its pruned search against the plain double loop, and
the host-side pieces of the library: hfpf_check_deviation_opts, the struct sizes and the PLY reader."""
import ctypes as C
import os

import numpy as np
import pytest

import deviation_ref as D

IDENT = np.eye(4)[:3]
A, B, C3 = np.array([0.0, 0, 0]), np.array([2.0, 0, 0]), np.array([0.0, 2, 0])  # a right triangle in z = 0, normal +z


def _rows(P):
    r = np.zeros(len(P), D.ROW_DTYPE)
    P = np.asarray(P, np.float32)
    r["x"], r["y"], r["z"] = P[:, 0], P[:, 1], P[:, 2]
    r["count"] = 5
    r["ix"] = np.arange(len(P))
    return r


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


REGIONS = [  # P, expected Q, flag bits of the region, sign
    ((-1.0, -1.0, 1.0), (0, 0, 0), D.ON_VERTEX, +1), ((3.0, -0.5, -1.0), (2, 0, 0), D.ON_VERTEX, -1), ((-0.5, 3.0, 2.0), (0, 2, 0), D.ON_VERTEX, +1),
    ((1.0, -1.0, 1.0), (1, 0, 0), D.ON_EDGE, +1), ((-1.0, 0.5, -1.0), (0, 0.5, 0), D.ON_EDGE, -1), ((2.0, 2.0, 1.0), (1, 1, 0), D.ON_EDGE, +1),
    ((0.5, 0.5, -0.25), (0.5, 0.5, 0), 0, -1),
]


@pytest.mark.parametrize("case", REGIONS, ids=["A", "B", "C", "AB", "AC", "BC", "face"])
def test_each_region_by_hand(case):
    P, Q, flag, sign = case
    q, region, dd = D.closest_point(np.array(P), A, B, C3)
    assert q.tolist() == [float(v) for v in Q] and int(region) == flag
    want = sum((p - v) ** 2 for p, v in zip(P, Q))
    assert dd == want
    dev, s = D.compare(_rows([P]), _f32([A, B, C3]), 12, [[0, 1, 2]], IDENT, 0.0, 10.0)
    assert dev["flags"][0] == (D.FOUND | flag) and dev["tri"][0] == 0
    assert dev["distance"][0] == np.float32(np.sqrt(want)) and dev["signed_distance"][0] == np.float32(sign * np.sqrt(want))
    assert dev["q"][0].tolist() == [float(v) for v in Q] and dev["reserved"][0] == 0
    assert s["n_found"] == 1 and s["n_negative"] == (1 if sign < 0 else 0) and s["n_tris_valid"] == 1


def test_tie_on_a_shared_edge_goes_to_the_smaller_index():
    verts = _f32([[0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0]])
    P = [[1.0, 1.0, 0.5]]  # above the diagonal both triangles share
    for tris, want in (([[0, 1, 2], [1, 3, 2]], 0), ([[1, 3, 2], [0, 1, 2]], 0)):
        for prune in (True, False):
            dev, _ = D.compare(_rows(P), verts, 12, tris, IDENT, 0.0, 1.0, prune=prune)
            assert dev["tri"][0] == want and dev["distance"][0] == np.float32(0.5)


def test_invalid_triangles_are_skipped_and_counted():
    verts = _f32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [np.nan, 0, 0], [0, 0, 1]])
    tris = [[0, 1, 1], [0, 1, 3], [0, 1, 4], [0, 1, 6], [0, 1, 0xFFFFFFFF], [0, 1, 2]]  # repeated, collinear, NaN, two out of range, valid
    for prune in (True, False):
        dev, s = D.compare(_rows([[0.25, 0.25, 0.125]]), verts, 12, tris, IDENT, 0.0, 1.0, prune=prune)
        assert s["n_tris_invalid"] == 5 and s["n_tris_valid"] == 1
        assert dev["tri"][0] == 5 and dev["distance"][0] == np.float32(0.125) and dev["flags"][0] == D.FOUND


def test_dd_equal_to_the_bound_is_kept_and_beyond_is_not():
    P = [[0.5, 0.5, 0.25]]
    for prune in (True, False):
        dev, s = D.compare(_rows(P), _f32([A, B, C3]), 12, [[0, 1, 2]], IDENT, 0.0, 0.25, prune=prune)
        assert dev["flags"][0] == D.FOUND and dev["distance"][0] == np.float32(0.25)
        dev, s = D.compare(_rows(P), _f32([A, B, C3]), 12, [[0, 1, 2]], IDENT, 0.0, np.nextafter(0.25, 0), prune=prune)
        assert dev["flags"][0] == 0 and dev["tri"][0] == D.NO_TRI and s["n_found"] == 0 and s["max_abs"] == 0.0
        assert dev["distance"].view(np.uint32)[0] == D.NAN_BITS and (dev["q"].view(np.uint32) == D.NAN_BITS).all()
        assert dev["signed_distance"].view(np.uint32)[0] == D.NAN_BITS


def _random_case(seed):
    rng = np.random.default_rng(seed)
    P = rng.uniform(-0.1, 0.1, (300, 3))
    c = P[rng.integers(0, 300, 400)] + rng.uniform(-0.03, 0.03, (400, 3))
    verts = (c[:, None, :] + rng.uniform(-0.01, 0.01, (400, 3, 3))).reshape(-1, 3)
    tris = np.arange(1200, dtype=np.uint32).reshape(400, 3)
    return _rows(P), _f32(verts), tris


@pytest.mark.parametrize("posed", [False, True], ids=["identity", "posed"])
def test_pruned_equals_the_double_loop(posed):
    rows, verts, tris = _random_case(11)
    pose = IDENT
    if posed:  # the mesh given in another frame: rotate and shift it there, the pose brings it back (up to rounding)
        a = 0.7
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]]) @ np.array([[1, 0, 0], [0, 0.8, -0.6], [0, 0.6, 0.8]])
        t = np.array([0.3, -0.2, 0.1])
        verts = _f32((verts.astype(np.float64) - t) @ R)
        pose = np.hstack([R, t.reshape(3, 1)])
    for md in (0.03, 0.004):
        a_dev, a_sum = D.compare(rows, verts, 12, tris, pose, 0.0, md, prune=True)
        b_dev, b_sum = D.compare(rows, verts, 12, tris, pose, 0.0, md, prune=False)
        assert a_dev.tobytes() == b_dev.tobytes() and a_sum == b_sum
        assert 0 < a_sum["n_found"] and (md > 0.01 or a_sum["n_found"] < 300)
    found = (a_dev["flags"] & D.FOUND) != 0
    assert set(np.unique(a_dev["flags"][found])) <= {1, 3, 5}


def test_summary_is_rebuilt_from_the_rows_and_count_gate():
    rows, verts, tris = _random_case(5)
    rows["count"][::3] = 1
    dev, s = D.compare(rows, verts, 12, tris, IDENT, 2.0, 0.02)
    assert s["n_rows"] == len(dev) == 200
    again = D.summary(dev)
    for k in ("n_rows", "n_found", "n_negative", "max_abs", "sum_abs_q30", "sum_sq_q30"):
        assert again[k] == s[k]
    d = dev["distance"][(dev["flags"] & 1) != 0].astype(np.float64)
    assert s["sum_abs_q30"] == sum(int(np.rint(v * 2.0 ** 30)) for v in d) and s["max_abs"] == float(d.max())
    assert s["n_negative"] == int((dev["signed_distance"] < 0).sum()) > 0
    # stride 32: the same mesh as hfpf_mesh_vertex records
    mv = np.zeros(len(verts), [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rest", "<u4", (5,))])
    mv["x"], mv["y"], mv["z"] = verts[:, 0], verts[:, 1], verts[:, 2]
    dev32, s32 = D.compare(rows, mv, 32, tris, IDENT, 2.0, 0.02)
    assert dev32.tobytes() == dev.tobytes() and s32 == s


# ---- through the library (host code: no GPU) ---------------------------------------------------------------------------

def test_check_deviation_opts_and_struct_sizes(hfpf_mod):
    H = hfpf_mod
    assert C.sizeof(H.DeviationOpts) == 32 and C.sizeof(H.DeviationSummary) == 64 and H.DEVIATION_DTYPE.itemsize == 32
    assert H.DEVIATION_DTYPE == D.DEVIATION_DTYPE
    assert (H.DEV_FOUND, H.DEV_ON_EDGE, H.DEV_ON_VERTEX) == (D.FOUND, D.ON_EDGE, D.ON_VERTEX)
    assert H.check_deviation_opts(H.deviation_opts()) == 0
    assert H.check_deviation_opts(None) == H.HFPF_ERR_BAD_ARG if hasattr(H, "HFPF_ERR_BAD_ARG") else H.check_deviation_opts(None) == -2
    faults = [("struct_size", 28), ("flags", 1), ("reserved", 1), ("min_count", float("nan")), ("max_distance", float("nan")),
              ("max_distance", float("inf")), ("max_distance", 0.0), ("max_distance", -0.01)]
    for field, value in faults:
        o = H.deviation_opts()
        setattr(o, field, value)
        assert H.check_deviation_opts(o) == -2, (field, value)


def _mesh5(H):
    v = np.zeros(5, H.MESH_VERTEX_DTYPE)
    v["x"], v["y"], v["z"] = [0, 1, 0, 1, 0.5], [0, 0, 1, 1, 0.5], [0, 0, 0, 0, 1]
    v["nx"], v["ny"], v["nz"] = 0.0, 0.6, 0.8
    v["rgb"] = [0x000000, 0xFF0000, 0x00FF00, 0x0000FF, 0x123456]
    t = np.array([[0, 1, 4], [1, 3, 4], [3, 2, 4], [2, 0, 4]], np.uint32)
    return v, t


def test_ply_round_trip(hfpf_mod, tmp_path):
    H = hfpf_mod
    v, t = _mesh5(H)
    path = tmp_path / "m.ply"
    H.write_ply(v, t, path)
    v2, t2 = H.read_ply(path)
    assert v2.tobytes() == v.tobytes() and t2.tobytes() == t.tobytes()  # count is 0 on both sides


def _write(path, header, body):
    with open(path, "wb") as f:
        f.write(header.encode() + body)
    return path


HEAD_XYZ = ("ply\nformat binary_little_endian 1.0\ncomment made by hand\nelement vertex %d\nproperty float x\nproperty double extra\nproperty float y\n"
            "property float z\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n")


def test_ply_with_only_xyz_and_a_skipped_property(hfpf_mod, tmp_path):
    H = hfpf_mod
    rec = np.zeros(3, [("x", "<f4"), ("extra", "<f8"), ("y", "<f4"), ("z", "<f4")])
    rec["x"], rec["y"], rec["z"], rec["extra"] = [1, 2, 3], [4, 5, 6], [7, 8, 9], 1e300
    face = b"\x03" + np.array([0, 1, 2], "<i4").tobytes()
    v, t = H.read_ply(_write(tmp_path / "xyz.ply", HEAD_XYZ % (3, 1), rec.tobytes() + face))
    assert v["x"].tolist() == [1, 2, 3] and v["y"].tolist() == [4, 5, 6] and v["z"].tolist() == [7, 8, 9]
    assert not v["nx"].any() and not v["ny"].any() and not v["nz"].any() and not v["rgb"].any() and not v["count"].any()
    assert t.tolist() == [[0, 1, 2]]


def test_ply_faults_are_io_errors(hfpf_mod, tmp_path):
    H = hfpf_mod
    v, t = _mesh5(H)
    good = tmp_path / "good.ply"
    H.write_ply(v, t, good)
    blob = open(good, "rb").read()
    head_end = blob.index(b"end_header\n") + len(b"end_header\n")
    cases = {
        "ascii": blob.replace(b"binary_little_endian", b"ascii"),
        "truncated": blob[:-5],
        "quad": blob[:head_end + 5 * 27] + b"\x04" + blob[head_end + 5 * 27 + 1:],
        "too_many_vertices": blob.replace(b"element vertex 5", b"element vertex 4000000000"),
        "too_many_faces": blob.replace(b"element face 4", b"element face 400000"),
        "no_header_end": blob[:head_end - 4],
    }
    for name, data in cases.items():
        path = tmp_path / (name + ".ply")
        open(path, "wb").write(data)
        with pytest.raises(H.HfpfError) as e:
            H.read_ply(path)
        assert e.value.code == -6 and "read_ply" in str(e.value), name
    with pytest.raises(H.HfpfError) as e:
        H.read_ply(tmp_path / "missing.ply")
    assert e.value.code == -6
