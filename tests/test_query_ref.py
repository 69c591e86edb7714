"""CPU: the point-query contract (tests/query_ref.py) against an O(N * M) brute force and on hand-built cases with known answers,
and the ctypes / numpy mirrors of the query structs against include/hfpf.h."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import hfpf
import query_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.01
BBOX = (0.0, 0.2, 0.0, 0.2, 0.0, 0.2)  # 20 cells per axis
IDENT = np.hstack([np.eye(3), np.zeros((3, 1))])


def rows_of(*specs):
    """specs: (ix, iy, iz, x, y, z, count[, normal]); sorted into extract's lexicographic order."""
    r = np.zeros(len(specs), dtype=hfpf.ROW_DTYPE)
    for i, s in enumerate(sorted(specs, key=lambda s: s[:3])):
        r[i]["ix"], r[i]["iy"], r[i]["iz"] = s[:3]
        r[i]["x"], r[i]["y"], r[i]["z"] = s[3:6]
        r[i]["count"] = s[6]
        r[i]["nx"], r[i]["ny"], r[i]["nz"] = s[7] if len(s) > 7 else (0.0, 0.0, -1.0)
        r[i]["sd_dist"] = 0.5 + i
        r[i]["rgb"] = 0x010203 * (i + 1)
    return r


def centre(i, j, k):
    return (RES * i + RES / 2, RES * j + RES / 2, RES * k + RES / 2)


def random_rows(rng, n, dim=20):
    cells = set()
    while len(cells) < n:
        cells.add(tuple(int(c) for c in rng.integers(0, dim, 3)))
    specs = []
    for c in cells:
        x, y, z = (np.float32(v + (rng.random() - 0.5) * RES * 0.9) for v in centre(*c))
        nrm = rng.normal(size=3)
        nrm = tuple(np.float32(v) for v in nrm / np.linalg.norm(nrm))
        specs.append(c + (x, y, z, int(rng.integers(0, 6)), nrm))
    return rows_of(*specs)


def same(a, b, what):
    for x, y, name in ((a[0], b[0], "hits"), (a[1], b[1], "rows")):
        if x.tobytes() != y.tobytes():
            bad = np.flatnonzero((x.view(np.uint8).reshape(len(x), -1) != y.view(np.uint8).reshape(len(y), -1)).any(axis=1))
            raise AssertionError("%s: %s differ at %d points, first %d: %r vs %r" % (what, name, bad.size, bad[0], x[bad[0]], y[bad[0]]))


def q(rows, pts, occ=None, pose=IDENT, **kw):
    occ = np.stack([rows["ix"], rows["iy"], rows["iz"]], axis=1) if occ is None else occ
    return Q.query(rows, occ, np.asarray(pts, np.float32).reshape(-1, 3), pose, BBOX, RES, **kw)


# ---- against the brute force ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(6))
def test_agrees_with_brute_force_on_random_rows(seed):
    rng = np.random.default_rng(seed)
    rows = random_rows(rng, 300)
    occ = np.unique(np.vstack([np.stack([rows["ix"], rows["iy"], rows["iz"]], axis=1), rng.integers(0, 21, (200, 3))]), axis=0)
    # points in and around the bbox, some on cell boundaries and bbox faces, some not finite
    pts = rng.uniform(-0.02, 0.22, (400, 3)).astype(np.float32)
    pts[::7] = (np.round(pts[::7] / RES) * RES).astype(np.float32)
    pts[1::11, 0] = np.float32(0.0)
    pts[2::13, 1] = np.float32(0.2)
    pts[3::17, 2] = np.nan
    pts[4::19, 0] = np.inf
    a = np.radians(10.0)
    pose = np.array([[np.cos(a), -np.sin(a), 0, 0.01], [np.sin(a), np.cos(a), 0, -0.005], [0, 0, 1, 0.002]])
    n_found = n_has_row = 0
    for radius, min_count, max_distance, zclip in [(0, 0.0, np.inf, False), (1, 0.0, np.inf, True), (2, 3.0, 0.015, False),
                                                   (4, 1.5, np.inf, False), (3, 0.0, 0.004, True), (1, 5.0, 1.0, False)]:
        kw = dict(radius=radius, min_count=min_count, max_distance=max_distance, zclip=zclip, z_clip=(0.01, 0.15))
        got = Q.query(rows, occ, pts, pose, BBOX, RES, **kw)
        ref = Q.brute_force(rows, occ, pts, pose, BBOX, RES, **kw)
        same(got, ref, str(kw))
        n_found += int((got[0]["flags"] & Q.FOUND != 0).sum())
        n_has_row += int((got[0]["flags"] & Q.HAS_ROW != 0).sum())
    assert n_found > 50 and n_has_row > 0, (n_found, n_has_row)


# ---- hand-built cases --------------------------------------------------------------------------------------------------

def test_nearest_row_inside_the_window():
    c = centre(5, 5, 5)
    rows = rows_of((5, 5, 5, 0.051, c[1], c[2], 3), (6, 5, 5, 0.061, c[1], c[2], 4, (1.0, 0.0, 0.0)))
    p = np.float32([0.058, c[1], c[2]])  # in cell 5, nearer cell 6's centroid
    hits, out = q(rows, [p], radius=1)
    h = hits[0]
    assert h["flags"] == Q.USED | Q.IN_BBOX | Q.OCCUPIED | Q.HAS_ROW | Q.FOUND
    assert h["voxel"].tolist() == [5, 5, 5] and h["row_voxel"].tolist() == [6, 5, 5] and h["row_count"] == 4
    d = float(p[0]) - float(np.float32(0.061))
    assert h["distance"] == np.float32(abs(d)) and h["signed_distance"] == np.float32(d) and d < 0
    assert out[0].tobytes() == rows[1].tobytes()
    # radius 0: only the own cell
    hits, out = q(rows, [p], radius=0)
    assert hits[0]["row_voxel"].tolist() == [5, 5, 5] and out[0].tobytes() == rows[0].tobytes()


def test_each_edge_of_the_radius():
    for r in range(5):
        for off in (r, r + 1, -r, -r - 1):
            rows = rows_of((10 + off, 10, 10) + centre(10 + off, 10, 10) + (2,))
            hits, _ = q(rows, [centre(10, 10, 10)], radius=r)
            assert bool(hits[0]["flags"] & Q.FOUND) == (abs(off) <= r), (r, off)
            rows = rows_of((10 + off, 10 - off, 10 + off) + centre(10 + off, 10 - off, 10 + off) + (2,))
            hits, _ = q(rows, [centre(10, 10, 10)], radius=r)
            assert bool(hits[0]["flags"] & Q.FOUND) == (abs(off) <= r), (r, off)


def test_a_tie_goes_to_the_smallest_voxel():
    p = centre(8, 8, 8)
    # three rows with the same centroid: the same d2 from any point
    rows = rows_of((9, 8, 8, p[0], p[1], p[2] + 0.003, 1), (7, 8, 8, p[0], p[1], p[2] + 0.003, 1), (8, 9, 8, p[0], p[1], p[2] + 0.003, 1))
    hits, out = q(rows, [p], radius=1)
    assert hits[0]["row_voxel"].tolist() == [7, 8, 8] and out[0].tobytes() == rows[0].tobytes()
    hits, _ = q(rows[1:], [p], radius=1)
    assert hits[0]["row_voxel"].tolist() == [8, 9, 8]
    same(q(rows, [p], radius=1), Q.brute_force(rows, np.zeros((0, 3)), np.float32([p]), IDENT, BBOX, RES, radius=1)[:1] +
         (q(rows, [p], radius=1)[1],), "tie")


def test_min_count_and_max_distance_gates():
    rows = rows_of((4, 4, 4) + centre(4, 4, 4) + (1,), (4, 4, 5) + centre(4, 4, 5) + (0,), (4, 5, 4) + centre(4, 5, 4) + (5,))
    p = centre(4, 4, 4)
    hits, _ = q(rows, [p], radius=1)
    assert hits[0]["row_voxel"].tolist() == [4, 4, 4] and hits[0]["flags"] & Q.HAS_ROW
    hits, _ = q(rows, [p], radius=1, min_count=2.0)  # count 1 and 0 fall out
    assert hits[0]["row_voxel"].tolist() == [4, 5, 4] and not hits[0]["flags"] & Q.HAS_ROW
    hits, out = q(rows, [p], radius=1, min_count=2.0, max_distance=0.009)  # 1 cm away: beyond the gate
    assert not hits[0]["flags"] & Q.FOUND and out[0]["ix"] == -1 and out[0]["count"] == 0
    assert np.isnan(hits[0]["distance"]) and hits[0]["row_voxel"].tolist() == [-1, -1, -1]
    hits, _ = q(rows, [p], radius=1, min_count=2.0, max_distance=0.011)
    assert hits[0]["flags"] & Q.FOUND
    hits, _ = q(rows, [p], radius=0, min_count=0.0)  # count 0 rows are never candidates
    assert hits[0]["flags"] & Q.FOUND


def test_unused_points_and_the_zclip_flag():
    rows = rows_of((1, 1, 1) + centre(1, 1, 1) + (2,))
    pts = [(np.nan, 0.01, 0.01), (0.01, np.inf, 0.01), centre(1, 1, 1), (0.015, 0.015, 0.5)]
    hits, out = q(rows, pts, radius=0, zclip=True, z_clip=(0.0, 0.02))
    assert hits["flags"].tolist() == [0, 0, Q.USED | Q.IN_BBOX | Q.OCCUPIED | Q.HAS_ROW | Q.FOUND, 0]
    for i in (0, 1, 3):
        assert hits[i]["voxel"].tolist() == [Q.INT_MIN] * 3 and (hits[i]["p"].view(np.uint32) == Q.NAN_BITS).all()
        assert hits[i]["distance"].view(np.uint32) == Q.NAN_BITS and out[i]["ix"] == -1
    hits, _ = q(rows, pts, radius=0, zclip=False)
    assert hits["flags"][3] == Q.USED and hits[3]["voxel"].tolist() == [1, 1, 50]  # outside the bbox: voxel, p, no search


def test_bbox_faces_are_outside():
    rows = rows_of((0, 0, 0) + centre(0, 0, 0) + (2,), (19, 19, 19) + centre(19, 19, 19) + (2,))
    hits, _ = q(rows, [(0.0, 0.005, 0.005), (0.2, 0.195, 0.195), (np.float32(1e-9), 0.005, 0.005), (0.19999, 0.195, 0.195)], radius=1)
    assert [int(f & Q.IN_BBOX) for f in hits["flags"]] == [0, 0, Q.IN_BBOX, Q.IN_BBOX]
    assert hits[2]["row_voxel"].tolist() == [0, 0, 0] and hits[3]["row_voxel"].tolist() == [19, 19, 19]


def test_voxel_boundaries_follow_the_floor():
    # 0.03 / 0.01 rounds below 3 in f64: the point belongs to cell 2, as integrate indexes it
    p = np.float32([0.03, 0.05, 0.07])
    v = Q.voxel(p.reshape(1, 3), BBOX, RES)[0]
    assert v.tolist() == [int(np.floor(float(c) / RES)) for c in p]


def test_occupied_without_a_row():
    rows = rows_of((2, 2, 2) + centre(2, 2, 2) + (2,))
    hits, _ = q(rows, [centre(3, 3, 3)], occ=np.array([[3, 3, 3], [2, 2, 2]]), radius=0)
    assert hits[0]["flags"] == Q.USED | Q.IN_BBOX | Q.OCCUPIED
    hits, _ = q(rows, [centre(3, 3, 3)], occ=np.array([[3, 3, 3], [2, 2, 2]]), radius=1)
    assert hits[0]["flags"] == Q.USED | Q.IN_BBOX | Q.OCCUPIED | Q.FOUND


# ---- the ctypes / numpy mirrors against the header -------------------------------------------------------------------

FIELDS = {"hfpf_query_opts": [f for f, _ in hfpf.QueryOpts._fields_], "hfpf_query_hit": list(hfpf.QUERY_HIT_DTYPE.names)}


def test_structs_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler to check the header with")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hfpf.h"', "int main(void) {"]
    for s, fields in FIELDS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for f in fields:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    lines.append('printf("flags %u %u %u %u %u %u\\n", HFPF_QUERY_ZCLIP, HFPF_QHIT_USED, HFPF_QHIT_IN_BBOX, HFPF_QHIT_OCCUPIED, '
                 'HFPF_QHIT_HAS_ROW, HFPF_QHIT_FOUND);')
    lines.append("return 0; }")
    src = tmp_path / "q.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "q"
    subprocess.check_call([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) if not line.startswith("flags") else ("flags", line[6:]) for line in
               subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["hfpf_query_opts"]) == C.sizeof(hfpf.QueryOpts) == 40
    for f, _ in hfpf.QueryOpts._fields_:
        assert int(got["hfpf_query_opts." + f]) == getattr(hfpf.QueryOpts, f).offset, f
    assert int(got["hfpf_query_hit"]) == hfpf.QUERY_HIT_DTYPE.itemsize == Q.HIT_DTYPE.itemsize == 64
    for f in hfpf.QUERY_HIT_DTYPE.names:
        assert int(got["hfpf_query_hit." + f]) == hfpf.QUERY_HIT_DTYPE.fields[f][1], f
    assert hfpf.QUERY_HIT_DTYPE == Q.HIT_DTYPE
    assert got["flags"].split() == [str(v) for v in (hfpf.QUERY_ZCLIP, Q.USED, Q.IN_BBOX, Q.OCCUPIED, Q.HAS_ROW, Q.FOUND)]
