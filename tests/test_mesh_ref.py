"""CPU: the mesh contract's numpy restatement (tests/mesh_ref.py) on synthetic row sets with known surfaces: a plane patch, a closed
sphere, and a per-cube unwelded construction against the welded one."""
import numpy as np
import pytest

import hfpf
import mesh_ref as M

RES = 0.005
BBOX = (0.0, 0.2, 0.0, 0.2, 0.0, 0.2)  # 40 cells per axis
DIMS = (40, 40, 40)


def rows_at(cells, xyz, normals):
    """Rows in extract's order for cells (n, 3), centroids (n, 3) and normals (n, 3)."""
    order = np.lexsort((cells[:, 2], cells[:, 1], cells[:, 0]))
    r = np.zeros(len(cells), hfpf.ROW_DTYPE)
    for k, a in enumerate(("ix", "iy", "iz")):
        r[a] = cells[order, k]
    for k, a in enumerate(("x", "y", "z")):
        r[a] = xyz[order, k]
    for k, a in enumerate(("nx", "ny", "nz")):
        r[a] = normals[order, k]
    r["count"] = 5
    r["rgb"] = (np.arange(len(r)) * 0x010305) & 0xFFFFFF
    return r


def plane_rows(z0=0.0512):
    ij = np.array([(i, j) for i in range(8, 30) for j in range(10, 28)], np.int64)
    k0 = int(np.floor(z0 / RES))
    cells = np.column_stack([ij, np.full(len(ij), k0)])
    xyz = np.column_stack([(cells[:, :2] + 0.5) * RES, np.full(len(ij), z0)]).astype(np.float32)
    return rows_at(cells, xyz, np.tile(np.float32([0, 0, 1]), (len(ij), 1))), z0


def sphere_rows(c=(0.1, 0.1, 0.1), r=0.06):
    c = np.asarray(c)
    g = np.stack(np.meshgrid(*[np.arange(40)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    centre = (g + 0.5) * RES
    d = np.linalg.norm(centre - c, axis=1)
    near = np.abs(d - r) < 0.87 * RES
    cells, centre, d = g[near], centre[near], d[near]
    nrm = (centre - c) / d[:, None]
    xyz = (c + nrm * r).astype(np.float32)
    return rows_at(cells, xyz, nrm.astype(np.float32)), c, r


def occ_of(rows):
    return np.stack([rows["ix"], rows["iy"], rows["iz"]], axis=1).astype(np.int32)


@pytest.fixture(scope="module")
def plane():
    rows, z0 = plane_rows()
    v, t, sizes = M.mesh(rows, occ_of(rows), BBOX, RES, DIMS, radius=2)
    return rows, z0, v, t


@pytest.fixture(scope="module")
def sphere():
    rows, c, r = sphere_rows()
    v, t, sizes = M.mesh(rows, occ_of(rows), BBOX, RES, DIMS, radius=2)
    return rows, c, r, v, t


def test_the_table_covers_every_case_once():
    for t in range(6):
        assert M.TABLE[(t, 0)] == [] and M.TABLE[(t, 15)] == []
        for m in range(1, 15):
            n_in = bin(m).count("1")
            assert len(M.TABLE[(t, m)]) == (2 if n_in == 2 else 1)
            # complementary cases are the same surface with the opposite winding
            a, b = M.TABLE[(t, m)], M.TABLE[(t, 15 - m)]
            assert sorted(map(sorted, a)) == sorted(map(sorted, b))


def test_plane_vertices_lie_on_the_plane(plane):
    rows, z0, v, t = plane
    assert len(v) > 100 and len(t) > 100
    assert np.abs(v["z"].astype(np.float64) - z0).max() < 1e-6
    assert (v["nz"] == 1).all()


def test_plane_is_a_disc_with_upward_faces(plane):
    rows, z0, v, t = plane
    u, cnt, net = M.edge_use(t)
    assert cnt.max() <= 2
    assert (net[cnt == 2] == 0).all(), "interior edges are used twice, in opposite directions"
    assert M.euler(len(v), t) == 1
    n = M.face_normals(v, t)
    big = np.linalg.norm(n, axis=1) > 1e-12
    assert (n[big, 2] > 0).all()


def test_sphere_is_closed(sphere):
    rows, c, r, v, t = sphere
    u, cnt, net = M.edge_use(t)
    assert (cnt == 2).all() and (net == 0).all()
    assert M.euler(len(v), t) == 2


def test_sphere_volume_and_radii(sphere):
    rows, c, r, v, t = sphere
    p = M.positions(v).astype(np.float64) - c
    tt = np.asarray(t, np.int64)
    vol = np.einsum("ij,ij->i", p[tt[:, 0]], np.cross(p[tt[:, 1]], p[tt[:, 2]])).sum() / 6.0
    assert abs(vol / (4.0 / 3.0 * np.pi * r ** 3) - 1.0) < 0.02
    assert np.abs(np.linalg.norm(p, axis=1) - r).max() < 0.25 * RES
    n = M.face_normals(v, t)
    ctr = p[tt].mean(axis=1)
    assert (np.einsum("ij,ij->i", n, ctr) > 0).mean() > 0.99, "faces look outwards, to the sensor side"


def test_unwelded_construction_agrees_with_the_welded_mesh(sphere):
    rows, c, r, v, t = sphere
    loose = M.mesh_unwelded(rows, occ_of(rows), BBOX, RES, DIMS, radius=2)
    welded = M.positions(v)[np.asarray(t, np.int64)]
    assert loose.shape == welded.shape
    assert loose.tobytes() == welded.tobytes()
    # welding by exact position gives back as many vertices as the welded mesh has
    assert len(np.unique(loose.reshape(-1, 3), axis=0)) == len(v)


def test_attributes_come_from_the_closer_endpoint():
    rows, z0 = plane_rows()
    v, t, _ = M.mesh(rows, occ_of(rows), BBOX, RES, DIMS, radius=2)
    assert set(v["rgb"]) <= set(rows["rgb"]) and (v["count"] == 5).all()


def test_gates_and_empty_sets():
    rows, z0 = plane_rows()
    v, t, s = M.mesh(rows, occ_of(rows), BBOX, RES, DIMS, radius=2, min_count=6)
    assert len(v) == 0 and len(t) == 0 and s["cubes"] == 0
    # a tight distance gate leaves corners undefined: fewer meshed cubes, never more triangles
    v2, t2, _ = M.mesh(rows, occ_of(rows), BBOX, RES, DIMS, radius=2, max_distance=0.4 * RES)
    _, tt, _ = M.mesh(rows, occ_of(rows), BBOX, RES, DIMS, radius=2)
    assert len(t2) < len(tt)
