"""The mesh contract of include/hfpf.h restated in numpy (imported by tests only): extracted rows + the occupied list -> the vertices
and triangles hfpf_extract_mesh* return.  The corner samples are tests/query_ref.py's hits of the lattice points; the cube set, the
Kuhn tetrahedra, the case / winding table, the welded vertex order and the triangle order follow the header's text."""
import numpy as np

import query_ref as Q

VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("rgb", "<u4"),
                         ("count", "<u4")])
assert VERTEX_DTYPE.itemsize == 32
# cube corner codes 4 dx + 2 dy + dz; the Kuhn tetrahedra of the permutations xyz, xzy, yxz, yzx, zxy, zyx: 0, e_pi1, e_pi1 + e_pi2, 7
TETS = ((0, 4, 6, 7), (0, 4, 5, 7), (0, 2, 6, 7), (0, 2, 3, 7), (0, 1, 5, 7), (0, 1, 3, 7))
POP = np.array([bin(i).count("1") for i in range(256)], np.uint32)
IDENT = np.hstack([np.eye(3), np.zeros((3, 1))])


def offset(code):
    """The (dx, dy, dz) of a corner or direction code."""
    return np.array([code >> 2 & 1, code >> 1 & 1, code & 1], np.int64)


def offset_key(code):
    d = offset(code)
    return int(Q.keys(d[0], d[1], d[2]))


def case_table():
    """{(tetrahedron, inside mask): [triangle, ...]}, a triangle = three lattice edges (origin code, direction code)."""
    table = {}
    for t, tet in enumerate(TETS):
        for m in range(16):
            ins = [i for i in range(4) if m >> i & 1]
            outs = [i for i in range(4) if not m >> i & 1]
            if len(ins) == 1:
                tris = [[(ins[0], o) for o in outs]]
            elif len(ins) == 3:
                tris = [[(i, outs[0]) for i in ins]]
            elif len(ins) == 2:
                e = lambda I, O: (ins[I], outs[O])  # noqa: E731
                tris = [[e(0, 0), e(0, 1), e(1, 1)], [e(0, 0), e(1, 1), e(1, 0)]]
            else:
                tris = []
            want = len(ins) * sum((offset(tet[o]) for o in outs), np.zeros(3, np.int64)) - \
                len(outs) * sum((offset(tet[i]) for i in ins), np.zeros(3, np.int64))
            out = []
            for tri in tris:
                mid = [offset(tet[i]) + offset(tet[o]) for i, o in tri]
                if not np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), want) > 0:
                    tri = [tri[0], tri[2], tri[1]]
                out.append([(min(tet[i], tet[o]), max(tet[i], tet[o]) - min(tet[i], tet[o])) for i, o in tri])
            table[(t, m)] = out
    return table


TABLE = case_table()


def lattice_points(keys, bbox, res):
    """c[a] = (float)(bbox_min[a] + (double)i_a * res) of lattice keys."""
    lo = np.asarray(bbox, np.float64)[0::2]
    ijk = [(keys >> (Q.KEY_BITS * (2 - a))) & ((1 << Q.KEY_BITS) - 1) for a in range(3)]
    return np.stack([(lo[a] + ijk[a].astype(np.float64) * float(res)).astype(np.float32) for a in range(3)], axis=1)


def cube_set(rows, dims, min_count=0.0):
    """Sorted keys of the valid cells within Chebyshev distance 1 of a candidate row's cell."""
    cand = Q.candidates(rows, min_count)
    cells = np.stack([cand["ix"], cand["iy"], cand["iz"]], axis=1).astype(np.int64)
    out = []
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for oz in (-1, 0, 1):
                c = cells + np.array([ox, oy, oz])
                ok = ((c >= 0) & (c < np.asarray(dims))).all(axis=1)
                out.append(Q.keys(c[ok, 0], c[ok, 1], c[ok, 2]))
    return np.unique(np.concatenate(out)) if out else np.zeros(0, np.int64)


def corner_set(cubes):
    return np.unique(np.concatenate([cubes + offset_key(c) for c in range(8)])) if len(cubes) else np.zeros(0, np.int64)


def samples(rows, occupied, corners, bbox, res, radius, min_count, max_distance):
    """(defined, s, row) per corner: the query hit of the lattice point under the identity pose."""
    pts = lattice_points(corners, bbox, res)
    hits, rws = Q.query(rows, occupied, pts, IDENT, bbox, res, radius=radius, min_count=min_count, max_distance=max_distance)
    return (hits["flags"] & Q.FOUND) != 0, hits["signed_distance"], rws


def mesh(rows, occupied, bbox, res, dims, radius=2, min_count=0.0, max_distance=np.inf, with_ends=False):
    """(vertices of VERTEX_DTYPE, triangles (n, 3) uint32, sizes dict) of hfpf_extract_mesh.  with_ends: a fourth element, the rows
    of each vertex's two edge endpoints (origin, far end) as two row arrays."""
    cubes = cube_set(rows, dims, min_count)
    corners = corner_set(cubes)
    sizes = {"cubes": len(cubes), "corners": len(corners)}
    if not len(cubes):
        empty = (np.zeros(0, VERTEX_DTYPE), np.zeros((0, 3), np.uint32), sizes)
        return empty + ((Q.empty_rows(0, rows.dtype),) * 2,) if with_ends else empty
    defined, s, rws = samples(rows, occupied, corners, bbox, res, radius, min_count, max_distance)
    idx = np.stack([np.searchsorted(corners, cubes + offset_key(c)) for c in range(8)], axis=1)
    meshed = defined[idx].all(axis=1)
    inside = s[idx] < 0
    cases = np.stack([sum(inside[:, tet[i]].astype(np.int64) << i for i in range(4)) for tet in TETS], axis=1)
    # marks: bit d - 1 of an origin corner for each crossing edge of a meshed tetrahedron
    marks = np.zeros(len(corners), np.uint32)
    for (t, m), tris in TABLE.items():
        sel = meshed & (cases[:, t] == m)
        if not tris or not sel.any():
            continue
        for tri in tris:
            for o, d in tri:
                np.bitwise_or.at(marks, idx[sel, o], np.uint32(1 << (d - 1)))
    vcount = POP[marks]
    vbase = np.concatenate([[0], np.cumsum(vcount)[:-1]]).astype(np.int64)
    nv = int(vcount.sum())

    def vid(k, d):
        return vbase[k] + POP[marks[k] & np.uint32((1 << (d - 1)) - 1)]

    verts = np.zeros(nv, VERTEX_DTYPE)
    ends = (Q.empty_rows(nv, rows.dtype), Q.empty_rows(nv, rows.dtype))
    c = lattice_points(corners, bbox, res).astype(np.float64)
    for d in range(1, 8):
        ka = np.flatnonzero(marks >> np.uint32(d - 1) & 1)
        if not len(ka):
            continue
        kb = np.searchsorted(corners, corners[ka] + offset_key(d))
        sa, sb = s[ka].astype(np.float64), s[kb].astype(np.float64)
        t = sa / (sa - sb)
        p = (c[ka] + t[:, None] * (c[kb] - c[ka])).astype(np.float32)
        w = np.where(np.abs(s[kb]) < np.abs(s[ka]), kb, ka)
        r = rws[w]
        v = vid(ka, d)
        verts["x"][v], verts["y"][v], verts["z"][v] = p[:, 0], p[:, 1], p[:, 2]
        for f in ("nx", "ny", "nz", "rgb", "count"):
            verts[f][v] = r[f]
        ends[0][v], ends[1][v] = rws[ka], rws[kb]
    # triangles: per cube (in key order), tetrahedron 0..5, triangle 0..1
    slots = np.full((len(cubes), 6, 2, 3), -1, np.int64)
    for (t, m), tris in TABLE.items():
        sel = np.flatnonzero(meshed & (cases[:, t] == m))
        if not tris or not len(sel):
            continue
        for r, tri in enumerate(tris):
            for j, (o, d) in enumerate(tri):
                slots[sel, t, r, j] = vid(idx[sel, o], d)
    flat = slots.reshape(-1, 3)
    tris = flat[flat[:, 0] >= 0].astype(np.uint32)
    sizes.update(meshed=int(meshed.sum()), defined=int(defined.sum()))
    return (verts, tris, sizes, ends) if with_ends else (verts, tris, sizes)


def cubes_with_a_tied_corner(rows, occupied, bbox, res, dims, radius=2, min_count=0.0, max_distance=np.inf):
    """The number of meshed cubes with a corner sample whose nearest row was decided by the tie rule (query_ref.nearest_ties)."""
    cubes = cube_set(rows, dims, min_count)
    corners = corner_set(cubes)
    if not len(cubes):
        return 0
    pts = lattice_points(corners, bbox, res)
    hits, _ = Q.query(rows, occupied, pts, IDENT, bbox, res, radius=radius, min_count=min_count, max_distance=max_distance)
    tied = Q.nearest_ties(rows, hits, pts, radius, min_count, max_distance)
    idx = np.stack([np.searchsorted(corners, cubes + offset_key(c)) for c in range(8)], axis=1)
    meshed = ((hits["flags"] & Q.FOUND) != 0)[idx].all(axis=1)
    return int((meshed & tied[idx].any(axis=1)).sum())


def mesh_unwelded(rows, occupied, bbox, res, dims, radius=2, min_count=0.0, max_distance=np.inf):
    """Per meshed cube and tetrahedron, each triangle's three positions computed from its own edge's endpoints: (n, 3, 3) f32 in the
    triangle order of mesh(), without any shared vertex numbering."""
    cubes = cube_set(rows, dims, min_count)
    corners = corner_set(cubes)
    if not len(cubes):
        return np.zeros((0, 3, 3), np.float32)
    defined, s, _ = samples(rows, occupied, corners, bbox, res, radius, min_count, max_distance)
    c = lattice_points(corners, bbox, res).astype(np.float64)
    out = []
    for j, ck in enumerate(cubes):
        idx = np.searchsorted(corners, ck + np.array([offset_key(k) for k in range(8)]))
        if not defined[idx].all():
            continue
        inside = s[idx] < 0
        for t, tet in enumerate(TETS):
            m = sum(int(inside[tet[i]]) << i for i in range(4))
            for tri in TABLE[(t, m)]:
                pts = []
                for o, d in tri:
                    a, b = idx[o], idx[o + d]
                    tt = float(s[a]) / (float(s[a]) - float(s[b]))
                    pts.append((c[a] + tt * (c[b] - c[a])).astype(np.float32))
                out.append(pts)
    return np.asarray(out, np.float32).reshape(-1, 3, 3)


def edges(tris):
    """(n * 3, 2) directed edges of the triangles."""
    t = np.asarray(tris, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def edge_use(tris):
    """{undirected edge: (uses, directed uses that cancel)}: per undirected edge its count and whether its uses have opposite
    directions."""
    e = edges(tris)
    lo, hi = np.minimum(e[:, 0], e[:, 1]), np.maximum(e[:, 0], e[:, 1])
    key = lo << 32 | hi
    sign = np.where(e[:, 0] < e[:, 1], 1, -1)
    u, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    net = np.zeros(len(u), np.int64)
    np.add.at(net, inv, sign)
    return u, cnt, net


def euler(n_verts, tris):
    u, _, _ = edge_use(tris)
    used = len(np.unique(np.asarray(tris).reshape(-1)))
    assert used == n_verts, "every vertex is used by a triangle"
    return n_verts - len(u) + len(tris)


def positions(verts):
    return np.stack([verts["x"], verts["y"], verts["z"]], axis=1)


def face_normals(verts, tris):
    p = positions(verts).astype(np.float64)
    t = np.asarray(tris, np.int64)
    return np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
