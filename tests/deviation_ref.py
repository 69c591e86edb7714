"""The deviation contract of include/hfpf.h restated in numpy (imported by tests only): hfpf_extract_filtered's rows, a triangle mesh,
a pose and the options -> the per-row records and the summary hfpf_compare_mesh* return.  Everything is f64, one rounding per
operation, in the order the header writes it.

compare() may prune: it finds each row's candidates through a uniform grid of cells as wide as a search radius r, lists a triangle
in the cells its box inflated by r and a margin reaches, first with a small r (max_distance / 8, or a typical triangle's size if that is larger), then with r = max_distance for
the rows still without an answer.  A row whose best candidate has dd <= r^2 is final: every triangle with dd <= r^2 is among the candidates, so what
was pruned has a larger dd.  tests/test_deviation_ref.py holds the pruned form against the plain double loop."""
import numpy as np

from components_ref import ROW_DTYPE, count_gate

DEVIATION_DTYPE = np.dtype([("signed_distance", "<f4"), ("distance", "<f4"), ("tri", "<u4"), ("flags", "<u4"), ("q", "<f4", (3,)),
                            ("reserved", "<u4")])
assert DEVIATION_DTYPE.itemsize == 32
FOUND, ON_EDGE, ON_VERTEX = 1, 2, 4
NAN_BITS = 0x7FC00000
NO_TRI = 0xFFFFFFFF
SUMMARY_KEYS = ("n_rows", "n_found", "n_negative", "n_tris_valid", "n_tris_invalid", "max_abs", "pad", "sum_abs_q30", "sum_sq_q30")
PAIR_CHUNK = 1 << 20


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def closest_point(P, A, B, C):
    """The seven-region construction on f64 arrays of shape (..., 3) (or single points): (Q, region, dd) with region = ON_VERTEX,
    ON_EDGE or 0 for the face.  Every quantity is computed for every element and the branches select in the contract's order, which
    gives each element exactly the operations of its own branch."""
    P, A, B, C = (np.asarray(a, np.float64) for a in (P, A, B, C))
    with np.errstate(all="ignore"):
        ab, ac = B - A, C - A
        ap = P - A
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = P - B
        d3, d4 = dot(ab, bp), dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = P - C
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e, f = d4 - d3, d5 - d6
        s = (va + vb) + vc
        v, w = vb / s, vc / s
        q_face = (A + v[..., None] * ab) + w[..., None] * ac
        q_ab = A + (d1 / (d1 - d3))[..., None] * ab
        q_ac = A + (d2 / (d2 - d6))[..., None] * ac
        q_bc = B + (e / (e + f))[..., None] * (C - B)
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e >= 0) & (f >= 0)]
        picks = [(A, ON_VERTEX), (B, ON_VERTEX), (q_ab, ON_EDGE), (C, ON_VERTEX), (q_ac, ON_EDGE), (q_bc, ON_EDGE)]
        Q = q_face
        region = np.zeros(np.shape(d1), np.uint32)
        for cond, (q, flag) in reversed(list(zip(conds, picks))):
            Q = np.where(cond[..., None], np.broadcast_to(q, Q.shape), Q)
            region = np.where(cond, np.uint32(flag), region)
        r = P - Q
        dd = dot(r, r)
    return Q, region, dd


def vertex_xyz(verts, stride, n_verts=None):
    """(n, 3) float32 view-or-copy of the x, y, z of vertices `stride` bytes apart in verts (any array or bytes-like)."""
    raw = np.frombuffer(np.ascontiguousarray(verts).tobytes(), np.uint8)
    n = (len(raw) - 12) // stride + 1 if n_verts is None and len(raw) >= 12 else (n_verts or 0)
    if n == 0:
        return np.zeros((0, 3), np.float32)
    return np.lib.stride_tricks.as_strided(raw[:(n - 1) * stride + 12].view(np.uint8), shape=(n, 12), strides=(stride, 1)).copy().view("<f4")


def transform(xyz, pose):
    """V[a] = ((T[4a]*x + T[4a+1]*y) + T[4a+2]*z) + T[4a+3], x, y, z widened; f64."""
    T = np.asarray(pose, np.float64).reshape(3, 4)
    x, y, z = (xyz[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1)


def triangles(xyz, tris, pose):
    """(A, B, C, N, valid) of every triangle; the coordinates of an invalid one are zeros."""
    tris = np.asarray(tris, np.uint32).reshape(-1, 3).astype(np.int64)
    V = transform(xyz, pose)
    in_range = (tris < len(V)).all(axis=1)
    idx = np.where(in_range[:, None], tris, 0)
    if len(V) == 0:
        V = np.zeros((1, 3))
    A, B, C = (np.where(in_range[:, None], V[idx[:, k]], 0.0) for k in range(3))
    with np.errstate(all="ignore"):
        ab, ac = B - A, C - A
        N = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2], ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]],
                     axis=1)
        NN = dot(N, N)
    valid = in_range & np.isfinite(A).all(axis=1) & np.isfinite(B).all(axis=1) & np.isfinite(C).all(axis=1) & np.isfinite(NN) & (NN > 0)
    return A, B, C, N, valid


def _best_of_pairs(P, tri_geo, row_of, tri_of, md2):
    """Per row index in row_of: the smallest (dd, tri) among its pairs with dd <= md2.  Returns sorted unique rows, dd, tri, Q, region, neg."""
    A, B, C, N = tri_geo
    out = []
    for c0 in range(0, len(row_of), PAIR_CHUNK):
        r, t = row_of[c0:c0 + PAIR_CHUNK], tri_of[c0:c0 + PAIR_CHUNK]
        Q, region, dd = closest_point(P[r], A[t], B[t], C[t])
        keep = dd <= md2
        r, t, Q, region, dd = r[keep], t[keep], Q[keep], region[keep], dd[keep]
        order = np.lexsort((t, dd, r))
        first = np.ones(len(order), bool)
        first[1:] = r[order][1:] != r[order][:-1]
        sel = order[first]
        neg = dot(N[t[sel]], P[r[sel]] - Q[sel]) < 0
        out.append((r[sel], dd[sel], t[sel], Q[sel], region[sel], neg))
    if not out:
        z = np.zeros(0, np.int64)
        return z, np.zeros(0), z, np.zeros((0, 3)), np.zeros(0, np.uint32), np.zeros(0, bool)
    r, dd, t, Q, region, neg = (np.concatenate(x) for x in zip(*out))
    order = np.lexsort((t, dd, r))  # a row's pairs may straddle chunks
    first = np.ones(len(order), bool)
    first[1:] = r[order][1:] != r[order][:-1]
    sel = order[first]
    return r[sel], dd[sel], t[sel], Q[sel], region[sel], neg[sel]


def _candidate_pairs(P, rows_left, tri_geo, tri_ids, radius, cell_size):
    """(row, triangle) pairs that contain every pair with computed dd <= radius^2, rows from rows_left, triangles from tri_ids.  The
    margin: dd <= r^2 puts P within r (1 + 2^-50) of the computed Q per axis; the computed Q leaves the box of A, B, C by at most
    2^-50 M on an edge region (M = the largest |coordinate|) and, to first order, by 224 * 2^-53 L^3 D^2 / NN on the face region (L the
    longest edge, D a bound on |P - vertex|); four times that is taken (for a tiny sliver it can be millimetres: the box is inflated by
    it all the same), and a triangle for which it exceeds max(8 radius, 2 cm) meets every row.
    cell_size (any positive width: floor(x / cell_size) is monotone) only sets how many cells a triangle is listed in."""
    A, B, C, N = (g[tri_ids] for g in tri_geo)
    Pl = P[rows_left]
    with np.errstate(all="ignore"):
        M = np.maximum(np.abs(A), np.maximum(np.abs(B), np.abs(C))).max(axis=1)
        L2 = np.maximum(dot(B - A, B - A), np.maximum(dot(C - A, C - A), dot(C - B, C - B)))
        D = 2.0 * (np.abs(Pl).max() + M + radius)
        face = 2.0 ** -43 * (L2 * np.sqrt(L2)) * (D * D) / dot(N, N)
    everywhere = ~(face <= max(8.0 * radius, 0.02))
    infl = np.where(everywhere, 0.0, (radius * (1.0 + 2.0 ** -40) + face) + 2.0 ** -49 * (M + radius))
    big_int = 2.0 ** 62
    lo = np.clip(np.floor((np.minimum(A, np.minimum(B, C)) - infl[:, None]) / cell_size), -big_int, big_int).astype(np.int64)
    hi = np.clip(np.floor((np.maximum(A, np.maximum(B, C)) + infl[:, None]) / cell_size), -big_int, big_int).astype(np.int64)
    cell = np.floor(Pl / cell_size).astype(np.int64)
    base = cell.min(axis=0)
    span = cell.max(axis=0) - base + 1
    outside = ((hi < base) | (lo > base + span - 1)).any(axis=1) & ~everywhere  # reaches no cell that holds a row
    lo, hi = np.clip(lo - base, 0, span - 1), np.clip(hi - base, 0, span - 1)
    cell -= base
    key = (cell[:, 0] * span[1] + cell[:, 1]) * span[2] + cell[:, 2]
    order = np.argsort(key, kind="stable")
    ukey, ustart, ucount = np.unique(key[order], return_index=True, return_counts=True)
    ext = hi - lo + 1
    vol = ext.prod(axis=1)
    vol[outside] = 0
    big = everywhere | (vol > len(ukey))
    pc_tri, pc_cell = [], []  # (triangle position, index into ukey)
    small = np.flatnonzero(~big & (vol > 0))
    if len(small):
        v = vol[small]
        t = np.repeat(small, v)
        i = np.arange(v.sum()) - np.repeat(np.cumsum(v) - v, v)
        ez, ey = ext[t, 2], ext[t, 1]
        k = ((lo[t, 0] + i // (ez * ey)) * span[1] + lo[t, 1] + (i // ez) % ey) * span[2] + lo[t, 2] + i % ez
        at = np.searchsorted(ukey, k)
        ok = (at < len(ukey)) & (ukey[np.minimum(at, len(ukey) - 1)] == k)
        pc_tri.append(t[ok]), pc_cell.append(at[ok])
    ucell = np.stack([ukey // (span[1] * span[2]), (ukey // span[2]) % span[1], ukey % span[2]], axis=1)
    for t in np.flatnonzero(big):
        inside = np.ones(len(ukey), bool) if everywhere[t] else ((ucell >= lo[t]) & (ucell <= hi[t])).all(axis=1)
        at = np.flatnonzero(inside)
        pc_tri.append(np.full(len(at), t, np.int64)), pc_cell.append(at)
    if not pc_tri:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    pt, pcell = np.concatenate(pc_tri), np.concatenate(pc_cell)
    n = ucount[pcell]
    tri_pos = np.repeat(pt, n)
    j = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
    row_pos = order[np.repeat(ustart[pcell], n) + j]
    return rows_left[row_pos], tri_ids[tri_pos]


def compare(rows, verts, stride, tris, pose, min_count, max_distance, n_verts=None, prune=True):
    """(dev of DEVIATION_DTYPE, one per gated row; summary dict) as hfpf_compare_mesh returns them for these rows."""
    rows = np.asarray(rows)[count_gate(rows, min_count)]
    n = len(rows)
    P = np.stack([rows[k].astype(np.float64) for k in ("x", "y", "z")], axis=1) if n else np.zeros((0, 3))
    A, B, C, N, valid = triangles(vertex_xyz(verts, stride, n_verts), tris, pose)
    geo = (A, B, C, N)
    md = float(max_distance)
    md2 = md * md
    tri_ids = np.flatnonzero(valid)
    best_dd = np.full(n, np.inf)
    best_tri = np.full(n, -1, np.int64)
    best_q = np.zeros((n, 3))
    best_region = np.zeros(n, np.uint32)
    best_neg = np.zeros(n, bool)

    def take(res):
        r, dd, t, Q, region, neg = res
        best_dd[r], best_tri[r], best_q[r], best_region[r], best_neg[r] = dd, t, Q, region, neg

    if n and len(tri_ids):
        if not prune:
            for r0 in range(0, n, 256):
                r = np.repeat(np.arange(r0, min(n, r0 + 256)), len(tri_ids))
                take(_best_of_pairs(P, geo, r, np.tile(tri_ids, min(n, r0 + 256) - r0), md2))
        else:
            left = np.arange(n)
            with np.errstate(all="ignore"):  # cells no narrower than a typical triangle, so that one is listed in a few of them
                ext = (np.maximum(A, np.maximum(B, C)) - np.minimum(A, np.minimum(B, C)))[tri_ids].max(axis=1)
            typical = float(np.median(ext[np.isfinite(ext)])) if np.isfinite(ext).any() else 0.0
            for radius in (min(md, max(md / 8, typical)), md):
                if not len(left):
                    break
                r, t = _candidate_pairs(P, left, geo, tri_ids, radius, max(radius, typical))
                res = _best_of_pairs(P, geo, r, t, md2)
                final = res[1] <= radius * radius if radius < md else np.ones(len(res[0]), bool)
                take(tuple(x[final] for x in res))
                left = left[best_tri[left] < 0]
    dev = np.zeros(n, DEVIATION_DTYPE)
    found = best_tri >= 0
    nan = np.array([NAN_BITS], np.uint32).view(np.float32)[0]
    with np.errstate(all="ignore"):
        dist = np.sqrt(np.where(found, best_dd, 0.0)).astype(np.float32)
    dev["distance"] = np.where(found, dist, nan)
    dev["signed_distance"] = np.where(found, np.where(best_neg, -dist, dist), nan)
    dev["tri"] = np.where(found, best_tri, NO_TRI).astype(np.uint32)
    dev["flags"] = np.where(found, FOUND | best_region, 0).astype(np.uint32)
    dev["q"] = np.where(found[:, None], best_q.astype(np.float32), nan)
    # NaN must be the quiet NaN of the contract, bit for bit
    for name in ("distance", "signed_distance"):
        dev[name].view(np.uint32)[~found] = NAN_BITS
    dev["q"].view(np.uint32)[~found] = NAN_BITS
    s = summary(dev)
    s["n_tris_valid"], s["n_tris_invalid"] = int(valid.sum()), int(len(valid) - valid.sum())
    return dev, s


def summary(dev):
    """The row part of hfpf_deviation_summary rebuilt from the per-row output (the triangle counts are 0 here)."""
    found = (dev["flags"] & FOUND) != 0
    d = dev["distance"][found].astype(np.float64)
    return dict(n_rows=len(dev), n_found=int(found.sum()), n_negative=int((dev["signed_distance"][found] < 0).sum()), n_tris_valid=0,
                n_tris_invalid=0, max_abs=float(dev["distance"][found].max()) if found.any() else 0.0, pad=0,
                sum_abs_q30=int(np.rint(d * 2.0 ** 30).astype(np.int64).sum()), sum_sq_q30=int(np.rint((d * d) * 2.0 ** 30).astype(np.int64).sum()))
