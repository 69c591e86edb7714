"""The coverage contract of include/hfpf.h restated in numpy (imported by tests only): hfpf_extract's rows, hfpf_get_occupied's list, a
triangle mesh, a pose and the options -> the per-triangle records and the summary hfpf_cover_mesh* return.  The mesh intake and the
validity rules are deviation_ref's, the sample test is query_ref.query under the identity pose; everything else is f64, one rounding
per operation, in the order the header writes it.  The summary is built with Python integers."""
import numpy as np

import deviation_ref as D
import query_ref as Q

TRI_COVERAGE_DTYPE = np.dtype([("n_samples", "<u4"), ("n_in_bbox", "<u4"), ("n_covered", "<u4"), ("flags", "<u4"), ("area", "<f4"),
                               ("max_distance", "<f4"), ("sum_dist_q30", "<i8")])
assert TRI_COVERAGE_DTYPE.itemsize == 32
VALID, CAPPED, HUGE = 1, 2, 4
ABS_NORMAL = 1
SUMMARY_KEYS = ("n_tris_valid", "n_tris_invalid", "n_tris_huge", "n_samples", "n_in_bbox", "n_covered", "sum_dist_q30", "area_q40_lo",
                "area_q40_hi", "covered_q40_lo", "covered_q40_hi", "max_distance", "pad")
IDENT = np.eye(4)[:3]


def subdivision(L2, spacing, max_subdivision):
    """(n, capped) per triangle from the longest edge squared."""
    with np.errstate(all="ignore"):
        q = np.sqrt(np.asarray(L2, np.float64)) / float(spacing)
        n = np.where(~(q > 1.0), 1.0, np.where(q >= max_subdivision, float(max_subdivision), np.ceil(q)))
    return n.astype(np.uint32), q > max_subdivision


def sub_triangles(n):
    """(i, j, kind) of the n^2 sub-triangles: the upright ones, then the inverted ones."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    up, inv = (i + j) <= n - 1, (i + j) <= n - 2
    return (np.concatenate([i[up], i[inv]]), np.concatenate([j[up], j[inv]]),
            np.concatenate([np.zeros(int(up.sum()), np.int64), np.ones(int(inv.sum()), np.int64)]))


def barycentric(n):
    """(v, w) of the n^2 samples, in sub_triangles' order."""
    i, j, kind = sub_triangles(n)
    return (3 * i + 1 + kind).astype(np.float64) / float(3 * n), (3 * j + 1 + kind).astype(np.float64) / float(3 * n)


def sample_points(A, ab, ac, n):
    """(tri, S) of every sample of the triangles whose n is > 0: tri = its position in A, S = (A + v*ab) + w*ac, f64."""
    tri, S = [], []
    for m in np.unique(n[n > 0]):
        at = np.flatnonzero(n == m)
        v, w = barycentric(int(m))
        S.append(((A[at, None, :] + v[None, :, None] * ab[at, None, :]) + w[None, :, None] * ac[at, None, :]).reshape(-1, 3))
        tri.append(np.repeat(at, len(v)))
    if not tri:
        return np.zeros(0, np.int64), np.zeros((0, 3))
    return np.concatenate(tri), np.concatenate(S)


def geometry(verts, stride, tris, pose, n_verts=None):
    """(A, ab, ac, N, NN, L2, valid) of every triangle; zeros for an invalid one."""
    A, B, C, N, valid = D.triangles(D.vertex_xyz(verts, stride, n_verts), tris, pose)
    with np.errstate(all="ignore"):
        ab, ac, bc = B - A, C - A, C - B
        NN = D.dot(N, N)
        L2 = np.maximum(D.dot(ab, ab), np.maximum(D.dot(ac, ac), D.dot(bc, bc)))
    z = ~valid
    for a in (A, ab, ac, N):
        a[z] = 0.0
    NN, L2 = np.where(valid, NN, 0.0), np.where(valid, L2, 0.0)
    return A, ab, ac, N, NN, L2, valid


def records(n, capped, NN, valid, tri, in_bbox, covered, distance):
    """The per-triangle records from the per-sample results (tri = the sample's triangle, distance f32)."""
    cov = np.zeros(len(valid), TRI_COVERAGE_DTYPE)
    with np.errstate(all="ignore"):
        area_d = 0.5 * np.sqrt(NN)
    cov["n_samples"] = np.where(valid, n.astype(np.uint64) * n, 0)
    cov["flags"] = np.where(valid, VALID | np.where(capped, CAPPED, 0) | np.where(~(area_d < 2.0 ** 23), HUGE, 0), 0)
    cov["area"] = np.where(valid, area_d, 0.0).astype(np.float32)
    cov["n_in_bbox"] = np.bincount(tri[in_bbox], minlength=len(valid))
    cov["n_covered"] = np.bincount(tri[covered], minlength=len(valid))
    d = distance[covered]
    np.add.at(cov["sum_dist_q30"], tri[covered], np.rint(d.astype(np.float64) * 2.0 ** 30).astype(np.int64))
    np.maximum.at(cov["max_distance"].view(np.uint32), tri[covered], d.view(np.uint32))
    return cov, area_d


def summary(cov, area_d):
    """hfpf_coverage_summary of the records, with Python integers (area_d = 0.5 * sqrt(NN) per triangle, f64)."""
    valid = (cov["flags"] & VALID) != 0
    s = dict(n_tris_valid=int(valid.sum()), n_tris_invalid=int((~valid).sum()), n_tris_huge=int(((cov["flags"] & HUGE) != 0).sum()),
             n_samples=sum(int(x) for x in cov["n_samples"]), n_in_bbox=sum(int(x) for x in cov["n_in_bbox"]),
             n_covered=sum(int(x) for x in cov["n_covered"]), sum_dist_q30=sum(int(x) for x in cov["sum_dist_q30"]),
             area_q40_lo=0, area_q40_hi=0, covered_q40_lo=0, covered_q40_hi=0,
             max_distance=float(cov["max_distance"].max()) if len(cov) else 0.0, pad=0)
    for k in np.flatnonzero(valid & ((cov["flags"] & HUGE) == 0)):
        a = float(area_d[k])
        ta = int(np.rint(a * 2.0 ** 40))
        tc = int(np.rint(((a * float(cov["n_covered"][k])) / float(cov["n_samples"][k])) * 2.0 ** 40))
        s["area_q40_lo"] += ta & 0xFFFFFFFF
        s["area_q40_hi"] += ta >> 32
        s["covered_q40_lo"] += tc & 0xFFFFFFFF
        s["covered_q40_hi"] += tc >> 32
    return s


def normal_gate(N, NN, tri, normals, min_normal_dot, abs_normal):
    """Per sample: the gate on c = dot(N, n) against min_normal_dot * sqrt(NN) (normals: the found row's, f64)."""
    if float(min_normal_dot) == -2.0:
        return np.ones(len(tri), bool)
    with np.errstate(all="ignore"):
        c = (N[tri, 0] * normals[:, 0] + N[tri, 1] * normals[:, 1]) + N[tri, 2] * normals[:, 2]
        bound = float(min_normal_dot) * np.sqrt(NN[tri])
        return (c >= bound) | (bool(abs_normal) & (np.abs(c) >= bound))


def cover(rows, occupied, verts, stride, tris, pose, bbox, res, radius=2, min_count=0.0, max_distance=0.01, spacing=0.005,
          max_subdivision=64, min_normal_dot=-2.0, abs_normal=False, n_verts=None):
    """(records of TRI_COVERAGE_DTYPE, summary dict) as hfpf_cover_mesh returns them for these rows and this occupied list."""
    A, ab, ac, N, NN, L2, valid = geometry(verts, stride, tris, pose, n_verts)
    n, capped = subdivision(L2, spacing, max_subdivision)
    n = np.where(valid, n, 0).astype(np.uint32)
    tri, S = sample_points(A, ab, ac, n)
    with np.errstate(all="ignore"):
        p = S.astype(np.float32)
    hits, hrows = Q.query(rows, occupied, p, IDENT, bbox, res, radius=radius, min_count=min_count, max_distance=max_distance)
    in_bbox = (hits["flags"] & Q.IN_BBOX) != 0
    found = (hits["flags"] & Q.FOUND) != 0
    normals = np.stack([hrows[k].astype(np.float64) for k in ("nx", "ny", "nz")], axis=1)
    covered = found & normal_gate(N, NN, tri, normals, min_normal_dot, abs_normal)
    cov, area_d = records(n, capped, NN, valid, tri, in_bbox, covered, hits["distance"])
    return cov, summary(cov, area_d)
