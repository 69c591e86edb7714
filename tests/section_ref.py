"""The section contract of include/hfpf.h restated in numpy (imported by tests only): a triangle mesh, a pose, planes and the handle's
bounding box -> the points, segments, contours, per-plane records and the summary hfpf_section_mesh* return.  The mesh intake and the
validity rules are deviation_ref's; everything else is f64, one rounding per operation, in the order the header writes it.  The sums
are built with Python integers."""
import numpy as np

import deviation_ref as D

POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("plane", "<u4"), ("va", "<u4"), ("vb", "<u4"), ("contour", "<u4"),
                        ("ends", "<u4")])
SEGMENT_DTYPE = np.dtype([("p0", "<u4"), ("p1", "<u4"), ("tri", "<u4"), ("contour", "<u4")])
CONTOUR_DTYPE = np.dtype([("plane", "<u4"), ("first_point", "<u4"), ("n_points", "<u4"), ("n_segments", "<u4"), ("n_ends", "<u4"),
                          ("flags", "<u4"), ("length_q32", "<i8"), ("area_q28", "<i8"), ("reserved", "<u8")])
PLANE_DTYPE = np.dtype([("first_segment", "<u4"), ("n_segments", "<u4"), ("first_point", "<u4"), ("n_points", "<u4"), ("first_contour", "<u4"),
                        ("n_contours", "<u4"), ("n_closed", "<u4"), ("n_branched", "<u4"), ("length_q32", "<i8"), ("area_q28", "<i8"),
                        ("reserved", "<u8", (2,))])
assert (POINT_DTYPE.itemsize, SEGMENT_DTYPE.itemsize, CONTOUR_DTYPE.itemsize, PLANE_DTYPE.itemsize) == (32, 16, 48, 64)
CLOSED, BRANCHED = 1, 2
MAX_PLANES, MAX_PLANE_SEGMENTS, MAX_VERTS = 4096, 1 << 20, 1 << 26
HEADROOM = 32.0
SUMMARY_KEYS = ("n_tris_valid", "n_tris_invalid", "n_tris_far", "n_segments", "n_points", "n_contours", "n_closed", "reserved")


def cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def classify(verts, stride, tris, pose, bbox, n_verts=None):
    """(V, tris as int64, valid, in_range) of a mesh: the transformed vertices and the triangles' classes."""
    xyz = D.vertex_xyz(verts, stride, n_verts)
    tris = np.asarray(tris, np.uint32).reshape(-1, 3).astype(np.int64)
    A, B, C, _, valid = D.triangles(xyz, tris, pose)
    b = np.asarray(bbox, np.float64)
    c = (b[0::2] + b[1::2]) * 0.5
    with np.errstate(all="ignore"):
        near = np.ones(len(tris), bool)
        for X in (A, B, C):
            near &= (np.abs(X - c) < HEADROOM).all(axis=1)
    return D.transform(xyz, pose), tris, valid, valid & near


def _rint_q(v, bits):
    return [int(x) for x in np.rint(v * 2.0 ** bits)]


def section(verts, stride, tris, pose, planes, bbox, n_verts=None):
    """(points, segments, contours, plane records, summary dict) of a mesh cut by planes ((n, 4) f64: n.x, n.y, n.z, d)."""
    planes = np.asarray(planes, np.float64).reshape(-1, 4)
    V, tris, valid, in_range = classify(verts, stride, tris, pose, bbox, n_verts)
    summary = dict.fromkeys(SUMMARY_KEYS, 0)
    summary.update(n_tris_valid=int(valid.sum()), n_tris_invalid=int((~valid).sum()), n_tris_far=int((valid & ~in_range).sum()))
    T = np.flatnonzero(in_range)
    I = tris[T]  # (m, 3) vertex indices of the in-range triangles
    seg_plane, seg_tri, seg_key0, seg_key1 = [], [], [], []
    for j, (nx, ny, nz, d) in enumerate(planes):
        if len(T) == 0:
            break
        n = np.array([nx, ny, nz])
        s = D.dot(n, V) - d if len(V) else np.zeros(0)
        inside = s[I] < 0  # (m, 3)
        k = inside.sum(axis=1)
        crossing = (k == 1) | (k == 2)
        idx = np.flatnonzero(crossing)
        ins = inside[idx]
        lone_inside = k[idx] == 1
        L = np.where(lone_inside, ins.argmax(axis=1), (~ins).argmax(axis=1))  # the position that differs from the other two
        tri_i = I[idx]
        vL, vN, vP = (tri_i[np.arange(len(idx)), (L + o) % 3] for o in (0, 1, 2))
        key = lambda a, b: (np.minimum(a, b) << 26) | np.maximum(a, b)  # noqa: E731 (plane added below)
        k_prev, k_next = key(vP, vL), key(vL, vN)
        seg_plane.append(np.full(len(idx), j, np.int64))
        seg_tri.append(T[idx])
        seg_key0.append(np.where(lone_inside, k_prev, k_next))
        seg_key1.append(np.where(lone_inside, k_next, k_prev))
    if seg_plane:
        seg_plane, seg_tri, seg_key0, seg_key1 = (np.concatenate(x) for x in (seg_plane, seg_tri, seg_key0, seg_key1))
    else:
        seg_plane = seg_tri = seg_key0 = seg_key1 = np.zeros(0, np.int64)
    ns = len(seg_plane)
    # 52-bit edge keys under the plane: Python-sized integers are not needed, 12 + 52 bits fit a uint64
    full0 = (seg_plane.astype(np.uint64) << np.uint64(52)) | seg_key0.astype(np.uint64)
    full1 = (seg_plane.astype(np.uint64) << np.uint64(52)) | seg_key1.astype(np.uint64)
    ukeys, inv = np.unique(np.concatenate([full0, full1]), return_inverse=True)
    p0, p1 = inv[:ns], inv[ns:]
    npnt = len(ukeys)
    pl = (ukeys >> np.uint64(52)).astype(np.int64)
    va = ((ukeys >> np.uint64(26)) & np.uint64((1 << 26) - 1)).astype(np.int64)
    vb = (ukeys & np.uint64((1 << 26) - 1)).astype(np.int64)
    points = np.zeros(npnt, POINT_DTYPE)
    P = np.zeros((npnt, 3))
    if npnt:
        nrm, dd = planes[pl, :3], planes[pl, 3]
        sa, sb = D.dot(nrm, V[va]) - dd, D.dot(nrm, V[vb]) - dd
        t = sa / (sa - sb)
        P = V[va] + t[:, None] * (V[vb] - V[va])
        points["x"], points["y"], points["z"] = (P[:, a].astype(np.float32) for a in range(3))
        points["plane"], points["va"], points["vb"] = pl, va, vb
    # contours: union-find by the smallest point
    parent = np.arange(npnt)
    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(p0.tolist(), p1.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(x) for x in range(npnt)], np.int64)
    reps = np.flatnonzero(root == np.arange(npnt))
    label = np.zeros(npnt, np.int64)
    label[reps] = np.arange(len(reps))
    cont_of_point = label[root] if npnt else np.zeros(0, np.int64)
    n_out, n_in = np.bincount(p0, minlength=npnt), np.bincount(p1, minlength=npnt)
    points["contour"] = cont_of_point
    points["ends"] = np.minimum(n_out, 65535) | (np.minimum(n_in, 65535) << 16)
    segments = np.zeros(ns, SEGMENT_DTYPE)
    segments["p0"], segments["p1"], segments["tri"] = p0, p1, seg_tri
    seg_cont = cont_of_point[p0] if ns else np.zeros(0, np.int64)
    segments["contour"] = seg_cont
    nc = len(reps)
    contours = np.zeros(nc, CONTOUR_DTYPE)
    contours["plane"], contours["first_point"] = pl[reps], reps
    contours["n_points"] = np.bincount(cont_of_point, minlength=nc)
    contours["n_segments"] = np.bincount(seg_cont, minlength=nc)
    contours["n_ends"] = np.bincount(cont_of_point[(n_in + n_out) == 1], minlength=nc)
    is_open = np.bincount(cont_of_point[~((n_in == 1) & (n_out == 1))], minlength=nc) > 0
    branched = np.bincount(cont_of_point[(n_in > 1) | (n_out > 1)], minlength=nc) > 0
    contours["flags"] = np.where(is_open, 0, CLOSED) | np.where(branched, BRANCHED, 0)
    length, area = [0] * nc, [0] * nc
    if ns:
        P0, P1 = P[p0], P[p1]
        e = P1 - P0
        lq = _rint_q(np.sqrt(D.dot(e, e)), 32)
        Pr = P[reps[seg_cont]]
        nrm = planes[seg_plane, :3]
        U = nrm / np.sqrt(D.dot(nrm, nrm))[:, None]
        aq = _rint_q(0.5 * D.dot(U, cross(P0 - Pr, P1 - Pr)), 28)
        for c, l, a in zip(seg_cont.tolist(), lq, aq):
            length[c] += l
            area[c] += a
    contours["length_q32"], contours["area_q28"] = length, area
    recs = np.zeros(len(planes), PLANE_DTYPE)
    recs["n_segments"] = np.bincount(seg_plane, minlength=len(planes))
    recs["n_points"] = np.bincount(pl, minlength=len(planes))
    cp = contours["plane"].astype(np.int64)
    closed = (contours["flags"] & CLOSED) != 0
    recs["n_contours"] = np.bincount(cp, minlength=len(planes))
    recs["n_closed"] = np.bincount(cp[closed], minlength=len(planes))
    recs["n_branched"] = np.bincount(cp[(contours["flags"] & BRANCHED) != 0], minlength=len(planes))
    pl_len, pl_area = [0] * len(planes), [0] * len(planes)
    for c in range(nc):
        pl_len[cp[c]] += length[c]
        if closed[c]:
            pl_area[cp[c]] += area[c]
    recs["length_q32"], recs["area_q28"] = pl_len, pl_area
    for first, count in (("first_segment", "n_segments"), ("first_point", "n_points"), ("first_contour", "n_contours")):
        recs[first] = np.concatenate([[0], np.cumsum(recs[count].astype(np.int64))[:-1]]) if len(planes) else 0
    assert (recs["n_segments"] <= MAX_PLANE_SEGMENTS).all(), "a plane beyond the cap: the call returns HFPF_ERR_CAPACITY"
    summary.update(n_segments=ns, n_points=npnt, n_contours=nc, n_closed=int(closed.sum()))
    return points, segments, contours, recs, summary
