"""What the section tests share (imported by tests only): the small meshes, the planes, the device form's helper and the byte-for-byte
comparator.  No test and no fixture is defined here, and every assertion carries its message.  Nothing here needs a GPU."""
import numpy as np

import section_ref as X

BBOX = (-0.5, 0.5, -0.5, 0.5, 0.0, 1.0)  # the default box of the GPU tests (scenes.BBOX_1M)
IDENT = np.eye(4)[:3]
SPHERE = ((0.05, 0.0, 0.45), 0.10)                   # the synthetic scene's sphere and box (plan_support)
BOX = ((-0.20, -0.08), (-0.10, 0.10), (0.40, 0.60))
Q32, Q28 = 1 << 32, 1 << 28
NAMES = ("points", "segments", "contours", "planes")


def cube(lo=(-0.5, -0.5, 0.0), side=1.0):
    """The cube of `side` with its low corner at lo, 8 vertices and 12 triangles wound outwards (vertex index = 4x + 2y + z)."""
    corners = np.array([[lo[0] + side * x, lo[1] + side * y, lo[2] + side * z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]  # -x, +x, -y, +y, -z, +z seen from outside
    return corners, np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.uint32)


def outward(verts, tris, centre):
    """True per triangle whose winding normal points away from centre."""
    P0, P1, P2 = (verts[tris[:, k]].astype(np.float64) for k in range(3))
    return np.einsum("ij,ij->i", np.cross(P1 - P0, P2 - P0), (P0 + P1 + P2) / 3 - np.asarray(centre)) > 0


def fan(n=3):
    """n triangles around the edge (0, 1) on the z axis, each wound 0 -> 1 -> its own third vertex: a non-manifold edge."""
    a = 2 * np.pi * np.arange(n) / n
    verts = np.concatenate([[[0, 0, 0.2], [0, 0, 0.8]], np.stack([0.3 * np.cos(a), 0.3 * np.sin(a), np.full(n, 0.5)], axis=1)]).astype(np.float32)
    return verts, np.array([[0, 1, 2 + i] for i in range(n)], np.uint32)


def bow():
    """Two triangles on the edge (0, 1) wound the same way along it (0 -> 1 in both): their windings disagree across the edge."""
    verts = np.array([[0, 0, 0.2], [0, 0, 0.8], [0.3, 0, 0.5], [-0.3, 0, 0.5]], np.float32)
    return verts, np.array([[0, 1, 2], [0, 1, 3]], np.uint32)


def unweld(verts, tris):
    """The same triangles as a soup: every triangle gets three vertices of its own."""
    return np.ascontiguousarray(verts[tris.reshape(-1)]), np.arange(3 * len(tris), dtype=np.uint32).reshape(-1, 3)


# plan_support.sphere_and_box() repeats one point per pole under `slices` indices, so the valid triangles next to a pole are welded
# to nobody (welding follows indices) and a section through them is open.  They lie within 2 r sin(pi / 48) = 0.0131 m of their
# pole: a plane farther than CAP from both poles meets the closed part of the sphere only.
CAP = 0.015
POLES = np.array([[SPHERE[0][0], SPHERE[0][1] + s * SPHERE[1], SPHERE[0][2]] for s in (1.0, -1.0)])


def parallel_planes(n, pitch=0.0025, lo=-0.0817):
    """n <= 64 + 1 planes normal to y, `pitch` apart from lo up: they stay between the polar caps of the sphere (|y| < 0.1 - CAP)
    and inside the box (|y| < 0.1).  Plane 5 (when there is one) lies at y = 0.2 and misses everything.  One plane: the first.
    The planes of a smaller n are the first planes of a larger one."""
    p = np.zeros((n, 4))
    p[:, 1], p[:, 3] = 1.0, lo + pitch * np.arange(n)
    if n > 5:
        p[5, 3] = 0.2
    assert (np.abs(np.abs(p[:, 3]) - SPHERE[1]) > CAP).all(), "no plane meets a polar cap"
    return p


def mixed_planes(n=65, seed=0x5EC7):
    """n planes of seeded orientation through seeded points around the sphere and the box, none within CAP of a pole of the sphere;
    plane 7 misses everything; the normals are not unit vectors."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        nrm = rng.normal(size=3) * rng.uniform(0.1, 5.0)
        through = np.array([-0.05, 0.0, 0.48]) + rng.uniform(-0.12, 0.12, 3)
        d = float(nrm @ through)
        if (np.abs(POLES @ nrm - d) / np.linalg.norm(nrm) > CAP).all():
            out.append([*nrm, d])
    p = np.array(out)
    p[7] = (0.0, 0.0, 1.0, 0.95)
    return p


def soup(n=832, seed=0x5EC0, res=0.002, centre=(0.0, 0.0, 0.5)):
    """A seeded soup near the box centre: n triangles (13 waves of 64) 0.2 to 40 voxels across with vertices of their own; 78
    invalid in three ways (an index out of range, a NaN vertex, a repeated vertex) and 20 with a vertex 40 m away."""
    rng = np.random.default_rng(seed)
    c = np.asarray(centre) + rng.uniform(-0.03, 0.03, (n, 3))
    edge = res * np.exp(rng.uniform(np.log(0.2), np.log(40.0), (n, 1, 1)))
    verts = (c[:, None, :] + rng.uniform(-0.5, 0.5, (n, 3, 3)) * edge).reshape(-1, 3).astype(np.float32)
    tris = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    kinds = rng.permutation(n)[:98]
    bad, far = kinds[:78].reshape(3, 26), kinds[78:]
    tris[bad[0][:13], 2] = 3 * n + rng.integers(0, 1000, 13)
    tris[bad[0][13:], 0] = 0xFFFFFFFF
    verts[tris[bad[1], 1], 2] = np.nan
    tris[bad[2], 1] = tris[bad[2], 0]
    verts[tris[far, 2], 0] += 40.0
    return verts, tris


def soup_planes():
    """Five planes through the soup: three axis planes through its centre, two oblique."""
    return np.array([[1.0, 0, 0, 0.001], [0, 1.0, 0, -0.002], [0, 0, 2.0, 1.001], [1.0, 1.0, 1.0, 0.503], [-0.3, 0.8, 0.5, 0.247]])


def strip(n, x0=-0.25, pitch=2.0 ** -22, half=0.25):
    """n triangles in a row along x, each with its base below the plane y = 0 and its apex above it: all cross the plane, each
    segment has the closed-form length pitch / 2 (the coordinates and the pitch are dyadic, so that is exact)."""
    i = np.arange(n, dtype=np.float64)
    base = x0 + pitch * i
    verts = np.stack([np.stack([base, np.full(n, -half), np.full(n, 0.5)], 1), np.stack([base + pitch, np.full(n, -half), np.full(n, 0.5)], 1),
                      np.stack([base + pitch / 2, np.full(n, half), np.full(n, 0.5)], 1)], axis=1).reshape(-1, 3).astype(np.float32)
    assert (verts.astype(np.float64).reshape(n, 3, 3)[:, 0, 0] == base).all(), "the strip's coordinates are exact in f32"
    return verts, np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def rigid(angle, axis, shift):
    """A 3x4 pose: the rotation by `angle` about `axis`, then `shift`."""
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    return np.hstack([R, np.asarray(shift, np.float64).reshape(3, 1)])


def reference(verts, tris, pose, planes, bbox=BBOX, stride=None, n_verts=None):
    verts = np.ascontiguousarray(verts)
    stride = stride if stride is not None else (verts.dtype.itemsize if verts.dtype.names else 12)
    return X.section(verts, stride, tris, pose, planes, bbox, n_verts)


def same_section(got, ref, what):
    """(points, segments, contours, plane records, summary) byte for byte, with the first differing record of the first array that
    differs."""
    for name, a, b in zip(NAMES, got[:4], ref[:4]):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype.itemsize == b.dtype.itemsize and len(a) == len(b), "%s: %d %s of %d bytes vs %d of %d" % (what, len(a), name, a.dtype.itemsize, len(b),
                                                                                                                   b.dtype.itemsize)
        if a.tobytes() != b.tobytes():
            x, y = a.view(np.uint8).reshape(len(a), -1), b.view(np.uint8).reshape(len(b), -1)
            bad = np.flatnonzero((x != y).any(axis=1))
            raise AssertionError("%s: %d of %d %s differ, first %d: %r vs %r" % (what, bad.size, len(a), name, int(bad[0]), a[bad[0]], b[bad[0]]))
    for k in X.SUMMARY_KEYS:
        assert got[4][k] == ref[4][k], "%s: summary %s: %r vs %r" % (what, k, got[4][k], ref[4][k])


def consistent(points, segments, contours, recs, summary):
    """What holds for every section: the arrays add up, ids are in order, every record names what it belongs to."""
    assert summary["n_points"] == len(points) and summary["n_segments"] == len(segments) and summary["n_contours"] == len(contours), "the counts"
    assert summary["n_closed"] == int(((contours["flags"] & X.CLOSED) != 0).sum()) == int(recs["n_closed"].sum()), "closed contours"
    for first, count, total in (("first_segment", "n_segments", len(segments)), ("first_point", "n_points", len(points)),
                                ("first_contour", "n_contours", len(contours))):
        assert int(recs[count].sum()) == total and (recs[first] == np.concatenate([[0], np.cumsum(recs[count])[:-1]])[:len(recs)]).all(), first
    assert (np.diff(points["plane"].astype(np.int64)) >= 0).all() and (points["va"] < points["vb"]).all(), "points in (plane, va, vb) order"
    key = (points["plane"][segments["p0"]].astype(np.int64) << 32) | segments["tri"].astype(np.int64)
    assert (np.diff(key) > 0).all(), "segments in (plane, triangle) order"
    assert (points["contour"][segments["p0"]] == segments["contour"]).all() and (points["contour"][segments["p1"]] == segments["contour"]).all(), "labels"
    assert (points["contour"][contours["first_point"]] == np.arange(len(contours))).all() and (np.diff(contours["first_point"].astype(np.int64)) > 0).all(), \
        "contours by ascending representative"
    assert int(contours["n_points"].sum()) == len(points) and int(contours["n_segments"].sum()) == len(segments), "contour sizes"


def cut_to_planes(sec, n):
    """A section's arrays cut down to its first n planes (ids stay valid: planes lead every key)."""
    points, segments, contours, recs, _ = sec
    return points[points["plane"] < n], segments[points["plane"][segments["p0"]] < n], contours[contours["plane"] < n], recs[:n]


def section_device(g, H, d_verts, n_verts, stride, d_tris, n_tris, pose, planes):
    """hfpf_section_mesh_device on a mesh in HBM, downloaded and freed: (points, segments, contours, plane records, summary)."""
    (p, npt), (s, ns), (c, nc), recs, summ = g.section_mesh_device(d_verts, n_verts, stride, d_tris, n_tris, pose, planes)
    try:
        out = []
        for ptr, n, dt in ((p, npt, H.SECTION_POINT_DTYPE), (s, ns, H.SECTION_SEGMENT_DTYPE), (c, nc, H.SECTION_CONTOUR_DTYPE)):
            assert bool(ptr) == bool(n), "a device array is NULL exactly when it is empty"
            out.append(g.device_download(ptr, n * dt.itemsize).view(dt).copy() if n else np.zeros(0, dt))
    finally:
        for ptr in (p, s, c):
            if ptr:
                g.device_free(ptr)
    return out[0], out[1], out[2], recs, summ
