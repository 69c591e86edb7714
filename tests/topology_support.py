"""What the topology tests share (imported by tests only): the meshes beyond section_support's, the reference call, the device form's
helper, the byte-for-byte comparator and the invariants of every result.  No test and no fixture is defined here, and every assertion
carries its message.  Nothing here needs a GPU."""
import numpy as np

import section_support as S
import topology_ref as T

BBOX, IDENT = S.BBOX, S.IDENT
Q32, Q28, Q40 = 1 << 32, 1 << 28, 1 << 40
NAMES = ("edges", "loops", "shells", "tri_shell")
FAR_LO = (1023.5, -512.5, 256.0)
FAR_BBOX = (1023.5, 1024.5, -512.5, -511.5, 256.0, 257.0)
STRIP_PITCH, STRIP_HALF = 2.0 ** -18, 0.25


def open_cube():
    """The cube without its +z face (the two triangles on the vertices 1, 3, 5, 7)."""
    verts, tris = S.cube()
    keep = ~np.isin(tris, (1, 3, 5, 7)).all(axis=1)
    assert keep.sum() == 10, "two triangles leave"
    return verts, np.ascontiguousarray(tris[keep])


def lone_triangle():
    return np.array([[0.1, 0.0, 0.3], [0.3, 0.1, 0.4], [0.0, 0.25, 0.7]], np.float32), np.array([[0, 1, 2]], np.uint32)


def welded_strip(n, x0=-0.25, pitch=STRIP_PITCH, half=STRIP_HALF, z=0.5):
    """n triangles on n + 2 welded vertices: columns `pitch` apart along x, vertex 2j below (y = -half) and 2j + 1 above (y = +half);
    triangle i joins the vertices i, i + 1, i + 2, wound the same way throughout.  The coordinates are dyadic: every rim edge along x
    is exactly `pitch` long, an end edge of an even n exactly 2 half, and a triangle's area exactly pitch * half."""
    j = np.arange(n + 2)
    verts = np.stack([x0 + pitch * (j // 2), np.where(j % 2 == 0, -half, half), np.full(n + 2, z)], axis=1)
    assert (verts.astype(np.float32).astype(np.float64) == verts).all(), "the strip's coordinates are exact in f32"
    i = np.arange(n)
    tris = np.where((i % 2 == 0)[:, None], np.stack([i, i + 1, i + 2], 1), np.stack([i + 1, i, i + 2], 1))
    return verts.astype(np.float32), tris.astype(np.uint32)


def reference(verts, tris, pose=IDENT, bbox=BBOX, stride=None, n_verts=None):
    verts = np.ascontiguousarray(verts)
    stride = stride if stride is not None else (verts.dtype.itemsize if verts.dtype.names else 12)
    return T.topology(verts, stride, tris, pose, bbox, n_verts)


def same_topology(got, ref, what, tri_shell=True):
    """(edges, loops, shells, tri_shell, summary) byte for byte, with the first differing record of the first array that differs."""
    for name, a, b in zip(NAMES, got[:4], ref[:4]):
        if name == "tri_shell" and not tri_shell:
            continue
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype.itemsize == b.dtype.itemsize and len(a) == len(b), "%s: %d %s of %d bytes vs %d of %d" % (what, len(a), name, a.dtype.itemsize, len(b),
                                                                                                                   b.dtype.itemsize)
        if a.tobytes() != b.tobytes():
            x, y = a.view(np.uint8).reshape(len(a), -1), b.view(np.uint8).reshape(len(b), -1)
            bad = np.flatnonzero((x != y).any(axis=1))
            raise AssertionError("%s: %d of %d %s differ, first %d: %r vs %r" % (what, bad.size, len(a), name, int(bad[0]), a[bad[0]], b[bad[0]]))
    for k in T.SUMMARY_KEYS:
        assert got[4][k] == ref[4][k], "%s: summary %s: %r vs %r" % (what, k, got[4][k], ref[4][k])


def consistent(edges, loops, shells, tri_shell, summary):
    """What holds for every result: the counts add up, ids are in order, every record names what it belongs to."""
    s = summary
    assert s["n_edges"] == s["n_interior"] + s["n_boundary"] + s["n_nonmanifold"] + s["n_miswound"], "the classes add up to the edges"
    assert len(edges) == s["n_edges"] - s["n_interior"] and len(loops) == s["n_loops"] and len(shells) == s["n_shells"], "the arrays"
    for name, kind in (("n_boundary", T.BOUNDARY), ("n_nonmanifold", T.NONMANIFOLD), ("n_miswound", T.MISWOUND)):
        assert int((edges["kind"] == kind).sum()) == s[name] == int(shells[name].sum()), name
    lo, hi = np.minimum(edges["p0"], edges["p1"]).astype(np.int64), np.maximum(edges["p0"], edges["p1"]).astype(np.int64)
    assert (np.diff((lo << 26) | hi) > 0).all(), "edges in ascending (va, vb) order"
    assert (np.diff(loops["first_vertex"].astype(np.int64)) > 0).all() and (np.diff(shells["first_vertex"].astype(np.int64)) > 0).all(), \
        "loops and shells by ascending representative"
    bnd = edges["kind"] == T.BOUNDARY
    assert (edges["loop"][bnd] < len(loops)).all() and (edges["loop"][~bnd] == T.NONE).all() and (edges["shell"] < max(len(shells), 1)).all(), \
        "every listed edge names its loop and its shell"
    assert (loops["shell"][edges["loop"][bnd]] == edges["shell"][bnd]).all(), "a loop lies in the shell of its edges"
    assert (np.bincount(edges["loop"][bnd], minlength=len(loops)) == loops["n_edges"]).all(), "loop sizes"
    listed = np.bincount(edges["shell"], minlength=len(shells)) if len(edges) else np.zeros(len(shells), np.int64)
    assert (shells["n_edges"] >= listed).all() and int(shells["n_edges"].sum()) == s["n_edges"], "per shell: interior + listed edges"
    assert (shells["n_boundary"] + shells["n_nonmanifold"] + shells["n_miswound"] == listed).all(), "per shell: the listed edges by class"
    assert int(shells["n_tris"].sum()) == s["n_tris_valid"] - s["n_tris_far"] == int((tri_shell != T.NONE).sum()), "sum(n_tris) == n_used"
    assert int(shells["n_verts"].sum()) == s["n_verts_used"] and int(shells["n_loops"].sum()) == len(loops), "vertices and loops per shell"
    assert (np.bincount(tri_shell[tri_shell != T.NONE], minlength=len(shells)) == shells["n_tris"]).all(), "tri_shell against n_tris"
    assert s["n_closed_loops"] == int(((loops["flags"] & T.LOOP_CLOSED) != 0).sum()), "closed loops"
    tight = (shells["flags"] & T.SHELL_WATERTIGHT) != 0
    assert s["n_watertight"] == int(tight.sum()) and ((shells["n_boundary"] + shells["n_nonmanifold"] + shells["n_miswound"] == 0) == tight).all(), "watertight"
    assert (edges["reserved"] == 0).all() and (loops["reserved"] == 0).all() and (shells["reserved"] == 0).all() and (shells["reserved0"] == 0).all(), "reserved"


def topology_device(g, H, d_verts, n_verts, stride, d_tris, n_tris, pose=IDENT, tri_shell=True):
    """hfpf_mesh_topology_device on a mesh in HBM, downloaded and freed: (edges, loops, shells, tri_shell or None, summary)."""
    (e, ne), (l, nl), (s, ns), t, summ = g.mesh_topology_device(d_verts, n_verts, stride, d_tris, n_tris, pose, tri_shell=tri_shell)
    try:
        out = []
        for ptr, n, dt in ((e, ne, H.TOPOLOGY_EDGE_DTYPE), (l, nl, H.TOPOLOGY_LOOP_DTYPE), (s, ns, H.TOPOLOGY_SHELL_DTYPE)):
            assert bool(ptr) == bool(n), "a device array is NULL exactly when it is empty"
            out.append(g.device_download(ptr, n * dt.itemsize).view(dt).copy() if n else np.zeros(0, dt))
        assert bool(t) == bool(tri_shell and n_tris), "tri_shell is produced exactly when it is asked for"
        out.append(None if not tri_shell else g.device_download(t, n_tris * 4).view(np.uint32).copy() if t else np.zeros(0, np.uint32))
    finally:
        for ptr in (e, l, s, t):
            if ptr:
                g.device_free(ptr)
    return out[0], out[1], out[2], out[3], summ
