"""The topology contract of include/hfpf.h restated in numpy (imported by tests only): a triangle mesh, a pose and the handle's bounding
box -> the listed edges, loops, shells, per-triangle shells and the summary hfpf_mesh_topology* return.  The mesh intake and the
triangle classes are section_ref's; everything is vectorised and sort-based, f64 with one rounding per operation in the order the header
writes it, and the sums are int64 and wrap as the header says."""
import numpy as np

import deviation_ref as D
import section_ref as X

EDGE_DTYPE = np.dtype([("p0", "<u4"), ("p1", "<u4"), ("tri", "<u4"), ("kind", "<u4"), ("uses", "<u4"), ("loop", "<u4"), ("shell", "<u4"),
                       ("reserved", "<u4")])
LOOP_DTYPE = np.dtype([("first_vertex", "<u4"), ("n_verts", "<u4"), ("n_edges", "<u4"), ("n_ends", "<u4"), ("flags", "<u4"), ("shell", "<u4"),
                       ("length_q32", "<i8"), ("area_q28", "<i8", (3,)), ("reserved", "<u8")])
SHELL_DTYPE = np.dtype([("first_vertex", "<u4"), ("n_verts", "<u4"), ("n_tris", "<u4"), ("flags", "<u4"), ("n_edges", "<u4"), ("n_boundary", "<u4"),
                        ("n_nonmanifold", "<u4"), ("n_miswound", "<u4"), ("n_loops", "<u4"), ("reserved0", "<u4"), ("area_q32", "<i8"),
                        ("volume_q40", "<i8"), ("reserved", "<u8")])
assert (EDGE_DTYPE.itemsize, LOOP_DTYPE.itemsize, SHELL_DTYPE.itemsize) == (32, 64, 64)
INTERIOR, BOUNDARY, NONMANIFOLD, MISWOUND = 0, 1, 2, 3
LOOP_CLOSED, LOOP_BRANCHED = 1, 2
SHELL_OPEN, SHELL_NONMANIFOLD, SHELL_MISWOUND, SHELL_WATERTIGHT = 1, 2, 4, 8
NONE = 0xFFFFFFFF
MAX_VERTS, MAX_HALF_EDGES = 1 << 26, 1 << 32
SUMMARY_KEYS = ("n_tris_valid", "n_tris_invalid", "n_tris_far", "n_verts_used", "n_edges", "n_interior", "n_boundary", "n_nonmanifold", "n_miswound",
                "n_loops", "n_closed_loops", "n_shells", "n_watertight")


def components(n, a, b):
    """label[v] = the smallest vertex of v's connected component among n vertices joined by the pairs (a[i], b[i]).  Roots are
    hooked under smaller labels and the paths are then jumped flat, round after round until no pair disagrees: a label never exceeds
    its vertex and never leaves the component, so the fixed point is the component's smallest vertex."""
    label = np.arange(n, dtype=np.int64)
    while len(a):
        la, lb = label[a], label[b]
        if (la == lb).all():
            break
        np.minimum.at(label, la, lb)
        np.minimum.at(label, lb, la)
        while True:
            jumped = label[label]
            if (jumped == label).all():
                break
            label = jumped
    return label


def _numbered(label, member):
    """(number of each vertex's component or -1, the representatives in ascending order) for the vertices `member` marks."""
    reps = np.unique(label[member])
    number = np.full(len(label), -1, np.int64)
    number[member] = np.searchsorted(reps, label[member])
    return number, reps


def _q(v, bits):
    return np.rint(v * 2.0 ** bits).astype(np.int64)


def _sum_into(n, index, terms):
    acc = np.zeros(n, np.int64)
    with np.errstate(over="ignore"):
        np.add.at(acc, index, terms)
    return acc


def topology(verts, stride, tris, pose, bbox, n_verts=None):
    """(edges, loops, shells, tri_shell, summary dict) of a mesh."""
    V, tris, valid, used = X.classify(verts, stride, tris, pose, bbox, n_verts)
    assert len(V) <= MAX_VERTS and 3 * len(tris) < MAX_HALF_EDGES, "beyond the limits the call returns HFPF_ERR_BAD_ARG"
    nv = len(V)
    summary = dict.fromkeys(SUMMARY_KEYS, 0)
    summary.update(n_tris_valid=int(valid.sum()), n_tris_invalid=int((~valid).sum()), n_tris_far=int((valid & ~used).sum()))
    T = np.flatnonzero(used)
    I = tris[T]
    tri_shell = np.full(len(tris), NONE, np.uint32)
    if len(T) == 0:
        return np.zeros(0, EDGE_DTYPE), np.zeros(0, LOOP_DTYPE), np.zeros(0, SHELL_DTYPE), tri_shell, summary
    # half-edges 3k + c from i_c to i_(c+1), in ascending id
    he_id = (3 * T[:, None] + np.arange(3)[None, :]).reshape(-1)
    frm, to = I.reshape(-1), I[:, [1, 2, 0]].reshape(-1)
    va, vb, fwd = np.minimum(frm, to), np.maximum(frm, to), frm < to
    key = (va << 26) | vb
    order = np.argsort(key, kind="stable")  # within an edge the ids stay ascending
    ukey, first, inv = np.unique(key[order], return_index=True, return_inverse=True)
    ne = len(ukey)
    n_fwd = np.bincount(inv, weights=fwd[order], minlength=ne).astype(np.int64)
    n_bwd = np.bincount(inv, weights=~fwd[order], minlength=ne).astype(np.int64)
    uses = n_fwd + n_bwd
    kind = np.where(uses == 1, BOUNDARY, np.where(uses >= 3, NONMANIFOLD, np.where((n_fwd == 1) & (n_bwd == 1), INTERIOR, MISWOUND)))
    eva, evb = ukey >> 26, ukey & ((1 << 26) - 1)
    e_tri = he_id[order][first] // 3
    # shells
    in_shell = np.zeros(nv, bool)
    in_shell[I.reshape(-1)] = True
    label = components(nv, np.concatenate([I[:, 0], I[:, 0]]), np.concatenate([I[:, 1], I[:, 2]]))
    vshell, shell_rep = _numbered(label, in_shell)
    ns = len(shell_rep)
    t_shell = vshell[I[:, 0]]
    tri_shell[T] = t_shell
    e_shell = vshell[eva]
    A, B, C, N, _ = D.triangles(D.vertex_xyz(verts, stride, n_verts), tris, pose)
    A, B, C, N = A[T], B[T], C[T], N[T]
    Pr = V[shell_rep[t_shell]]
    shells = np.zeros(ns, SHELL_DTYPE)
    shells["first_vertex"] = shell_rep
    shells["n_verts"] = np.bincount(vshell[in_shell], minlength=ns)
    shells["n_tris"] = np.bincount(t_shell, minlength=ns)
    shells["n_edges"] = np.bincount(e_shell, minlength=ns)
    for name, k in (("n_boundary", BOUNDARY), ("n_nonmanifold", NONMANIFOLD), ("n_miswound", MISWOUND)):
        shells[name] = np.bincount(e_shell[kind == k], minlength=ns)
    shells["area_q32"] = _sum_into(ns, t_shell, _q(0.5 * np.sqrt(D.dot(N, N)), 32))
    shells["volume_q40"] = _sum_into(ns, t_shell, _q(D.dot(A - Pr, X.cross(B - Pr, C - Pr)) / 6.0, 40))
    flags = (np.where(shells["n_boundary"] > 0, SHELL_OPEN, 0) | np.where(shells["n_nonmanifold"] > 0, SHELL_NONMANIFOLD, 0) |
             np.where(shells["n_miswound"] > 0, SHELL_MISWOUND, 0))
    shells["flags"] = np.where(flags == 0, SHELL_WATERTIGHT, flags)
    # loops
    bnd = kind == BOUNDARY
    b_fwd = n_fwd[bnd] == 1
    p0, p1 = np.where(b_fwd, eva[bnd], evb[bnd]), np.where(b_fwd, evb[bnd], eva[bnd])
    n_out, n_in = np.bincount(p0, minlength=nv), np.bincount(p1, minlength=nv)
    on_rim = (n_out + n_in) > 0
    vloop, loop_rep = _numbered(components(nv, p0, p1), on_rim)
    nl = len(loop_rep)
    e_loop = vloop[p0]
    loops = np.zeros(nl, LOOP_DTYPE)
    loops["first_vertex"], loops["shell"] = loop_rep, vshell[loop_rep]
    loops["n_verts"] = np.bincount(vloop[on_rim], minlength=nl)
    loops["n_edges"] = np.bincount(e_loop, minlength=nl)
    loops["n_ends"] = np.bincount(vloop[on_rim & (n_in + n_out == 1)], minlength=nl)
    is_open = np.bincount(vloop[on_rim & ~((n_in == 1) & (n_out == 1))], minlength=nl) > 0
    branched = np.bincount(vloop[on_rim & ((n_in > 1) | (n_out > 1))], minlength=nl) > 0
    loops["flags"] = np.where(is_open, 0, LOOP_CLOSED) | np.where(branched, LOOP_BRANCHED, 0)
    if nl:
        P0, P1, Lr = V[p0], V[p1], V[loop_rep[e_loop]]
        e = P1 - P0
        loops["length_q32"] = _sum_into(nl, e_loop, _q(np.sqrt(D.dot(e, e)), 32))
        area = _q(0.5 * X.cross(P0 - Lr, P1 - Lr), 28)
        for k in range(3):
            loops["area_q28"][:, k] = _sum_into(nl, e_loop, area[:, k])
    shells["n_loops"] = np.bincount(loops["shell"].astype(np.int64), minlength=ns)
    # the listed edges
    listed = kind != INTERIOR
    edges = np.zeros(int(listed.sum()), EDGE_DTYPE)
    loop_of_edge = np.full(ne, NONE, np.int64)
    loop_of_edge[bnd] = e_loop
    back = bnd & (n_fwd == 0)
    edges["p0"], edges["p1"] = np.where(back, evb, eva)[listed], np.where(back, eva, evb)[listed]
    edges["tri"], edges["kind"], edges["shell"], edges["loop"] = e_tri[listed], kind[listed], e_shell[listed], loop_of_edge[listed]
    edges["uses"] = (np.minimum(n_fwd, 65535) | (np.minimum(n_bwd, 65535) << 16))[listed]
    summary.update(n_verts_used=int(in_shell.sum()), n_edges=ne, n_interior=int((kind == INTERIOR).sum()), n_boundary=int(bnd.sum()),
                   n_nonmanifold=int((kind == NONMANIFOLD).sum()), n_miswound=int((kind == MISWOUND).sum()), n_loops=nl,
                   n_closed_loops=int(((loops["flags"] & LOOP_CLOSED) != 0).sum()), n_shells=ns,
                   n_watertight=int(((shells["flags"] & SHELL_WATERTIGHT) != 0).sum()))
    return edges, loops, shells, tri_shell, summary
