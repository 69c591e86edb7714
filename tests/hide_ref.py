"""The contract of hfpf_hide_voxels / hfpf_hide_box (include/hfpf.h), restated in numpy on extract's rows (imported by tests only).

F is the voxels of the rows hfpf_extract returns with nothing hidden, H a subset of it.  A call marks M (from a list of entries with
an optional selector word each, or from a box of inclusive voxel indices) and gives H' = H + M (HIDE), H - M (SHOW) or H + (F - M)
(HIDE_OTHERS), with five counts.  Voxel sets travel as (n, 3) int32 arrays in ascending (x, y, z) order, which is also what
hfpf_get_hidden lists."""
import numpy as np

HIDE, SHOW, HIDE_OTHERS = 1, 2, 3
OPS = {"hide": HIDE, "show": SHOW, "hide_others": HIDE_OTHERS}
COUNTS = ("n_selected", "n_matched", "n_changed", "n_hidden", "n_full")
KEY_BITS = 21   # bits of a key field at the largest grid (dims up to 2^21 - 2)


def keys(v):
    """One int64 per (n, 3) voxel with 0 <= index < 2^21: ascending keys are ascending (x, y, z)."""
    v = np.asarray(v, np.int64).reshape(-1, 3)
    return (v[:, 0] << (2 * KEY_BITS)) | (v[:, 1] << KEY_BITS) | v[:, 2]


def voxels_of(k):
    k = np.asarray(k, np.int64)
    m = (1 << KEY_BITS) - 1
    return np.ascontiguousarray(np.stack([k >> (2 * KEY_BITS), (k >> KEY_BITS) & m, k & m], axis=1).astype(np.int32)).reshape(-1, 3)


def row_voxels(rows):
    return np.stack([rows["ix"], rows["iy"], rows["iz"]], axis=1).astype(np.int64).reshape(-1, 3)


def full_set(rows):
    """F as sorted keys: the voxels of the rows (extract emits each voxel once)."""
    k = np.unique(keys(row_voxels(rows)))
    assert len(k) == len(rows), "extract emits a voxel once"
    return k


def selected(n, select, select_mask, select_value):
    if select is None:
        return np.ones(n, bool)
    w = np.asarray(select).astype(np.uint32).reshape(-1)
    assert len(w) == n, "one selector word per entry"
    return (w & np.uint32(select_mask & 0xFFFFFFFF)) == np.uint32(select_value & 0xFFFFFFFF)


def _finish(F, H, M, op, n_selected, n_matched):
    op = OPS.get(op, op)
    if op == HIDE:
        H2 = np.union1d(H, M)
    elif op == SHOW:
        H2 = np.setdiff1d(H, M)
    elif op == HIDE_OTHERS:
        H2 = np.union1d(H, np.setdiff1d(F, M))
    else:
        raise ValueError("unknown op %r" % (op,))
    counts = dict(n_selected=int(n_selected), n_matched=int(n_matched), n_changed=int(len(np.setxor1d(H, H2))), n_hidden=int(len(H2)),
                  n_full=int(len(F)))
    return voxels_of(H2), counts


def _state(rows, H, dims):
    F = full_set(rows)
    Hk = np.unique(keys(H)) if H is not None and len(H) else np.zeros(0, np.int64)
    assert np.isin(Hk, F).all(), "H is a subset of F"
    d = np.asarray(dims, np.int64).reshape(3)
    assert ((row_voxels(rows) >= 0) & (row_voxels(rows) < d)).all(), "a row outside 0..dim-1"
    return F, Hk, d


def hide_voxels(rows, H, dims, voxels, op="hide", select=None, select_mask=0, select_value=0):
    """(H', counts) of a list call.  rows: extract's rows with nothing hidden; H: (k, 3) hidden voxels (or None); voxels: (n, 3)
    integers of any int32 value; select: n uint32 words or None.  A handle without rows returns an all-zero result."""
    F, Hk, d = _state(rows, H, dims)
    if len(F) == 0:
        return voxels_of(Hk), dict.fromkeys(COUNTS, 0)
    v = np.asarray(voxels, np.int64).reshape(-1, 3)
    sel = selected(len(v), select, select_mask, select_value)
    in_range = ((v >= 0) & (v < d)).all(axis=1)
    cand = sel & in_range
    matched = np.zeros(len(v), bool)
    matched[cand] = np.isin(keys(v[cand]), F)
    M = np.unique(keys(v[matched]))
    return _finish(F, Hk, M, op, sel.sum(), matched.sum())


def hide_box(rows, H, dims, lo, hi, op="hide"):
    """(H', counts) of a box call: M = the voxels of F with lo[a] <= i_a <= hi[a] on every axis (any int32 lo, hi)."""
    F, Hk, _ = _state(rows, H, dims)
    if len(F) == 0:
        return voxels_of(Hk), dict.fromkeys(COUNTS, 0)
    fv = voxels_of(F).astype(np.int64)
    lo, hi = np.asarray(lo, np.int64).reshape(3), np.asarray(hi, np.int64).reshape(3)
    M = F[((fv >= lo) & (fv <= hi)).all(axis=1)]
    return _finish(F, Hk, M, op, len(M), len(M))


def visible(rows, H):
    """The rows every read-out sees: rows minus H, order kept."""
    if H is None or len(H) == 0:
        return rows
    return rows[~np.isin(keys(row_voxels(rows)), keys(H))]


def box_of_metres(box_m, bbox, res):
    """hfpf_node_hide_box: (lo, hi) voxel indices of a box in fusion-frame metres (x0, x1, y0, y1, z0, z1), each bound through the
    voxel = floor((p - bbox_min) / res) of the query contract, saturated to the int32 range."""
    b = np.asarray(box_m, np.float64).reshape(3, 2)
    lo0 = np.asarray(bbox, np.float64)[0::2]
    f = np.clip(np.floor((b - lo0[:, None]) / float(res)), -2.0 ** 31, 2.0 ** 31 - 1)
    return f[:, 0].astype(np.int64).astype(np.int32), f[:, 1].astype(np.int64).astype(np.int32)


# ---- the hidden set of the tests --------------------------------------------------------------------------------------------------

def middle_third(rows):
    """(lo, hi) of the voxel box spanning the middle third of the rows' ix range (all y, z): with x0, x1 = min, max of ix and n = x1 - x0
    + 1, the planes x0 + n // 3 .. x0 + 2 * n // 3 - 1."""
    x0, x1 = int(rows["ix"].min()), int(rows["ix"].max())
    n = x1 - x0 + 1
    big = 2 ** 31 - 1
    return np.array([x0 + n // 3, -big - 1, -big - 1], np.int32), np.array([x0 + 2 * n // 3 - 1, big, big], np.int32)


def hashed(rows):
    """Per row: (ix * 73856093 ^ iy * 19349663 ^ iz * 83492791) % 8 == 0 (int64 products)."""
    v = row_voxels(rows)
    return ((v[:, 0] * 73856093) ^ (v[:, 1] * 19349663) ^ (v[:, 2] * 83492791)) % 8 == 0


def hidden_set(rows):
    """S, (n, 3) int32 in ascending order: the rows inside middle_third's box plus the hashed ones."""
    lo, hi = middle_third(rows)
    v = row_voxels(rows)
    inside = (v[:, 0] >= int(lo[0])) & (v[:, 0] <= int(hi[0]))
    return voxels_of(np.unique(keys(v[inside | hashed(rows)])))


# What hidden_set does to faces scene `cut`, counted with the other restatements on the CPU oracle's rows alone (asserted exactly in
# test_hide_ref.py only): rows hidden and kept; points of faces.query_points whose hit changes (radius 2); every second ray of faces.rays whose
# hit changes (radius 2, step 0.5, no culling); triangles of the mesh of the kept rows (radius 2; all rows: 79,992); plane words that hold
# both a hidden and a visible row.
CUT_TABLE = dict(hidden=3747, kept=6340, query_changed=4502, rays_changed=213, masked_triangles=60372, mixed_words=284)
# half of each, as the floor the GPU tests hold their own session to: a mask that hides nothing, or everything, cannot pass
CUT_FLOOR = dict(hidden=1873, kept=3170, query_changed=2251, rays_changed=106, masked_triangles=30186, mixed_words=142)
FLOOR_QUERY = dict(radius=2)
FLOOR_RAYS = dict(radius=2, cull_backfaces=False, step=0.5)
FLOOR_RAYS_EVERY = 2   # every second ray of faces.rays: the march of the reference is the slowest of the restatements


def changed_records(a, b):
    """How many records of two equally long arrays differ in any byte."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    return int((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1).sum())


def mixed_plane_words(rows, H):
    """(brick, x-plane) words -- 8 x 8 cells of one x, a brick's (y, z) extent -- that hold both a hidden and a visible row: where a
    mask applied per word instead of per bit would show."""
    v = row_voxels(rows)
    word = keys(np.stack([v[:, 0], v[:, 1] >> 3, v[:, 2] >> 3], axis=1))
    hid = np.isin(keys(v), keys(H)) if len(H) else np.zeros(len(v), bool)
    return int(len(np.intersect1d(word[hid], word[~hid])))
