"""The connected-components contract of include/hfpf.h restated in numpy (imported by tests only): hfpf_extract's rows and the options
-> the rows, labels and component records hfpf_extract_components* return.  Rows come in extract's lexicographic order, so
np.searchsorted on their keys finds the row of a cell; the neighbour pairs are collected over the lexicographically positive half of
the (2 reach + 1)^3 offsets (the relation is symmetric), and the components come from min-label propagation with pointer jumping:
a label is a row index, and at the end every row carries the smallest row index of its component."""
import numpy as np

ROW_FIELDS = ("ix", "iy", "iz", "count", "x", "y", "z", "nx", "ny", "nz", "sdx", "sdy", "sdz", "mean_dist", "sd_dist", "rgb")
ROW_DTYPE = np.dtype([(f, "<i4") for f in ROW_FIELDS[:3]] + [("count", "<u4")] + [(f, "<f4") for f in ROW_FIELDS[4:15]] + [("rgb", "<u4")])
COMPONENT_DTYPE = np.dtype([("first_row", "<u4"), ("n_rows", "<u4"), ("points", "<u8"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)),
                            ("source_row", "<u4"), ("reserved", "<u4")])
assert ROW_DTYPE.itemsize == 64 and COMPONENT_DTYPE.itemsize == 48
KEY_BITS = 21  # cell coordinates below 2^21 per axis


def keys(ix, iy, iz):
    return (ix.astype(np.int64) << (2 * KEY_BITS)) | (iy.astype(np.int64) << KEY_BITS) | iz.astype(np.int64)


def count_gate(rows, min_count):
    """The rows hfpf_extract_filtered keeps: a row is dropped iff (double)(int)count < min_count; 0 (or less) keeps all."""
    if not min_count > 0.0:
        return np.ones(len(rows), bool)
    return ~(rows["count"].astype(np.int32).astype(np.float64) < float(min_count))


def neighbour_pairs(rows, reach):
    """(a, b), a < b: every pair of rows within Chebyshev distance `reach` of each other, each once."""
    n = len(rows)
    ix, iy, iz = (rows[f].astype(np.int64) for f in ("ix", "iy", "iz"))
    k = keys(ix, iy, iz)
    assert n < 2 or (np.diff(k) > 0).all(), "rows must be in lexicographic (ix, iy, iz) order, one per cell"
    lim = 1 << KEY_BITS
    out_a, out_b = [], []
    me = np.arange(n, dtype=np.int64)
    r = int(reach)
    for dx in range(0, r + 1):
        for dy in range(-r, r + 1):
            for dz in range(-r, r + 1):
                if (dx, dy, dz) <= (0, 0, 0):
                    continue  # the positive half: the neighbour's key is the larger one, so its row index is
                x, y, z = ix + dx, iy + dy, iz + dz
                ok = (y >= 0) & (z >= 0) & (x < lim) & (y < lim) & (z < lim)
                nk = keys(x[ok], y[ok], z[ok])
                pos = np.searchsorted(k, nk)
                hit = pos < n
                hit[hit] = k[pos[hit]] == nk[hit]
                out_a.append(me[ok][hit])
                out_b.append(pos[hit])
    if not out_a:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(out_a), np.concatenate(out_b)


def normal_gate(rows, a, b, min_normal_dot):
    """((double)nx_a*(double)nx_b + (double)ny_a*(double)ny_b) + (double)nz_a*(double)nz_b >= min_normal_dot; a NaN compares false."""
    nx, ny, nz = (rows[f].astype(np.float64) for f in ("nx", "ny", "nz"))
    with np.errstate(invalid="ignore", over="ignore"):
        dot = (nx[a] * nx[b] + ny[a] * ny[b]) + nz[a] * nz[b]
        return dot >= float(min_normal_dot)


def labels_of(n, a, b):
    """Min-label propagation with pointer jumping: lab[j] = the smallest row index of j's component.  Between rounds lab is a forest
    of stars (lab[lab[j]] == lab[j]) whose labels are rows of the same component not above j.  A round hooks every root under the
    smallest label any of its tree's edges sees (only roots are rewritten, so no link of a tree is lost and trees only merge), then
    jumps pointers until the stars are back.  An edge inside one tree stays there and is dropped; without edges left every component
    is one star, rooted at its smallest row."""
    lab = np.arange(n, dtype=np.int64)
    while True:
        live = lab[a] != lab[b]
        a, b = a[live], b[live]
        if len(a) == 0:
            return lab
        m = np.minimum(lab[a], lab[b])
        np.minimum.at(lab, np.maximum(lab[a], lab[b]), m)
        while True:  # pointer jumping: the label of my label
            nn = lab[lab]
            if np.array_equal(nn, lab):
                break
            lab = nn


def components(rows, reach=1, min_count=0.0, min_normal_dot=-2.0, min_rows=0, min_points=0, keep_largest=0):
    """(rows, labels, comps) of hfpf_extract_components for `rows` = hfpf_extract's rows (any min_count gate not yet applied)."""
    rows = np.ascontiguousarray(rows, ROW_DTYPE)
    rows = rows[count_gate(rows, min_count)]
    n = len(rows)
    if n == 0:
        return rows.copy(), np.zeros(0, np.uint32), np.zeros(0, COMPONENT_DTYPE)
    a, b = neighbour_pairs(rows, reach)
    ok = normal_gate(rows, a, b, min_normal_dot)
    lab = labels_of(n, a[ok], b[ok])
    reps, comp_of, n_rows = np.unique(lab, return_inverse=True, return_counts=True)  # ascending representative
    assert np.array_equal(lab[reps], reps)
    nc = len(reps)
    points = np.zeros(nc, np.uint64)
    np.add.at(points, comp_of, rows["count"].astype(np.uint64))
    lo = np.full((nc, 3), np.iinfo(np.int32).max, np.int32)
    hi = np.full((nc, 3), np.iinfo(np.int32).min, np.int32)
    for k, f in enumerate(("ix", "iy", "iz")):
        np.minimum.at(lo[:, k], comp_of, rows[f])
        np.maximum.at(hi[:, k], comp_of, rows[f])
    keep = (n_rows >= int(min_rows)) & (points >= np.uint64(min_points))
    if keep_largest:
        cand = np.flatnonzero(keep)
        order = cand[np.lexsort((reps[cand], -n_rows[cand].astype(np.int64)))]  # n_rows descending, then representative ascending
        keep = np.zeros(nc, bool)
        keep[order[:int(keep_largest)]] = True
    new_id = np.cumsum(keep) - 1
    row_keep = keep[comp_of]
    new_row = np.cumsum(row_keep) - 1
    comps = np.zeros(int(keep.sum()), COMPONENT_DTYPE)
    kc = np.flatnonzero(keep)
    comps["first_row"] = new_row[reps[kc]]
    comps["n_rows"] = n_rows[kc]
    comps["points"] = points[kc]
    comps["lo"], comps["hi"] = lo[kc], hi[kc]
    comps["source_row"] = reps[kc]
    return rows[row_keep].copy(), new_id[comp_of[row_keep]].astype(np.uint32), comps
