"""CPU: tests/hide_ref.py, the numpy restatement of hfpf_hide_voxels / hfpf_hide_box, against its own properties on the CPU oracle's
rows of faces scene `cut` (10,087 rows): duplicates, out-of-range and index == dim entries, voxels without a row, the selector, the
algebra of the ops.  It is also the one place where the hidden set S of the GPU tests and what it does to the other read-outs'
restatements are counted exactly; tests/hide_ref.py holds half of each figure as the floor of the GPU tests."""
import numpy as np
import pytest

import faces
import hide_ref as HR
import mesh_ref as M
import query_ref as Q
import raycast_ref as RC
import scenes
from gpu_support import IDENT

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
_MODEL = []


@pytest.fixture
def model(oracle_mod, synth_mod):
    """(scene, rows, occupied, dims, res) of the oracle alone, computed once."""
    if not _MODEL:
        sc = faces.FaceScene("cut")
        og = oracle_mod.OracleGrid(resolution=sc.resolution, bbox=sc.bbox, fuse_color=True, **sc.config)
        rows = scenes.run(og, sc, "capture", color=True)
        occ = og.occupied()
        dims, res = og.dims
        og.close()
        _MODEL.append((sc, rows, occ, dims, res))
    return _MODEL[0]


def _v(rows):
    return HR.row_voxels(rows).astype(np.int32)


def _set(v):
    return set(map(tuple, np.asarray(v).reshape(-1, 3).tolist()))


def test_the_scene(model):
    sc, rows, occ, dims, res = model
    assert len(rows) == 10087 == faces.ORACLE_TABLE["cut"][0] and tuple(dims) == (104, 72, 88)


def test_duplicates_do_not_count_twice(model):
    _, rows, _, dims, _ = model
    v = _v(rows)[::7]
    once = HR.hide_voxels(rows, None, dims, v)
    thrice = HR.hide_voxels(rows, None, dims, np.vstack([v, v[::-1], v]))
    assert np.array_equal(once[0], thrice[0]) and _set(once[0]) == _set(v)
    assert once[1] == dict(n_selected=len(v), n_matched=len(v), n_changed=len(v), n_hidden=len(v), n_full=len(rows))
    assert thrice[1] == dict(n_selected=3 * len(v), n_matched=3 * len(v), n_changed=len(v), n_hidden=len(v), n_full=len(rows))
    # the listing is ascending (x, y, z)
    k = HR.keys(once[0])
    assert (np.diff(k) > 0).all()


def test_entries_out_of_range_and_voxels_without_a_row(model):
    _, rows, occ, dims, _ = model
    v = _v(rows)
    d = np.asarray(dims, np.int32)
    outside = np.array([[-1, 5, 5], [5, -1, 5], [5, 5, -1], [d[0], 5, 5], [5, d[1], 5], [5, 5, d[2]], [INT_MIN, INT_MIN, INT_MIN], [INT_MAX, 0, 0],
                        [INT_MIN, 5, 5], list(v[0] + [d[0], 0, 0])], np.int32)
    at_dim = occ[(occ == d).any(axis=1)]
    inside = occ[(occ < d).all(axis=1)]
    no_row = inside[~np.isin(HR.keys(inside), HR.full_set(rows))]
    assert len(at_dim) >= 100 and len(no_row) >= 100, "occupied cells at index == dim and occupied cells without a row"
    entries = np.vstack([outside, at_dim, no_row, v[:3]])
    H, c = HR.hide_voxels(rows, None, dims, entries)
    assert _set(H) == _set(v[:3]) and c == dict(n_selected=len(entries), n_matched=3, n_changed=3, n_hidden=3, n_full=len(rows))
    # an empty free cell
    free = np.array([[0, 0, 0]], np.int32)
    assert tuple(free[0]) not in _set(occ)
    assert HR.hide_voxels(rows, H, dims, free)[1]["n_matched"] == 0
    # no rows at all: an all-zero result, whatever the list
    H0, c0 = HR.hide_voxels(rows[:0], None, dims, entries)
    assert len(H0) == 0 and c0 == dict.fromkeys(HR.COUNTS, 0)
    assert HR.hide_box(rows[:0], None, dims, (0, 0, 0), (5, 5, 5), "hide_others")[1] == dict.fromkeys(HR.COUNTS, 0)


def test_the_selector(model):
    _, rows, _, dims, _ = model
    v = _v(rows)
    words = (np.arange(len(v)) % 5).astype(np.uint32) | np.uint32(0x100)
    H, c = HR.hide_voxels(rows, None, dims, v, select=words, select_mask=0xFF, select_value=3)
    assert _set(H) == _set(v[3::5]) and c["n_selected"] == c["n_matched"] == len(v[3::5])
    H, c = HR.hide_voxels(rows, None, dims, v, select=words, select_mask=0xFFFFFFFF, select_value=3)
    assert len(H) == 0 and c["n_selected"] == 0
    H, c = HR.hide_voxels(rows, None, dims, v, select=words, select_mask=0, select_value=0)   # mask 0: every word matches value 0
    assert len(H) == len(v)
    flags = np.where(np.arange(len(v)) % 3 == 0, 5, 3).astype(np.uint32)                     # mask = value = 4: the flag's bit
    H, c = HR.hide_voxels(rows, None, dims, v, select=flags, select_mask=4, select_value=4)
    assert _set(H) == _set(v[0::3])


def test_the_algebra_of_the_ops(model):
    _, rows, _, dims, _ = model
    v = _v(rows)
    S = HR.hidden_set(rows)
    H0, _ = HR.hide_voxels(rows, None, dims, v[::11])
    L = v[np.arange(len(v)) % 11 == 5][::2]   # disjoint from H0: HIDE then SHOW of it restores H0
    assert len(L) > 400 and not _set(L) & _set(H0)
    H1, c1 = HR.hide_voxels(rows, H0, dims, L, "hide")
    H2, c2 = HR.hide_voxels(rows, H1, dims, L, "show")
    assert np.array_equal(H2, H0) and c1["n_changed"] == c2["n_changed"] == len(L) and c2["n_hidden"] == len(H0)
    # SHOW of what is not hidden, HIDE of what is: nothing changes
    assert HR.hide_voxels(rows, H0, dims, L, "show")[1]["n_changed"] == 0 and HR.hide_voxels(rows, H1, dims, L, "hide")[1]["n_changed"] == 0
    # HIDE_OTHERS is cumulative: it never shows what was hidden before
    K, ck = HR.hide_voxels(rows, H0, dims, S, "hide_others")
    assert _set(K) == _set(H0) | (_set(v) - _set(S)) and ck["n_matched"] == len(S)
    K2, _ = HR.hide_voxels(rows, K, dims, v, "hide_others")   # keep everything: nothing more is hidden, nothing shown
    assert np.array_equal(K2, K)
    # with n = 0 it hides everything
    A, ca = HR.hide_voxels(rows, None, dims, np.zeros((0, 3), np.int32), "hide_others")
    assert len(A) == len(rows) and ca == dict(n_selected=0, n_matched=0, n_changed=len(rows), n_hidden=len(rows), n_full=len(rows))
    assert len(HR.visible(rows, A)) == 0 and HR.visible(rows, None) is rows
    with pytest.raises(ValueError):
        HR.hide_voxels(rows, None, dims, L, 4)


def test_a_box_is_the_list_of_its_voxels(model):
    _, rows, _, dims, _ = model
    v = _v(rows)
    for lo, hi in (((10, 5, 0), (40, 60, 87)), ((-5, -5, -5), (3, 200, 200)), ((INT_MIN,) * 3, (INT_MAX,) * 3), ((103, 0, 0), (INT_MAX, 71, 87)),
                   ((50, 30, 40), (49, 71, 87)), ((104, 0, 0), (200, 71, 87)), HR.middle_third(rows)):
        inside = ((v >= np.asarray(lo, np.int64)) & (v <= np.asarray(hi, np.int64))).all(axis=1)
        for op in ("hide", "show", "hide_others"):
            H0 = v[::3]
            a = HR.hide_box(rows, H0, dims, lo, hi, op)
            b = HR.hide_voxels(rows, H0, dims, v[inside], op)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1], (lo, hi, op)
            assert a[1]["n_selected"] == a[1]["n_matched"] == int(inside.sum())
    assert HR.hide_box(rows, None, dims, (50, 30, 40), (49, 71, 87))[1]["n_matched"] == 0, "lo > hi is the empty box"


def test_a_box_in_metres(model):
    sc, rows, _, dims, res = model
    lo0 = np.asarray(sc.bbox, np.float64)[0::2]
    box = [lo0[0] + 10.5 * res, lo0[0] + 20.25 * res, lo0[1] - 1.0, lo0[1] + 1.0, lo0[2] + 3.0 * res + 1e-9, lo0[2] + 1e12]
    lo, hi = HR.box_of_metres(box, sc.bbox, res)
    assert lo.tolist() == [10, int(np.floor(-1.0 / res)), 3] and hi.tolist()[:2] == [20, int(np.floor(1.0 / res))] and hi[2] == INT_MAX
    assert lo.dtype == hi.dtype == np.int32


def test_the_hidden_set_and_what_it_changes(model):
    """S, and the figures of tests/hide_ref.CUT_TABLE: counted here, on the oracle's rows alone, with the existing restatements."""
    sc, rows, occ, dims, res = model
    S = HR.hidden_set(rows)
    lo, hi = HR.middle_third(rows)
    assert (int(rows["ix"].min()), int(rows["ix"].max())) == (0, 103) and (int(lo[0]), int(hi[0])) == (34, 68)
    v = _v(rows)
    assert _set(S) == _set(v[((v[:, 0] >= 34) & (v[:, 0] <= 68)) | HR.hashed(rows)])
    assert HR.hashed(rows).sum() > len(rows) // 16 and (HR.hashed(rows) & ~((v[:, 0] >= 34) & (v[:, 0] <= 68))).sum() > 300
    vis = HR.visible(rows, S)
    got = dict(hidden=len(S), kept=len(vis), mixed_words=HR.mixed_plane_words(rows, S))
    pts = faces.query_points(rows, sc.bbox, res, dims)
    got["query_changed"] = HR.changed_records(Q.query(rows, occ, pts, IDENT, sc.bbox, res, **HR.FLOOR_QUERY)[0],
                                              Q.query(vis, occ, pts, IDENT, sc.bbox, res, **HR.FLOOR_QUERY)[0])
    rays = faces.rays(sc.bbox, res)[::HR.FLOOR_RAYS_EVERY]
    kw = dict(HR.FLOOR_RAYS, t_range=(0.0, faces.ray_t_max(sc.bbox, res, HR.FLOOR_RAYS["step"])))
    got["rays_changed"] = HR.changed_records(RC.raycast(rows, occ, rays, IDENT, sc.bbox, res, **kw), RC.raycast(vis, occ, rays, IDENT, sc.bbox, res, **kw))
    got["masked_triangles"] = len(M.mesh(vis, occ, sc.bbox, res, dims, radius=2)[1])
    print(got)
    assert got == HR.CUT_TABLE
    assert HR.CUT_FLOOR == {k: n // 2 for k, n in HR.CUT_TABLE.items()}, "the floors are half the counted values"
    assert len(S) + len(vis) == len(rows)
