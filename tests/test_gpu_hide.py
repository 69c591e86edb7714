"""GPU: hiding rows from every read-out (hfpf_hide_voxels, hfpf_hide_voxels_device, hfpf_hide_box, hfpf_show_all, hfpf_get_hidden).
The hidden set H and the five counts of every call are compared with tests/hide_ref.py; every read-out of a handle that hides S is
compared byte for byte with its own numpy restatement fed with the unmasked hfpf_extract rows minus S and the unchanged occupied list.
The session is faces scene `cut` (8 frames of 320 x 240, about 10 K rows, rows in all six face layers); S and the floors that keep it
meaningful are tests/hide_ref.py's (counted in test_hide_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import align_ref as A
import components_ref as CR
import consistency_ref as CS
import cover_ref as V
import deviation_ref as D
import faces
import gpu_support as G
import hide_ref as HR
import mesh_ref as M
import query_ref as Q
import raycast_ref as RC
import render_ref as R
import scenes
import track_ref as TR
from gpu_support import IDENT

pytestmark = pytest.mark.gpu
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
W, H = 320, 240
STEP = 0.5
CONS_KW = dict(window=1, tolerance=0.004, min_cos=0.3, min_through=1, through_ratio=0.0)
ALIGN_KW = dict(max_iterations=5, stride=8, eps_rotation=1e-5, eps_translation=1e-5)


@pytest.fixture(scope="module")
def session(hfpf_mod, synth_mod):
    """The `cut` session with what the tests share: S, the rows without it, its own mesh (of all rows), three depth frames."""
    s = G.Session(hfpf_mod, "cut")
    try:
        s.S = HR.hidden_set(s.rows)
        s.vis = HR.visible(s.rows, s.S)
        s.vox = HR.row_voxels(s.rows).astype(np.int32)
        s.own_mesh()
        s.g.extract()
        s.blob = s.g.snapshot().tobytes()   # of the handle that never hid anything (behind a plain extract: see test_snapshot_...)
        frames, poses = [], []
        for f in (0, 3, s.sc.n_frames + 1):
            pose = synth_mod.pose(s.sc.pose_seed, f)
            depth, _, K = synth_mod.depth_frame(s.sc.seed, f, W, H, pose)
            frames.append(depth), poses.append(pose)
        far = frames[0].copy()   # frame 0 again with its left half 50 mm farther: the rows in front of it are seen THROUGH
        left = far[:, :W // 2]
        left[left != 0] += 50
        s.frames, s.poses, s.K = np.stack(frames + [far]), np.stack(poses + [poses[0]]), K
        for a in (s.S, s.vis, s.vox, s.frames, s.poses):
            a.setflags(write=False)
        print("cut: %d rows, %d in S, %d kept, %d plane words with both" % (len(s.rows), len(s.S), len(s.vis), HR.mixed_plane_words(s.rows, s.S)))
        assert len(s.S) >= HR.CUT_FLOOR["hidden"] and len(s.vis) >= HR.CUT_FLOOR["kept"], "S hides nearly nothing or nearly everything"
        assert HR.mixed_plane_words(s.rows, s.S) >= HR.CUT_FLOOR["mixed_words"], "too few plane words hold both a hidden and a visible row"
    except BaseException:
        s.close()
        raise
    yield s
    s.close()


def _hide_S(s):
    s.g.show_all()
    c = s.g.hide_voxels(s.S)
    assert c["n_hidden"] == len(s.S) == c["n_matched"] and c["n_full"] == len(s.rows), c


def _state(s, H_ref, what):
    """The handle's H and rows are the restatement's."""
    got = s.g.hidden()
    assert got.dtype == np.int32 and got.tobytes() == np.ascontiguousarray(H_ref, np.int32).tobytes(), "%s: hfpf_get_hidden, %d vs %d voxels" % (what, len(got), len(H_ref))
    G.same_records(s.g.extract(), HR.visible(s.rows, H_ref), "%s: extract" % what, "rows")


def _as_rows(hfpf_mod, v):
    """Entries as an hfpf_row array (stride 64): only ix, iy, iz are read, the rest is noise."""
    r = np.frombuffer(np.random.default_rng(5).bytes(64 * len(v)), hfpf_mod.ROW_DTYPE).copy()
    r["ix"], r["iy"], r["iz"] = v[:, 0], v[:, 1], v[:, 2]
    return r


def _call(s, form, entries, op, select=None, mask=0, value=0):
    """One list call in the host or the device form; entries: (n, 3) int32 or an hfpf_row array."""
    if form == "host":
        return s.g.hide_voxels(entries, op, select=select, select_mask=mask, select_value=value)
    stride = entries.dtype.itemsize if entries.dtype.names else 12
    arrays = [entries] + ([np.ascontiguousarray(select)] if select is not None else [])
    with G.uploaded(s.g, *arrays) as ptrs:
        return s.g.hide_voxels(ptrs[0], op, select=ptrs[1] if select is not None else None, select_mask=mask, select_value=value, device=True, n=len(entries),
                               voxel_stride=stride, select_stride=4)


# ---- 1. ops and counts ----------------------------------------------------------------------------------------------------------

def _junk(s):
    """Entries that match nothing: out of range on every side, index == dim, INT_MIN / INT_MAX, occupied cells without a row."""
    d = np.asarray(s.dims, np.int32)
    out = np.array([[-1, 5, 5], [5, -1, 5], [5, 5, -1], [d[0], 5, 5], [5, d[1], 5], [5, 5, d[2]], [INT_MIN, INT_MIN, INT_MIN], [INT_MAX, 0, 0], [0, INT_MIN, 0],
                    [d[0] + 8, 0, 0], [0, 0, 0]], np.int32)
    at_dim = s.occ[(s.occ == d).any(axis=1)]
    inside = s.occ[(s.occ < d).all(axis=1)]
    no_row = inside[~np.isin(HR.keys(inside), HR.full_set(s.rows))]
    assert len(at_dim) >= 100 and len(no_row) >= 100, "occupied cells at index == dim and occupied cells without a row"
    assert (0, 0, 0) not in set(map(tuple, s.occ.tolist())), "(0, 0, 0) is a free cell"
    return np.ascontiguousarray(np.vstack([out, at_dim, no_row]).astype(np.int32))


@pytest.mark.parametrize("stride", [12, 64])
@pytest.mark.parametrize("form", ["host", "device"])
def test_list_ops_and_counts(hfpf_mod, session, form, stride):
    s = session
    s.g.show_all()
    junk = _junk(s)
    lists = [("hide", np.vstack([s.S, junk, s.S[::3], s.S[::-1][:500]])),          # duplicates and entries that match nothing
             ("show", np.vstack([s.S[::2], junk[:20], s.vox[5::7]])),               # half of what is hidden, some that is not
             ("hide_others", np.vstack([s.vox[::3], s.vox[::3], junk])),            # keep a third: cumulative
             ("hide", s.vox[:0]),                                                   # an empty list changes nothing
             ("show", s.vox),                                                       # everything again
             ("hide_others", s.vox[:0])]                                            # n = 0 hides everything
    H_ref = None
    for i, (op, v) in enumerate(lists):
        v = np.ascontiguousarray(v, np.int32)
        entries = _as_rows(hfpf_mod, v) if stride == 64 else v
        got = _call(s, form, entries, op)
        H_ref, want = HR.hide_voxels(s.rows, H_ref, s.dims, v, op)
        print("%s, stride %d, call %d (%s, %d entries): %r" % (form, stride, i, op, len(v), got))
        assert got == want, "call %d (%s): %r vs %r" % (i, op, got, want)
        _state(s, H_ref, "%s, stride %d, call %d (%s)" % (form, stride, i, op))
    assert len(H_ref) == len(s.rows) and len(s.g.extract()) == 0
    s.g.show_all()
    _state(s, s.vox[:0], "after show_all")


def test_box_ops_and_counts(session):
    s = session
    s.g.show_all()
    lo3, hi3 = HR.middle_third(s.rows)
    boxes = [("hide", lo3, hi3), ("hide", (-5, 60, -5), (300, 300, 300)), ("show", (40, INT_MIN, 10), (50, INT_MAX, 40)), ("hide", (50, 30, 40), (49, 71, 87)),
             ("hide", (104, 0, 0), (200, 71, 87)), ("hide", (7, 7, 7), (8, 8, 8)), ("hide", (0, 0, 0), (0, 71, 87)), ("hide_others", (0, 0, 0), (80, 71, 60)),
             ("show", (INT_MIN,) * 3, (INT_MAX,) * 3), ("hide_others", (10, 10, 10), (9, 9, 9))]
    H_ref = None
    for i, (op, lo, hi) in enumerate(boxes):
        got = s.g.hide_box(lo, hi, op)
        H_ref, want = HR.hide_box(s.rows, H_ref, s.dims, lo, hi, op)
        print("box %d (%s %r .. %r): %r" % (i, op, tuple(lo), tuple(hi), got))
        assert got == want, "box %d: %r vs %r" % (i, got, want)
        _state(s, H_ref, "box %d (%s)" % (i, op))
    assert len(H_ref) == len(s.rows), "HIDE_OTHERS of the empty box hides everything"
    s.g.show_all()
    # the box form and the list of the same voxels agree with S's box
    a = s.g.hide_box(lo3, hi3)
    assert a["n_matched"] == int(((s.vox[:, 0] >= lo3[0]) & (s.vox[:, 0] <= hi3[0])).sum()) > 1000
    s.g.show_all()


def test_select_through_consistency_flags_and_labels(hfpf_mod, session):
    s = session
    s.g.show_all()
    rows, cons, summary = s.g.depth_consistency(s.frames, s.poses, s.K, **CONS_KW)
    contra = (cons["flags"] & CS.CONTRADICTED) != 0
    print("consistency: %r" % (summary,))
    assert rows.tobytes() == s.rows.tobytes() and 1000 < contra.sum() < len(rows) - 1000, "some rows are contradicted, some are not"
    flags = cons["flags"]   # the flags word of hfpf_row_consistency: offset 24, stride 32
    assert flags.strides[0] == 32 and flags.ctypes.data - cons.ctypes.data == 24
    # host: the arrays of the call as they are
    got = s.g.hide_voxels(rows, "hide", select=flags, select_mask=CS.CONTRADICTED, select_value=CS.CONTRADICTED)
    H_ref, want = HR.hide_voxels(s.rows, None, s.dims, s.vox, "hide", flags, CS.CONTRADICTED, CS.CONTRADICTED)
    assert got == want and want["n_hidden"] == int(contra.sum()), (got, want)
    _state(s, H_ref, "contradicted rows, host form")
    again = s.g.depth_consistency(s.frames, s.poses, s.K, **CONS_KW)
    assert again[2]["n_contradicted"] == 0 and again[0].tobytes() == s.rows[~contra].tobytes(), "the contradicted rows are gone from the read-out that found them"
    s.g.show_all()
    # device: the arrays hfpf_depth_consistency_device returned, read in place
    with G.uploaded(s.g, s.frames) as (d,):
        desc = hfpf_mod.depth_desc(W, H, hfpf_mod.DEPTH_U16, 2 * W, s.K)
        r, c, nr, _ = s.g.depth_consistency_device(desc, d, s.frames.strides[0], len(s.frames), s.poses, **CONS_KW)
    try:
        got = s.g.hide_voxels(r, "hide", select=c + 24, select_mask=CS.CONTRADICTED, select_value=CS.CONTRADICTED, device=True, n=nr, voxel_stride=64, select_stride=32)
    finally:
        s.g.device_free(r), s.g.device_free(c)
    assert got == want
    _state(s, H_ref, "contradicted rows, device form")
    s.g.show_all()
    # labels: component c of a plain labelling, mask ~0
    rows, labels, comps = s.g.extract_components(reach=1)
    c = int(np.argsort(comps["n_rows"])[-2])   # the second largest component
    assert len(comps) >= 3 and 1 <= comps["n_rows"][c] < len(rows) // 2
    got = s.g.hide_voxels(rows, "hide", select=labels, select_mask=0xFFFFFFFF, select_value=c)
    H_ref, want = HR.hide_voxels(s.rows, None, s.dims, s.vox, "hide", labels, 0xFFFFFFFF, c)
    assert got == want and want["n_hidden"] == int(comps["n_rows"][c]), (got, want)
    _state(s, H_ref, "component %d, host form" % c)
    # ... and HIDE_OTHERS on the largest, with the device arrays: "keep only this component"
    # (this labelling sees component c hidden: its rows are not in the list, and stay hidden)
    rv, rl, rc = CR.components(HR.visible(s.rows, H_ref), reach=1)
    big = int(np.argmax(rc["n_rows"]))
    r, l, nr, cp, nc = s.g.extract_components(device=True, reach=1)
    try:
        assert s.g.device_download(l, nr * 4).view(np.uint32).tobytes() == rl.tobytes(), "the labels on the device"
        got = s.g.hide_voxels(r, "hide_others", select=l, select_mask=0xFFFFFFFF, select_value=big, device=True, n=nr, voxel_stride=64, select_stride=4)
    finally:
        for p in (r, l, cp):
            s.g.device_free(p)
    H_ref, want = HR.hide_voxels(s.rows, H_ref, s.dims, HR.row_voxels(rv), "hide_others", rl, 0xFFFFFFFF, big)
    assert got == want, (got, want)
    _state(s, H_ref, "keep the largest component, device form")
    assert len(s.g.extract()) == int(rc["n_rows"][big]) == int(comps["n_rows"].max())
    s.g.show_all()


def test_single_cells_planes_and_face_layers(session):
    """A cell at local bit 0 and one at bit 63 of a plane word, x-planes 0 and 7 of a brick, each hidden alone; then the rows of all
    six face layers."""
    s = session
    s.g.show_all()
    v = s.vox
    picks = {"bit 0": (v[:, 1] % 8 == 0) & (v[:, 2] % 8 == 0), "bit 63": (v[:, 1] % 8 == 7) & (v[:, 2] % 8 == 7), "x-plane 0": v[:, 0] % 8 == 0,
             "x-plane 7": v[:, 0] % 8 == 7}
    lo = faces.lo_hi(s.bbox)[0]
    for what, m in picks.items():
        live = np.flatnonzero(m & (s.rows["count"] > 0))
        assert len(live) >= 10, what
        one = np.ascontiguousarray(v[live[len(live) // 2]].reshape(1, 3))
        centre = (lo + (one.astype(np.float64) + 0.5) * s.res).astype(np.float32)   # a point of the cell itself
        assert (s.g.query(centre, IDENT, radius=0)[0]["flags"] & Q.HAS_ROW).all(), "%s: the cell has a row" % what
        c = s.g.hide_voxels(one)
        assert c == dict(n_selected=1, n_matched=1, n_changed=1, n_hidden=1, n_full=len(s.rows)), (what, c)
        _state(s, one, what)
        assert not (s.g.query(centre, IDENT, radius=0)[0]["flags"] & Q.HAS_ROW).any(), "%s: the hidden cell still has a row for a query" % what
        c = s.g.hide_voxels(one, "show")
        assert c["n_changed"] == 1 and c["n_hidden"] == 0
    d = np.asarray(s.dims)
    layer = ((v == 0) | (v == d - 1)).any(axis=1)
    for a in range(3):
        assert (v[:, a] == 0).sum() >= 20 and (v[:, a] == d[a] - 1).sum() >= 20, "rows in both face layers of axis %d" % a
    c = s.g.hide_voxels(np.ascontiguousarray(v[layer]))
    H_ref, want = HR.hide_voxels(s.rows, None, s.dims, v[layer])
    assert c == want and c["n_hidden"] == int(layer.sum())
    _state(s, H_ref, "the six face layers")
    s.g.show_all()


# ---- 2. every read-out honours H ------------------------------------------------------------------------------------------------

PARTS = ("rows_render_query", "mesh", "raycast", "components_compare_cover_consistency", "align", "track")


def _readouts(s, vis, what, parts=PARTS):
    """The read-outs of `parts` on s.g against their restatements on the rows `vis` and the unchanged occupied list.  Returns figures
    for the floors (what the same restatement gives on all rows is computed once a session and shared)."""
    g, occ, bbox, res, dims = s.g, s.occ, s.bbox, s.res, s.dims
    fig = {}
    cache = s.__dict__.setdefault("unmasked", {})
    if "rows_render_query" in parts:
        G.same_records(g.extract(), vis, "%s: extract" % what, "rows")
        G.same_records(g.extract_filtered(min_count=3.0), vis[vis["count"].astype(np.int32) >= 3], "%s: extract_filtered" % what, "rows")
        K, z_range = (300.0, 300.0, 159.5, 119.5), (0.05, 3.0)
        got = g.render(s.sc.poses[0], K, W, H, z_range=z_range, min_count=1, splat_radius=2, max_splat_radius=4, cull_backfaces=True, world_normals=True)
        G.same_planes(got, R.render(vis, s.sc.poses[0], K, W, H, res, z_range, 1, 2, 4, R.CULL_BACKFACES | R.WORLD_NORMALS), "%s: render" % what)
        fig["render_pixels"] = int((~np.isnan(got["depth"])).sum())
        # query: host, device, depth
        pts = faces.query_points(s.rows, bbox, res, dims)
        ref = Q.query(vis, occ, pts, IDENT, bbox, res, **HR.FLOOR_QUERY)
        G.same_query(g.query(pts, IDENT, **HR.FLOOR_QUERY), ref, "%s: query, host form" % what)
        with G.uploaded(g, pts) as (d,):
            G.same_query(g.query_device(d, len(pts), IDENT, **HR.FLOOR_QUERY), ref, "%s: query, device form" % what)
        if "query" not in cache:
            cache["query"] = Q.query(s.rows, occ, pts, IDENT, bbox, res, **HR.FLOOR_QUERY)[0]
        fig["query_changed"] = HR.changed_records(ref[0], cache["query"])
        kw = dict(radius=2, min_count=2.0, max_distance=3 * res, zclip=True)
        G.same_query(g.query_depth(s.frames[2], s.poses[2], s.K, **kw), Q.query(vis, occ, Q.depth_points(s.frames[2], s.K), s.poses[2], bbox, res, G.Z_CLIP, **kw),
                     "%s: query_depth" % what)
    if "mesh" in parts:  # host, device
        rv, rt, _ = M.mesh(vis, occ, bbox, res, dims, radius=2)
        G.same_mesh(g.extract_mesh(radius=2), (rv, rt), "%s: mesh, host form" % what)
        G.same_mesh(G.mesh_device(g, radius=2), (rv, rt), "%s: mesh, device form" % what)
        fig["masked_triangles"] = len(rt)
    if "raycast" in parts:  # general and view
        rays = faces.rays(bbox, res)[::HR.FLOOR_RAYS_EVERY]
        kw = dict(HR.FLOOR_RAYS, t_range=(0.0, faces.ray_t_max(bbox, res, STEP)))
        ref = RC.raycast(vis, occ, rays, IDENT, bbox, res, **kw)
        G.same_rays(g.raycast(rays, IDENT, **kw), ref, "%s: raycast, host form" % what)
        G.same_rays(G.rays_device(g, rays, IDENT, **kw), ref, "%s: raycast, device form" % what)
        if "rays" not in cache:
            cache["rays"] = RC.raycast(s.rows, occ, rays, IDENT, bbox, res, **kw)
        fig["rays_changed"] = HR.changed_records(ref, cache["rays"])
        pose, VK = faces.outside_view(bbox, 80, 60)
        lo, hi = faces.lo_hi(bbox)
        kw = dict(radius=2, step=STEP, t_range=(0.06, 0.08 + float(hi[2] - lo[2]) + 0.01))
        ref = RC.raycast_view(vis, occ, pose, VK, 80, 60, bbox, res, **kw)
        G.same_rays(g.raycast_view(pose, VK, 80, 60, **kw), ref, "%s: raycast_view" % what)
        fig["view_hits"] = int((ref["flags"] & RC.HIT != 0).sum())
    if "components_compare_cover_consistency" in parts:
        kw = dict(reach=2, min_normal_dot=0.9, min_rows=20)
        ref = CR.components(vis, **kw)
        G.same_components(g.extract_components(**kw), ref, "%s: components, host form" % what)
        G.same_components(G.components_device(g, s.H, **kw), ref, "%s: components, device form" % what)
        fig["components"] = len(ref[2])
        # compare and cover against the session's own mesh of ALL rows
        v, t, dv, dt = s.own_mesh()
        G.same_deviation(G.compare_device(g, s.H, dv, len(v), 32, dt, len(t), IDENT, max_distance=3 * res), D.compare(vis, v, 32, t, IDENT, 0.0, 3 * res),
                         "%s: compare_mesh" % what)
        ckw = dict(radius=2, max_distance=2 * res, spacing=res)
        cov = G.cover_device(g, s.H, dv, len(v), 32, dt, len(t), IDENT, **ckw)
        G.same_coverage(cov, V.cover(vis, occ, v, 32, t, IDENT, bbox, res, **ckw), "%s: cover_mesh" % what)
        fig["covered"], fig["samples"] = cov[1]["n_covered"], cov[1]["n_samples"]
        ref = CS.consistency(vis, s.frames, s.poses, s.K, **CONS_KW)
        got = g.depth_consistency(s.frames, s.poses, s.K, **CONS_KW)
        G.same_records(got[:2], ref[:2], "%s: depth_consistency" % what, ("rows", "records"))
        G.same_summary(got[2], ref[2], CS.SUMMARY_KEYS, "%s: depth_consistency" % what)
        fig["contradicted"] = ref[2]["n_contradicted"]
    if "align" in parts:
        v, t, dv, dt = s.own_mesh()
        start = A.rigid(0.3, (0.5, 1.0, -0.4), tuple(np.array([0.6, -0.64, 0.48]) * 2 * res), A.centre(bbox))
        akw = dict(ALIGN_KW, max_distance=8 * res)
        ref = A.align(vis, v, 32, t, start, bbox, **akw)
        G.same_align(g.align_mesh(dv, dt, start, device=True, n_verts=len(v), vertex_stride=32, n_tris=len(t), **akw), ref, "%s: align_mesh, device form" % what)
        G.same_align(g.align_mesh(v, t, start, **akw), ref, "%s: align_mesh, host form" % what)
        fig["align_inliers"], fig["align_sampled"] = ref["inliers"], ref["rows_sampled"]
    if "track" in parts:  # the held-out frame of the stream
        guess = G.perturb(s.poses[2], 2.0, (0.006, -0.005, 0.006))
        ref = G.track_reference(vis, TR.depth_points(s.frames[2], s.K, 1), guess, s.K, W, H)
        G.same_track(g.track_depth(s.frames[2], guess, s.K, stride=1, **G.TRACK_OPTS), ref, "%s: track_depth" % what)
        fig["track_inliers"], fig["track_iterations"] = ref["inliers"], ref["iterations"]
    return fig


@pytest.mark.parametrize("part", PARTS)
def test_every_read_out_honours_the_hidden_set(hfpf_mod, synth_mod, session, part):
    """With S hidden, each read-out equals, byte for byte, its restatement fed with the unmasked rows minus S and the unchanged
    occupied list.  The floors of tests/hide_ref.py keep a mask that hides nothing, or everything, from passing."""
    s = session
    assert s.sc.resolution == G.RES, "track_reference restates the render at RES"
    _hide_S(s)
    fig = _readouts(s, s.vis, "S hidden", (part,))
    print("S hidden, %s: %r" % (part, fig))
    for k in ("query_changed", "rays_changed", "masked_triangles"):
        if k in fig:
            assert fig[k] >= HR.CUT_FLOOR[k], "%s: %d, floor %d" % (k, fig[k], HR.CUT_FLOOR[k])
    if part == "rows_render_query":
        assert fig["render_pixels"] > 1000
    if part == "mesh":
        assert fig["masked_triangles"] < len(s.own_mesh()[1]), "the masked mesh has fewer triangles than the mesh of all rows"
    if part == "raycast":
        assert fig["view_hits"] >= 100
    if part == "components_compare_cover_consistency":
        assert fig["components"] >= 2 and 0 < fig["covered"] < fig["samples"] and fig["contradicted"] > 100
    if part == "align":
        assert fig["align_inliers"] > 100
    if part == "track":
        assert fig["track_inliers"] > 1000 and fig["track_iterations"] > 1
    # occupancy, counters and dirtiness do not see H
    assert s.g.occupied().tobytes() == s.occ.tobytes() and G.counters(s.g) == s.counters and not s.g.state_changed
    s.g.show_all()
    G.same_records(s.g.extract(), s.rows, "after show_all", "rows")


def test_everything_hidden_reads_as_a_model_without_rows(hfpf_mod, synth_mod, session):
    """HIDE_OTHERS with n = 0: every read-out returns what it returns on a handle before its first clean pass -- the restatements on
    no rows and the unchanged occupied list; the arrays are empty."""
    s = session
    s.g.show_all()
    c = s.g.hide_voxels(s.vox[:0], "hide_others")
    assert c == dict(n_selected=0, n_matched=0, n_changed=len(s.rows), n_hidden=len(s.rows), n_full=len(s.rows)), c
    fig = _readouts(s, s.rows[:0], "everything hidden")
    assert len(s.g.extract()) == 0 and len(s.g.extract_mesh(radius=2)[0]) == 0 and len(s.g.extract_components()[0]) == 0
    hits, _ = s.g.query(faces.query_points(s.rows, s.bbox, s.res, s.dims), IDENT, radius=4)
    assert not (hits["flags"] & (Q.HAS_ROW | Q.FOUND)).any() and (hits["flags"] & Q.OCCUPIED).sum() > 1000, "no row anywhere, occupancy as before"
    assert fig["track_inliers"] == 0 and fig["render_pixels"] == 0 and fig["masked_triangles"] == 0 and fig["view_hits"] == 0
    assert s.g.occupied().tobytes() == s.occ.tobytes() and G.counters(s.g) == s.counters
    s.g.show_all()
    G.same_records(s.g.extract(), s.rows, "after show_all", "rows")


# ---- 3. fusion does not see H ----------------------------------------------------------------------------------------------------

def _integrate(g, sc, f):
    """One frame of a scenes.Scene, as scenes.run hands it over."""
    lay = sc.layout
    g.integrate(sc.frame(f), sc.poses[f], point_step=lay["point_step"], off_x=lay["off_x"], off_y=lay["off_y"], off_z=lay["off_z"], off_rgb=lay["off_rgb"])


def test_fusion_does_not_see_the_hidden_set(hfpf_mod, synth_mod, session):
    """Handle b hides S1 after the first clean pass of the schedule and takes the remaining frames and passes: the rows of S1 stay
    hidden, voxels that got their row later are visible, and after show_all b is handle a, which never hid anything."""
    s = session
    sc = s.sc
    kw = dict(resolution=sc.resolution, bbox=sc.bbox, fuse_color=True, **sc.config, **G.SMALL_CAPS)
    with hfpf_mod.OccupancyGrid(**kw) as b:
        seen = {}

        def between(g, i):
            if "S1" not in seen and not g.state_changed and len(g.extract()):
                seen["rows1"] = g.extract().copy()
                seen["S1"] = HR.hidden_set(seen["rows1"])
                c = g.hide_voxels(seen["S1"])
                assert c["n_hidden"] == len(seen["S1"]) == c["n_changed"]

        G.run(b, sc, between=between, integrate=lambda g, f: _integrate(g, sc, f))
        S1, rows1 = seen["S1"], seen["rows1"]
        later = ~np.isin(HR.keys(HR.row_voxels(s.rows)), HR.full_set(rows1))
        print("%d rows after the first pass, %d hidden then, %d rows came later" % (len(rows1), len(S1), later.sum()))
        assert 1000 < len(rows1) < len(s.rows) and later.sum() > 1000 and len(S1) > 300
        assert b.hidden().tobytes() == S1.tobytes(), "H lasts through integrate and clean"
        got = b.extract()
        G.same_records(got, HR.visible(s.rows, S1), "b with S1 hidden", "rows")
        assert np.isin(HR.keys(HR.row_voxels(s.rows[later])), HR.keys(HR.row_voxels(got))).all(), "a voxel that got its row later is visible"
        assert b.occupied().tobytes() == s.occ.tobytes()
        b.show_all()
        assert b.extract().tobytes() == s.rows.tobytes() and b.occupied().tobytes() == s.occ.tobytes(), "after show_all b is a"
        assert G.contract_counters(b) == G.contract_counters(s.g), "%r vs %r" % (G.contract_counters(b), G.contract_counters(s.g))
        assert len(b.snapshot()) == len(s.blob), "and its snapshot has no HIDDEN section"


# ---- 4. snapshot -----------------------------------------------------------------------------------------------------------------

def test_snapshot_carries_the_hidden_set(hfpf_mod, synth_mod, session):
    s = session
    # (the counter section of a snapshot holds the row count of the last row set built, a scratch word: every snapshot compared here is
    # taken behind a plain extract)
    s.g.show_all()
    s.g.extract()
    assert s.g.snapshot().tobytes() == s.blob, "hide, show_all, snapshot: the blob of a handle that never hid anything"
    _hide_S(s)
    s.g.extract()
    blob = s.g.snapshot()
    assert len(blob) > len(s.blob), "the HIDDEN section is there"
    mesh = s.g.extract_mesh(radius=2)
    larger = dict(G.SMALL_CAPS, max_bricks=100000, max_normals=2 << 20, max_frames=8192)  # (max_log_points must be the snapshot's)
    with hfpf_mod.OccupancyGrid(resolution=s.sc.resolution, bbox=s.bbox, fuse_color=True, **s.sc.config, **larger) as g2:
        g2.restore(blob)
        again = g2.snapshot()
        assert again.tobytes()[hfpf_mod.SNAPSHOT_HEADER_BYTES:] == blob.tobytes()[hfpf_mod.SNAPSHOT_HEADER_BYTES:], "the payload of the snapshot of the restore"
        assert g2.hidden().tobytes() == s.S.tobytes(), "hfpf_get_hidden on the restored handle"
        G.same_records(g2.extract(), s.vis, "restored: extract", "rows")
        G.same_mesh(g2.extract_mesh(radius=2), mesh, "restored: mesh")
        assert g2.occupied().tobytes() == s.occ.tobytes()
        # a blob without the section empties a set that was there
        g2.restore(s.blob)
        assert len(g2.hidden()) == 0 and g2.extract().tobytes() == s.rows.tobytes()
        g2.restore(blob)
        g2.show_all()
        g2.extract()
        assert g2.snapshot().tobytes()[hfpf_mod.SNAPSHOT_HEADER_BYTES:] == s.blob[hfpf_mod.SNAPSHOT_HEADER_BYTES:], "restore, show_all, snapshot"
        # hfpf_clear empties H: the same stream again gives all rows
        g2.restore(blob)
        g2.clear()
        assert len(g2.hidden()) == 0 and len(g2.extract()) == 0
        assert scenes.run(g2, s.sc, "integrate").tobytes() == s.rows.tobytes() and len(g2.hidden()) == 0
    s.g.show_all()
    s.g.extract()
    assert s.g.snapshot().tobytes() == s.blob


# ---- 5. the largest indices ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["deepx", "deep3"])
def test_largest_indices(hfpf_mod, synth_mod, name):
    """deepx: cell indices up to 2,097,149; deep3: every row's linear directory index above 2^31.  Half the rows hidden by list and
    by box; the extract and one query set against the restatements."""
    s = G.Session(hfpf_mod, name)
    try:
        v = HR.row_voxels(s.rows).astype(np.int32)
        d = np.asarray(s.dims, np.int32)
        junk = np.array([[d[0], v[0, 1], v[0, 2]], [-1, 0, 0], [INT_MIN, INT_MIN, INT_MIN], [d[0] - 1, d[1] - 1, d[2]]], np.int32)
        pts = faces.query_points(s.rows, s.bbox, s.res, s.dims)[::4]
        x_mid = int(np.median(v[:, 0]))
        lst = np.ascontiguousarray(np.vstack([v[::2], junk, v[v[:, 0] == d[0] - 1][:8]]))   # every other row, and some at index dim - 1
        calls = [("list", lambda: s.g.hide_voxels(lst), lambda: HR.hide_voxels(s.rows, None, s.dims, lst)),
                 ("box", lambda: s.g.hide_box((x_mid, 0, 0), (INT_MAX, INT_MAX, INT_MAX)), lambda: HR.hide_box(s.rows, None, s.dims, (x_mid, 0, 0), (INT_MAX,) * 3))]
        for what, call, ref in calls:
            s.g.show_all()
            got = call()
            H_ref, want = ref()
            print("%s, %s: %r" % (name, what, got))
            assert got == want and len(s.rows) // 3 < got["n_hidden"] < 2 * len(s.rows) // 3, (what, got, want)
            assert s.g.hidden().tobytes() == H_ref.tobytes(), "%s: hfpf_get_hidden" % what
            vis = HR.visible(s.rows, H_ref)
            G.same_records(s.g.extract(), vis, "%s, %s: extract" % (name, what), "rows")
            ref_q = Q.query(vis, s.occ, pts, IDENT, s.bbox, s.res, radius=2)
            G.same_query(s.g.query(pts, IDENT, radius=2), ref_q, "%s, %s: query" % (name, what))
            assert HR.changed_records(ref_q[0], Q.query(s.rows, s.occ, pts, IDENT, s.bbox, s.res, radius=2)[0]) > 500
            assert int(H_ref[:, 0].max()) == s.dims[0] - 1, "a hidden row at index dim - 1"
        if name == "deep3":
            assert (faces.brick_lin(s.rows, s.dims)[::2] > 2 ** 31).all(), "every hidden row's directory index lies above 2^31"
        s.g.show_all()
        assert s.g.extract().tobytes() == s.rows.tobytes()
    finally:
        s.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_leave_the_hidden_set_and_the_rows_alone(hfpf_mod, session):
    s = session
    H_ = hfpf_mod
    L = H_.lib()
    _hide_S(s)
    v = np.ascontiguousarray(s.vox[::5])
    words = np.zeros(len(v), np.uint32)
    vp, wp = C.c_void_p(v.ctypes.data), C.c_void_p(words.ctypes.data)
    res = H_.HideResult()
    res.struct_size = C.sizeof(H_.HideResult)
    marker = 0x5A5A5A5A5A5A5A5A
    res.n_hidden = marker

    def opts(**kw):
        o = H_.hide_opts("show")
        for k, x in kw.items():
            setattr(o, k, x)
        return o

    bad_opts = [opts(struct_size=20), opts(struct_size=0), opts(op=0), opts(op=4), opts(op=0xFFFFFFFF), opts(flags=1), opts(reserved=1)]
    for o in bad_opts:
        assert H_.check_hide_opts(o) == -2
        assert L.hfpf_hide_voxels(s.g._h, C.byref(o), vp, len(v), 12, None, 0, C.byref(res)) == -2
    assert H_.check_hide_opts(None) == -2 and H_.check_hide_opts(opts()) == 0
    assert L.hfpf_hide_voxels(s.g._h, None, vp, len(v), 12, None, 0, C.byref(res)) == -2, "NULL opts"
    ok = opts()
    for vs, ss, sel in ((8, 0, None), (0, 0, None), (13, 0, None), (14, 0, None), (12, 0, wp), (12, 2, wp), (12, 6, wp)):
        assert L.hfpf_hide_voxels(s.g._h, C.byref(ok), vp, len(v), vs, sel, ss, C.byref(res)) == -2, (vs, ss)
    assert L.hfpf_hide_voxels(s.g._h, C.byref(ok), None, 5, 12, None, 0, C.byref(res)) == -2, "NULL voxels with n > 0"
    short = H_.HideResult()
    short.struct_size = 40
    assert L.hfpf_hide_voxels(s.g._h, C.byref(ok), vp, len(v), 12, None, 0, C.byref(short)) == -2, "a result of another size"
    assert L.hfpf_hide_box(s.g._h, H_.SHOW, v[0].ctypes.data, v[1].ctypes.data, C.byref(short)) == -2
    with G.uploaded(s.g, v, words) as (dv, dw):
        assert L.hfpf_hide_voxels_device(s.g._h, C.byref(ok), C.c_void_p(dv + 2), len(v) - 1, 12, None, 0, C.byref(res)) == -2, "a misaligned device list"
        assert L.hfpf_hide_voxels_device(s.g._h, C.byref(ok), C.c_void_p(dv), len(v), 12, C.c_void_p(dw + 1), 4, C.byref(res)) == -2, "a misaligned device selector"
    lo = np.zeros(3, np.int32)
    hi = np.full(3, 1000, np.int32)
    for op in (0, 4, 99):
        assert L.hfpf_hide_box(s.g._h, op, lo.ctypes.data, hi.ctypes.data, C.byref(res)) == -2, op
    assert L.hfpf_hide_box(s.g._h, H_.SHOW, None, hi.ctypes.data, C.byref(res)) == -2 and L.hfpf_hide_box(s.g._h, H_.SHOW, lo.ctypes.data, None, C.byref(res)) == -2
    assert L.hfpf_get_hidden(s.g._h, None, 0, None) == -2
    assert res.n_hidden == marker, "a refused call wrote its result"
    _state(s, s.S, "after the refused calls")
    # NULL res and a NULL list with n = 0 are fine
    assert L.hfpf_hide_voxels(s.g._h, C.byref(ok), None, 0, 12, None, 0, None) == 0
    assert L.hfpf_hide_box(s.g._h, H_.SHOW, hi.ctypes.data, lo.ctypes.data, None) == 0
    _state(s, s.S, "after two calls that match nothing")
    n = C.c_uint64()
    few = np.full((4, 3), -7, np.int32)
    assert L.hfpf_get_hidden(s.g._h, few.ctypes.data, 3, C.byref(n)) == 0 and n.value == len(s.S), "cap below the count"
    assert few[:3].tobytes() == s.S[:3].tobytes() and (few[3] == -7).all(), "at most cap triplets are written"
    s.g.show_all()


def test_empty_uncleaned_and_exchanging_handles(hfpf_mod, synth_mod, session):
    s = session
    sc = s.sc
    kw = dict(resolution=sc.resolution, bbox=sc.bbox, fuse_color=True, **sc.config, **G.SMALL_CAPS)
    zeros = dict.fromkeys(HR.COUNTS, 0)
    with hfpf_mod.OccupancyGrid(**kw) as g:
        for label in ("empty", "before its first clean pass"):
            before = g.counters()["device_bytes"]
            assert g.hide_voxels(s.vox) == zeros and g.hide_box((0, 0, 0), (50, 50, 50), "hide_others") == zeros, label
            assert g.hide_voxels(s.vox[:0], "hide_others") == zeros and len(g.hidden()) == 0, label
            g.show_all()
            assert g.counters()["device_bytes"] == before, "%s: a call on a handle without rows allocates nothing" % label
            _integrate(g, sc, 0)
        g.clean()
        assert g.hide_voxels(s.vox, "show")["n_hidden"] == 0 and g.hide_voxels(s.vox[:0])["n_hidden"] == 0
        mid = g.counters()["device_bytes"]
        c = g.hide_voxels(s.vox[:0], "hide_others")
        assert c["n_hidden"] == c["n_full"] == g.counters()["voxels_with_normal"] > 0 and len(g.extract()) == 0
        assert g.counters()["device_bytes"] - mid >= 64 * G.SMALL_CAPS["max_bricks"], "the hidden bits come with the first call that hides a row, counted in device_bytes"
        g.clear()
        assert len(g.hidden()) == 0
    with hfpf_mod.OccupancyGrid(**kw) as g:
        _integrate(g, sc, 0)
        g.epoch_export()
        for call in (lambda: g.hide_voxels(s.vox), lambda: g.hide_box((0, 0, 0), (5, 5, 5)), g.show_all, g.hidden):
            with pytest.raises(hfpf_mod.HfpfError) as e:
                call()
            assert e.value.code == -5, "a handle that has exported epoch records: HFPF_ERR_STATE, as hfpf_snapshot"
        with pytest.raises(hfpf_mod.HfpfError) as e:
            g.snapshot()
        assert e.value.code == -5
