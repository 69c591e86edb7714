"""The view-planning contract of include/hfpf.h restated in numpy (imported by tests only): hfpf_extract's rows, hfpf_get_occupied's
list, a triangle mesh, its pose, the options and the candidate camera poses -> the scores, the per-triangle records and the summary
hfpf_plan_views* return.  The samples and their test are cover_ref's (whose sample test is query_ref's), the rows of
HFPF_PLAN_MODEL_OCCLUDES and the auto radius are render_ref's; everything else is f64, one rounding per operation, in the order the
header writes it.  Depth buffers are uint32 words reduced with np.minimum.at; every sum is made of Python integers."""
import numpy as np

import cover_ref as V
import query_ref as Q
import render_ref as R

VIEW_SCORE_DTYPE = np.dtype([("rank", "<i4"), ("n_in_view", "<u4"), ("n_facing", "<u4"), ("n_visible", "<u4"), ("visible_q40", "<u8"),
                             ("gain_q40", "<u8"), ("gain_samples", "<u8")])
TRI_PLAN_DTYPE = np.dtype([("n_targets", "<u4"), ("n_reachable", "<u4"), ("n_planned", "<u4"), ("flags", "<u4")])
assert VIEW_SCORE_DTYPE.itemsize == 40 and TRI_PLAN_DTYPE.itemsize == 16
TWO_SIDED, MODEL_OCCLUDES = 1, 2
SUMMARY_KEYS = ("n_views", "n_selected", "n_targets", "n_reachable", "n_planned", "target_q40", "reachable_q40", "planned_q40")
EMPTY = np.uint32(0xFFFFFFFF)


def project(p, pose, K, z_lo, z_far):
    """The render contract's projection of f32 points: (ok = z_lo < zc < z_far and |u|, |v| < 2^30; dx, dy, dz, zc, pu, pv)."""
    T = np.asarray(pose, np.float64).reshape(12)
    fx, fy, cx, cy = (float(k) for k in K)
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        dx, dy, dz = x - T[3], y - T[7], z - T[11]
        xc = (T[0] * dx + T[4] * dy) + T[8] * dz
        yc = (T[1] * dx + T[5] * dy) + T[9] * dz
        zc = (T[2] * dx + T[6] * dy) + T[10] * dz
        ok = (float(z_lo) < zc) & (zc < float(z_far))
        u = (xc / zc) * fx + cx
        v = (yc / zc) * fy + cy
        ok &= (np.abs(u) < 2.0 ** 30) & (np.abs(v) < 2.0 ** 30)
        pu = np.where(ok, np.floor(u + 0.5), 0.0).astype(np.int64)
        pv = np.where(ok, np.floor(v + 0.5), 0.0).astype(np.int64)
    return ok, dx, dy, dz, zc, pu, pv


def splat(zb, width, height, zc, pu, pv, r):
    """zb[pixel] = min(zb[pixel], bits((float)zc)) over every candidate's window (r per candidate), inside the image."""
    words = zc.astype(np.float32).view(np.uint32)
    for rad in np.unique(r):
        sel = np.flatnonzero(r == rad)
        off = np.arange(-rad, rad + 1, dtype=np.int64)
        px = (pu[sel][:, None, None] + off[None, None, :]).repeat(off.size, axis=1)
        py = (pv[sel][:, None, None] + off[None, :, None]).repeat(off.size, axis=2)
        w = np.broadcast_to(words[sel][:, None, None], px.shape)
        inside = (px >= 0) & (px < width) & (py >= 0) & (py < height)
        np.minimum.at(zb, (py * width + px)[inside], w[inside])


def splat_radii(n, scale, K, zc, splat_radius, max_splat_radius):
    """r per candidate: the fixed one, or the auto radius with `scale` (cover.spacing for samples, res for rows)."""
    if splat_radius >= 0:
        return np.full(n, int(splat_radius), np.int64)
    return R.auto_radius(scale, K[0], K[1], zc, max_splat_radius)


def depth_buffer(p_all, rows, pose, K, width, height, z_far, occluder_near, spacing, res, splat_radius, max_splat_radius, cull, view_min_count):
    """zmin of one view as uint32 words (all ones = no occluder): the finite samples, and `rows` (or None) as a render draws them."""
    zb = np.full(width * height, EMPTY, np.uint32)
    fin = np.isfinite(p_all).all(axis=1)
    ok, _, _, _, zc, pu, pv = project(p_all, pose, K, occluder_near, z_far)
    at = np.flatnonzero(ok & fin)
    splat(zb, width, height, zc[at], pu[at], pv[at], splat_radii(at.size, spacing, K, zc[at], splat_radius, max_splat_radius))
    if rows is not None:
        drawn = R.drawn_rows(rows, view_min_count)
        ok, zc, pu, pv = R.project(drawn, pose, K, (occluder_near, z_far), cull=cull)
        at = np.flatnonzero(ok)
        splat(zb, width, height, zc[at], pu[at], pv[at], splat_radii(at.size, res, K, zc[at], splat_radius, max_splat_radius))
    return zb


def classes(p, N, NN, pose, K, width, height, z_range, zb, min_cos, tolerance, slope, two_sided):
    """(IN_VIEW, FACING, VISIBLE) per target with point p and triangle normal N in the view whose depth buffer is zb."""
    ok, dx, dy, dz, zc, pu, pv = project(p, pose, K, z_range[0], z_range[1])
    in_view = ok & (pu >= 0) & (pu < width) & (pv >= 0) & (pv < height)
    with np.errstate(all="ignore"):
        c = -((N[:, 0] * dx + N[:, 1] * dy) + N[:, 2] * dz)
        d2 = (dx * dx + dy * dy) + dz * dz
        passes = c * c >= ((float(min_cos) * float(min_cos)) * NN) * d2
        gate = np.ones(len(p), bool) if float(min_cos) < 0.0 else (((c > 0.0) | bool(two_sided)) & passes)
        facing = in_view & gate
        pix = np.where(in_view, pv * width + pu, 0)
        depth32 = zc.astype(np.float32)
        zmin = zb[pix].view(np.float32)
        visible = facing & ((depth32.astype(np.float64) - zmin.astype(np.float64)) <= float(tolerance) + float(slope) * zc)
    return in_view, facing, visible


def weights(n, NN, valid):
    """w_s per triangle as Python integers: rint((area_d / n_samples) * 2^40), 0 for a HUGE or an invalid triangle."""
    out = []
    for k in range(len(valid)):
        area_d = 0.5 * float(np.sqrt(NN[k]))
        if not valid[k] or not area_d < 2.0 ** 23:
            out.append(0)
        else:
            out.append(int(np.rint((area_d / float(int(n[k]) * int(n[k]))) * 2.0 ** 40)))
    return out


def weighted(mask, tri, w, n_tris):
    """(the sum of w over the targets of mask, their number), through the per-triangle counts, as Python integers."""
    cnt = np.bincount(tri[mask], minlength=n_tris)
    return sum(int(cnt[k]) * w[k] for k in np.flatnonzero(cnt)), int(mask.sum())


def greedy(vis, tri, w, n_tris, max_views, min_gain_q40):
    """The selection over vis (views x targets, bool): [(view, G, C)] in rank order and the targets left over."""
    remaining = np.ones(vis.shape[1], bool)
    chosen, taken = [], set()
    for _ in range(int(max_views)):
        best = None
        for v in range(len(vis)):
            if v in taken:
                continue
            G, Cn = weighted(vis[v] & remaining, tri, w, n_tris)
            if best is None or (G, Cn) > (best[1], best[2]):  # strict: the smaller index keeps a tie
                best = (v, G, Cn)
        if best is None or best[1] < max(1, int(min_gain_q40)):
            break
        chosen.append(best)
        taken.add(best[0])
        remaining &= ~vis[best[0]]
    return chosen, remaining


def plan(rows, occupied, verts, stride, tris, pose, poses, bbox, res, K, width, height, radius=2, min_count=0.0, max_distance=0.01, spacing=0.005,
         max_subdivision=64, min_normal_dot=-2.0, abs_normal=False, z_range=(0.01, 100.0), view_min_count=0.0, splat_radius=0,
         max_splat_radius=4, cull_backfaces=False, occluder_near=None, min_cos=0.0, tolerance=0.004, slope=0.0, min_gain_q40=0, max_views=8,
         two_sided=False, model_occludes=False, n_verts=None):
    """(scores of VIEW_SCORE_DTYPE, records of TRI_PLAN_DTYPE, summary dict with the coverage summary under "coverage") as
    hfpf_plan_views returns them.  The cover keywords are cover_ref.cover's; view_min_count is the view's min_count."""
    poses = np.asarray(poses, np.float64).reshape(-1, 12)
    occluder_near = float(z_range[0] if occluder_near is None else occluder_near)
    A, ab, ac, N, NN, L2, valid = V.geometry(verts, stride, tris, pose, n_verts)
    n, capped = V.subdivision(L2, spacing, max_subdivision)
    n = np.where(valid, n, 0).astype(np.uint32)
    tri, S = V.sample_points(A, ab, ac, n)
    with np.errstate(all="ignore"):
        p = S.astype(np.float32)
    hits, hrows = Q.query(rows, occupied, p, V.IDENT, bbox, res, radius=radius, min_count=min_count, max_distance=max_distance)
    in_bbox = (hits["flags"] & Q.IN_BBOX) != 0
    found = (hits["flags"] & Q.FOUND) != 0
    normals = np.stack([hrows[k].astype(np.float64) for k in ("nx", "ny", "nz")], axis=1)
    covered = found & V.normal_gate(N, NN, tri, normals, min_normal_dot, abs_normal)
    cov, area_d = V.records(n, capped, NN, valid, tri, in_bbox, covered, hits["distance"])
    coverage = V.summary(cov, area_d)
    assert (coverage["area_q40_hi"] << 32) + coverage["area_q40_lo"] < 2 ** 62, "HFPF_ERR_CAPACITY: the mesh's area"

    n_tris = len(valid)
    target = in_bbox & ~covered
    tt, tp = tri[target], p[target]
    w = weights(n, NN, valid)
    vis = np.zeros((len(poses), len(tt)), bool)
    scores = np.zeros(len(poses), VIEW_SCORE_DTYPE)
    scores["rank"] = -1
    for v, T in enumerate(poses):
        zb = depth_buffer(p, rows if model_occludes else None, T, K, width, height, z_range[1], occluder_near, spacing, res, splat_radius,
                          max_splat_radius, cull_backfaces, view_min_count)
        in_view, facing, vis[v] = classes(tp, N[tt], NN[tt], T, K, width, height, z_range, zb, min_cos, tolerance, slope, two_sided)
        scores["n_in_view"][v], scores["n_facing"][v], scores["n_visible"][v] = in_view.sum(), facing.sum(), vis[v].sum()
        scores["visible_q40"][v] = weighted(vis[v], tt, w, n_tris)[0]
    chosen, remaining = greedy(vis, tt, w, n_tris, max_views, min_gain_q40)
    for k, (v, G, Cn) in enumerate(chosen):
        scores["rank"][v], scores["gain_q40"][v], scores["gain_samples"][v] = k, G, Cn
    everything = np.ones(len(tt), bool)
    reachable = vis.any(axis=0) if len(poses) else ~everything
    planned = ~remaining
    rec = np.zeros(n_tris, TRI_PLAN_DTYPE)
    rec["flags"] = cov["flags"]
    rec["n_targets"] = np.bincount(tt, minlength=n_tris)
    rec["n_reachable"] = np.bincount(tt[reachable], minlength=n_tris)
    rec["n_planned"] = np.bincount(tt[planned], minlength=n_tris)
    s = dict(coverage=coverage, n_views=len(poses), n_selected=len(chosen))
    for name, mask in (("target", everything), ("reachable", reachable), ("planned", planned)):
        s[name + "_q40"], s["n_" + name + "s" if name == "target" else "n_" + name] = weighted(mask, tt, w, n_tris)
    return scores, rec, s
