"""CPU: the view-planning contract (tests/plan_ref.py) on hand-built cases with known answers, the greedy selection against a brute
force over every order, and hfpf_check_plan_opts and the struct sizes through the built library (host code, no GPU).
Every triangle here has one sample, its centroid (max_subdivision = 1), there is no model (every in-box sample is a target), and the
camera sits at the origin and looks along +z, so zc of a sample is its z."""
import ctypes as C
import itertools
import os
import re

import numpy as np

import hfpf
import plan_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.002
BBOX = (-0.05, 0.05, -0.05, 0.05, 0.0, 0.1)
NO_ROWS, NO_OCC = np.zeros(0, hfpf.ROW_DTYPE), np.zeros((0, 3), np.int32)
CAM = np.eye(4)[:3]
K, W, H = (200.0, 200.0, 32.0, 32.0), 64, 64
BASE = dict(max_subdivision=1, spacing=0.02, z_range=(0.01, 1.0), tolerance=2.0 ** -8, max_views=8)


def tri(cx, cy, z, half=0.004, towards_camera=True):
    """A triangle in the plane z with its centroid at (cx, cy, z): its normal points to -z (at the camera) or, reversed, to +z."""
    v = np.array([[cx - half, cy - half, z], [cx + half, cy - half, z], [cx, cy + 2 * half, z]], np.float32)
    return v[[0, 2, 1]] if towards_camera else v


def mesh(*triangles):
    return np.concatenate(triangles), np.arange(3 * len(triangles), dtype=np.uint32).reshape(-1, 3)


def plan(triangles, poses=(CAM,), **kw):
    v, t = mesh(*triangles)
    return P.plan(NO_ROWS, NO_OCC, v, 12, t, np.eye(4)[:3], np.asarray(poses, np.float64), BBOX, RES, K, W, H, **dict(BASE, **kw))


def counts(scores, v=0):
    return tuple(int(scores[k][v]) for k in ("n_in_view", "n_facing", "n_visible"))


# ---- occlusion ------------------------------------------------------------------------------------------------------------------

def test_a_triangle_behind_another_is_occluded_until_the_front_one_moves_aside():
    back = tri(0.0, 0.0, 0.0625)
    scores, rec, s = plan([tri(0.0, 0.0, 0.04), back])
    assert s["n_targets"] == 2 and counts(scores) == (2, 2, 1)
    assert rec["n_targets"].tolist() == [1, 1] and rec["n_reachable"].tolist() == [1, 0] and rec["n_planned"].tolist() == [1, 0]
    assert s["n_selected"] == 1 and scores["rank"][0] == 0 and s["planned_q40"] == scores["gain_q40"][0] == scores["visible_q40"][0]
    assert s["n_reachable"] == 1 and s["target_q40"] == 2 * s["reachable_q40"], "two triangles of the same area"
    scores, rec, s = plan([tri(0.005, 0.0, 0.04), back])
    assert counts(scores) == (2, 2, 2) and rec["n_reachable"].tolist() == [1, 1] and s["planned_q40"] == s["target_q40"]


def test_tolerance_and_slope_at_the_exact_boundary():
    # depth32 of the two centroids: 2^-4 - 2^-8 and 2^-4, exactly; their difference is 2^-8
    pair = [tri(0.0, 0.0, 0.0625 - 2.0 ** -8), tri(0.0, 0.0, 0.0625)]
    assert counts(plan(pair, tolerance=2.0 ** -8)[0]) == (2, 2, 2), "difference == tolerance: visible"
    assert counts(plan(pair, tolerance=2.0 ** -8 - 2.0 ** -60)[0]) == (2, 2, 1)
    # slope * zc = 2^-5 * 2^-4 = 2^-9, exactly
    assert counts(plan(pair, tolerance=2.0 ** -9, slope=2.0 ** -5)[0]) == (2, 2, 2), "difference == tolerance + slope * zc: visible"
    assert counts(plan(pair, tolerance=2.0 ** -9 - 2.0 ** -60, slope=2.0 ** -5)[0]) == (2, 2, 1)
    assert counts(plan(pair, tolerance=2.0 ** -9, slope=0.0)[0]) == (2, 2, 1)


def test_an_occluder_between_occluder_near_and_z_near_still_blocks():
    pair = [tri(0.0, 0.0, 0.03), tri(0.0, 0.0, 0.0625)]
    kw = dict(z_range=(0.05, 1.0))
    assert counts(plan(pair, occluder_near=0.02, **kw)[0]) == (1, 1, 0), "the near triangle is out of range itself, and blocks"
    assert counts(plan(pair, occluder_near=0.04, **kw)[0]) == (1, 1, 1)
    assert counts(plan(pair, **kw)[0]) == (1, 1, 1), "occluder_near defaults to z_near"


# ---- the facing gate ------------------------------------------------------------------------------------------------------------

def _tilted():
    """One triangle off the axis, tilted about y: its normal is neither along the ray nor across it."""
    a = 0.7
    v = tri(0.0, 0.0, 0.0).astype(np.float64)
    Rm = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    return (v @ Rm.T + np.array([0.006, -0.004, 0.06])).astype(np.float32)


def _gate_terms(v):
    """c*c and NN * d2 of the triangle's one sample as the contract computes them."""
    A, B, Cc = v.astype(np.float64)
    ab, ac = B - A, Cc - A
    N = np.array([ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]])
    NN = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]
    S = (A + (1.0 / 3.0) * ab) + (1.0 / 3.0) * ac
    d = S.astype(np.float32).astype(np.float64)
    c = -((N[0] * d[0] + N[1] * d[1]) + N[2] * d[2])
    return c, NN, (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def test_min_cos_at_the_exact_boundary_gate_off_and_two_sided():
    v = _tilted()
    c, NN, d2 = _gate_terms(v)
    assert c > 0
    m = float(np.sqrt(c * c / (NN * d2)))
    passes = lambda x: c * c >= ((x * x) * NN) * d2
    while not passes(m):
        m = float(np.nextafter(m, 0.0))
    while passes(float(np.nextafter(m, 1.0))):
        m = float(np.nextafter(m, 1.0))
    assert 0.5 < m < 0.9, "the triangle is tilted by about 0.7 rad"
    assert counts(plan([v], min_cos=m)[0]) == (1, 1, 1), "the largest min_cos that passes"
    assert counts(plan([v], min_cos=float(np.nextafter(m, 1.0)))[0]) == (1, 0, 0), "one ulp above it"
    back = np.ascontiguousarray(v[[0, 2, 1]])  # the reversed winding: c < 0
    assert counts(plan([back], min_cos=0.0)[0]) == (1, 0, 0)
    assert counts(plan([back], min_cos=-1.0)[0]) == (1, 1, 1), "min_cos < 0 switches the gate off"
    assert counts(plan([back], min_cos=m, two_sided=True)[0]) == (1, 1, 1)
    assert counts(plan([back], min_cos=float(np.nextafter(m, 1.0)), two_sided=True)[0]) == (1, 0, 0)


# ---- the greedy selection ---------------------------------------------------------------------------------------------------------

def brute_force(vis, tri_of, w, max_views, min_gain):
    """The greedy sequence is the order whose (G, C, -view) marginal keys are lexicographically largest: every order is tried."""
    best_keys, best_order = None, None
    for order in itertools.permutations(range(len(vis))):
        left = np.ones(vis.shape[1], bool)
        keys = []
        for v in order:
            take = vis[v] & left
            keys.append((sum(w[k] for k in tri_of[take]), int(take.sum()), -v))
            left &= ~vis[v]
        if best_keys is None or keys > best_keys:
            best_keys, best_order = keys, order
    out = []
    for v, (G, Cn, _) in zip(best_order or (), best_keys or ()):
        if len(out) == max_views or G < max(1, min_gain):
            break
        out.append((v, G, Cn))
    return out


def _check_greedy(vis, tri_of, w, max_views=8, min_gain=0):
    got, left = P.greedy(vis, tri_of, w, len(w), max_views, min_gain)
    assert got == brute_force(vis, tri_of, w, max_views, min_gain)
    taken = np.zeros(vis.shape[1], bool)
    for v, _, _ in got:
        taken |= vis[v]
    assert (left == ~taken).all()
    return got


def test_greedy_against_every_order():
    rng = np.random.default_rng(0x91A7)
    for n_views in (1, 3, 5, 6):
        tri_of = rng.integers(0, 9, 150)
        w = [int(x) for x in rng.integers(0, 2 ** 50, 9)]
        vis = rng.random((n_views, 150)) < rng.uniform(0.1, 0.5, (n_views, 1))
        for max_views in (1, 2, 8):
            _check_greedy(vis, tri_of, w, max_views)
    # a duplicated view: the smaller index wins, the copy then gains nothing and the selection ends
    vis = np.array([[1, 1, 0, 0], [0, 0, 1, 0], [1, 1, 0, 0]], bool)
    got = _check_greedy(vis, np.zeros(4, np.int64), [5])
    assert [g[0] for g in got] == [0, 1], "view 2 duplicates view 0 and adds nothing: max_views is larger than the useful views"
    # equal G, different C: one target of weight 2 against two of weight 1
    vis = np.array([[1, 0, 0], [0, 1, 1]], bool)
    got = _check_greedy(vis, np.array([0, 1, 1]), [2, 1])
    assert got == [(1, 2, 2), (0, 2, 1)]
    # min_gain stops early; G = 0 never selects
    vis = np.array([[1, 1, 1, 0, 0, 0], [0, 0, 0, 1, 1, 0], [0, 0, 0, 0, 0, 1]], bool)
    assert [g[0] for g in _check_greedy(vis, np.zeros(6, np.int64), [4], min_gain=8)] == [0, 1]
    assert [g[0] for g in _check_greedy(vis, np.zeros(6, np.int64), [4], min_gain=9)] == [0]
    assert _check_greedy(vis, np.zeros(6, np.int64), [0]) == [], "weight 0 everywhere"


def test_a_duplicated_pose_loses_to_the_smaller_index():
    aside = np.hstack([np.eye(3), [[0.004], [0.0], [0.0]]])  # sees the same two triangles from the side: both visible
    scores, rec, s = plan([tri(0.0, 0.0, 0.04), tri(0.0, 0.0, 0.0625)], poses=(CAM, aside, aside))
    assert counts(scores, 0) == (2, 2, 1) and counts(scores, 1) == counts(scores, 2) == (2, 2, 2)
    assert scores["rank"].tolist() == [-1, 0, -1] and s["n_selected"] == 1 and s["n_planned"] == s["n_reachable"] == 2
    assert scores["gain_q40"][2] == 0 and scores["gain_samples"].tolist() == [0, 2, 0] and scores["visible_q40"][1] == scores["visible_q40"][2]


# ---- HUGE triangles ---------------------------------------------------------------------------------------------------------------

def test_a_huge_triangle_occludes_but_weighs_nothing():
    huge = np.array([[-8192, -8192, 0.04], [0, 16384, 0.04], [8192, -8192, 0.04]], np.float32)  # its centroid: (0, 0, 0.04), in the box
    scores, rec, s = plan([huge, tri(0.0, 0.0, 0.0625)])
    assert rec["flags"].tolist() == [1 | 2 | 4, 1] and s["coverage"]["n_tris_huge"] == 1
    assert s["n_targets"] == 2 and counts(scores) == (2, 2, 1), "the huge triangle's sample is seen, the one behind it is not"
    assert scores["visible_q40"][0] == 0 and s["reachable_q40"] == 0 and s["n_reachable"] == 1
    assert s["target_q40"] > 0 and s["n_selected"] == 0 and scores["rank"][0] == -1, "G = 0: nothing is selected"


def test_no_views_and_no_triangles():
    scores, rec, s = plan([tri(0.0, 0.0, 0.05)], poses=np.zeros((0, 12)))
    assert len(scores) == 0 and s["n_targets"] == 1 and s["n_reachable"] == s["n_planned"] == s["n_selected"] == 0 and s["coverage"]["n_samples"] == 1
    scores, rec, s = P.plan(NO_ROWS, NO_OCC, np.zeros((0, 3), np.float32), 12, np.zeros((0, 3), np.uint32), CAM, CAM[None], BBOX, RES, K, W, H, **BASE)
    assert len(rec) == 0 and scores["rank"].tolist() == [-1] and not any(s[k] for k in P.SUMMARY_KEYS if k != "n_views")


# ---- the library's host code ------------------------------------------------------------------------------------------------------

def test_check_plan_opts_rejects_every_bad_field():
    def opts(**fields):
        o = hfpf.plan_opts(K, W, H, spacing=0.004, z_range=(0.05, 2.0), occluder_near=0.02, min_cos=0.2, tolerance=0.004, slope=0.01)
        for k, val in fields.items():
            target = o
            *path, leaf = k.split("__")
            for part in path:
                target = getattr(target, part)
            setattr(target, leaf, val)
        return o

    assert hfpf.check_plan_opts(opts()) == 0
    assert hfpf.check_plan_opts(opts(flags=3, min_cos=-1.0, tolerance=1.0, slope=0.0, max_views=256, occluder_near=0.05)) == 0
    assert hfpf.check_plan_opts(opts(min_cos=1.0, slope=1.0, max_views=1, view__flags=3)) == 0
    assert hfpf.check_plan_opts(None) == -2
    nan, inf = float("nan"), float("inf")
    bad = [dict(struct_size=200), dict(flags=4), dict(reserved0=1), dict(reserved=1),
           # everything hfpf_check_cover_opts rejects
           dict(cover__struct_size=48), dict(cover__flags=2), dict(cover__reserved=7), dict(cover__radius=0), dict(cover__radius=5),
           dict(cover__max_subdivision=0), dict(cover__max_subdivision=65), dict(cover__min_count=nan), dict(cover__max_distance=0.0),
           dict(cover__max_distance=1.5), dict(cover__max_distance=inf), dict(cover__spacing=0.0), dict(cover__spacing=inf),
           dict(cover__min_normal_dot=-2.5), dict(cover__min_normal_dot=1.5), dict(cover__min_normal_dot=nan),
           # everything hfpf_render rejects in the view
           dict(view__struct_size=80), dict(view__flags=4), dict(view__reserved=1), dict(view__width=0), dict(view__height=0),
           dict(view__width=1 << 16, view__height=(1 << 15) + 1), dict(view__fx=0.0), dict(view__fy=-1.0), dict(view__fx=inf), dict(view__cx=nan),
           dict(view__cy=inf), dict(view__z_near=0.0, occluder_near=0.0), dict(view__z_near=3.0), dict(view__z_far=inf), dict(view__min_count=nan),
           dict(view__splat_radius=-2), dict(view__splat_radius=16), dict(view__max_splat_radius=-1), dict(view__max_splat_radius=16),
           # the plan's own fields
           dict(occluder_near=0.0), dict(occluder_near=-0.01), dict(occluder_near=0.0500001), dict(occluder_near=nan), dict(occluder_near=inf),
           dict(min_cos=-1.5), dict(min_cos=1.5), dict(min_cos=nan), dict(tolerance=0.0), dict(tolerance=1.5), dict(tolerance=nan), dict(tolerance=inf),
           dict(slope=-0.1), dict(slope=1.5), dict(slope=nan), dict(max_views=0), dict(max_views=257)]
    for f in bad:
        assert hfpf.check_plan_opts(opts(**f)) == -2, f


def test_struct_sizes_and_mirrors():
    txt = open(os.path.join(ROOT, "include", "hfpf.h")).read()
    for struct, size, mirror in (("hfpf_plan_opts", 208, C.sizeof(hfpf.PlanOpts)), ("hfpf_view_score", 40, hfpf.VIEW_SCORE_DTYPE.itemsize),
                                 ("hfpf_tri_plan", 16, hfpf.TRI_PLAN_DTYPE.itemsize), ("hfpf_plan_summary", 152, C.sizeof(hfpf.PlanSummary))):
        assert int(re.search(r"static_assert\(sizeof\(%s\) == (\d+)" % struct, txt).group(1)) == size == mirror
    assert hfpf.VIEW_SCORE_DTYPE == P.VIEW_SCORE_DTYPE and hfpf.TRI_PLAN_DTYPE == P.TRI_PLAN_DTYPE
    assert (hfpf.PLAN_TWO_SIDED, hfpf.PLAN_MODEL_OCCLUDES) == (P.TWO_SIDED, P.MODEL_OCCLUDES)
    assert tuple(k for k, _ in hfpf.PlanSummary._fields_[1:]) == P.SUMMARY_KEYS
    assert hfpf.PlanOpts.cover.offset == 8 and hfpf.PlanOpts.view.offset == 64 and hfpf.PlanOpts.occluder_near.offset == 152
    assert int(re.search(r"#define\s+HFPF_ABI_VERSION\s+(\d+)", txt).group(1)) == 6
    for sym in ("hfpf_check_plan_opts", "hfpf_plan_views", "hfpf_plan_views_device", "hfpf_free_plan"):
        assert sym in hfpf.EXPORTS and getattr(hfpf.lib(), sym)
