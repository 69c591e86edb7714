"""GPU: planning the next views against a reference mesh (hfpf_plan_views, hfpf_plan_views_device).  The call is defined on the rows
hfpf_extract returns and the cells hfpf_get_occupied lists, so every score, every triangle record and every summary is compared byte for
byte with tests/plan_ref.py run on those: the contract is exact, no tolerance is involved.  The session is the one of the cover tests
(three 160 x 120 synthetic depth frames at 2 mm); the reference mesh is the scene's sphere and box, cut into some 90,000 samples."""
import ctypes as C

import numpy as np
import pytest

import plan_support as S
from gpu_support import IDENT, RES, counters, grid, run, uploaded
from scenes import DepthScene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def session(hfpf_mod, synth_mod):
    sc = DepthScene(3, 160, 120, clean_every=2)
    g = grid(hfpf_mod)
    run(g, sc)
    rows = g.extract().copy()
    occ = g.occupied().copy()
    verts, tris = S.sphere_and_box()
    print("session: %d rows; reference mesh %d vertices / %d triangles" % (len(rows), len(verts), len(tris)))
    assert len(rows) > 1000
    yield sc, g, rows, occ, verts, tris
    g.close()


@pytest.fixture(scope="module")
def main_case(session):
    """The main case's reference and the host form's answer, computed once."""
    sc, g, rows, occ, verts, tris = session
    poses = S.main_poses()
    ref = S.reference(g, rows, occ, verts, 12, tris, IDENT, poses, **S.VIEW, **S.MAIN)
    got = g.plan_views(verts, tris, poses, IDENT, **S.VIEW, **S.MAIN)
    return poses, ref, got


def _both(g, rows, occ, verts, tris, poses, what, pose=IDENT, view=S.VIEW, **kw):
    """The host form against the reference; returns it."""
    got = g.plan_views(verts, tris, poses, pose, **view, **kw)
    stride = verts.dtype.itemsize if verts.dtype.names else 12
    S.same_plan(got, S.reference(g, rows, occ, verts, stride, tris, pose, poses, **view, **kw), what)
    S.plan_sums(*got)
    return got


# ---- 1. the main case -------------------------------------------------------------------------------------------------------------

def test_main_case_against_the_reference(hfpf_mod, session, main_case):
    sc, g, rows, occ, verts, tris = session
    poses, ref, got = main_case
    scores, rec, s = got
    print("main: %d samples, %d targets, %d reachable, %d planned, %d selected" % (s["coverage"]["n_samples"], s["n_targets"], s["n_reachable"],
                                                                                 s["n_planned"], s["n_selected"]))
    print(scores)
    S.same_plan(got, ref, "main case, host form")
    S.plan_sums(*got)
    assert s["coverage"]["n_tris_invalid"] == 96 and len(tris) == 2316, "the polar triangles are invalid"
    assert s["n_targets"] > 0
    assert ((scores["n_facing"] > scores["n_visible"]) & (scores["n_visible"] > 0)).any(), "some view has facing targets behind an occluder"
    assert s["n_selected"] >= 3
    assert scores["rank"][12] == -1 and all(scores[k][12] == scores[k][3] for k in ("n_in_view", "n_facing", "n_visible", "visible_q40")), \
        "view 12 is view 3 again, and never selected"
    assert 0 < s["n_planned"] <= s["n_reachable"] < s["n_targets"]
    assert s["planned_q40"] == sum(int(x) for x in scores["gain_q40"])
    cov, cs = g.cover_mesh(verts, tris, IDENT, **{k: S.MAIN[k] for k in ("radius", "max_distance", "spacing")})
    assert s["coverage"] == cs, "the embedded coverage summary is hfpf_cover_mesh's own"
    assert rec["flags"].tobytes() == cov["flags"].tobytes() and (rec["n_targets"] == cov["n_in_bbox"] - cov["n_covered"]).all()


def test_a_duplicated_view_loses_to_the_smaller_index(hfpf_mod, session, main_case):
    sc, g, rows, occ, verts, tris = session
    poses, ref, got = main_case
    best = int(np.flatnonzero(got[0]["rank"] == 0)[0])
    twice = np.stack([poses[best], poses[best]])
    scores, rec, s = _both(g, rows, occ, verts, tris, twice, "one pose twice", **S.MAIN)
    assert scores["rank"].tolist() == [0, -1] and s["n_selected"] == 1 and scores["gain_q40"][0] == got[0]["gain_q40"][best]


def test_device_form_gives_the_same_bytes(hfpf_mod, session, main_case):
    sc, g, rows, occ, verts, tris = session
    poses, ref, got = main_case
    with uploaded(g, verts, tris) as (dv, dt):
        dev = S.plan_device(g, hfpf_mod, dv, len(verts), 12, dt, len(tris), poses, IDENT, **S.VIEW, **S.MAIN)
        S.same_plan(dev, ref, "main case, device form")
        assert dev[0].tobytes() == got[0].tobytes() and dev[1].tobytes() == got[1].tobytes() and dev[2] == got[2]
        scores, ptr, s = g.plan_views(dv, dt, poses, IDENT, device=True, tri_plan=False, n_verts=len(verts), vertex_stride=12, n_tris=len(tris), **S.VIEW, **S.MAIN)
        assert ptr == 0 and scores.tobytes() == got[0].tobytes() and s == got[2], "without the triangle records"
    scores, rec, s = g.plan_views(verts, tris, poses, IDENT, tri_plan=False, **S.VIEW, **S.MAIN)
    assert rec is None and scores.tobytes() == got[0].tobytes() and s == got[2]


@pytest.mark.parametrize("chunk", ["1", "5"])
def test_forced_chunks_give_the_bytes_of_the_default(hfpf_mod, session, main_case, monkeypatch, chunk):
    sc, g, rows, occ, verts, tris = session
    poses, ref, got = main_case
    monkeypatch.setenv("HFPF_PLAN_CHUNK", chunk)
    again = g.plan_views(verts, tris, poses, IDENT, **S.VIEW, **S.MAIN)
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes() and again[2] == got[2]


# ---- 2. numbers of views ------------------------------------------------------------------------------------------------------------

def test_seventy_views_cross_a_chunk_of_64(hfpf_mod, session):
    sc, g, rows, occ, verts, tris = session
    poses = np.concatenate([S.ring(35, 0.42), S.ring(35, 0.5, lift=0.15)])
    kw = dict(S.MAIN, spacing=4 * RES, splat_radius=0, max_views=70)
    scores, rec, s = _both(g, rows, occ, verts, tris, poses, "70 views at 32 x 24", view=S.SMALL_VIEW, **kw)
    print("70 views: %d targets, %d selected" % (s["n_targets"], s["n_selected"]))
    assert s["n_views"] == 70 and (scores["n_visible"][64:] > 0).any() and s["n_selected"] >= 3


def test_one_view_no_view_and_views_that_look_away(hfpf_mod, session):
    sc, g, rows, occ, verts, tris = session
    scores, rec, s = _both(g, rows, occ, verts, tris, S.ring(12)[5:6], "one view", **S.MAIN)
    assert s["n_selected"] == 1 and scores["rank"][0] == 0 and s["n_planned"] == s["n_reachable"] == scores["n_visible"][0] > 0
    scores, rec, s = _both(g, rows, occ, verts, tris, np.zeros((0, 12)), "no view", **S.MAIN)
    assert len(scores) == 0 and s["n_targets"] > 0 and s["n_selected"] == s["n_reachable"] == s["n_planned"] == 0 and s["coverage"]["n_samples"] > 0
    away = np.stack([S.look_at(p[:, 3], 2 * p[:, 3] - np.array(S.LOOK_AT)) for p in S.ring(5)])  # from the ring, outwards
    scores, rec, s = _both(g, rows, occ, verts, tris, away, "every view looks away", **S.MAIN)
    assert s["n_targets"] > 0 and s["n_selected"] == 0 and (scores["rank"] == -1).all()
    assert all(int(scores[k].sum()) == 0 for k in ("n_in_view", "n_facing", "n_visible", "visible_q40", "gain_q40", "gain_samples"))


# ---- 3. numbers of targets: the tail of the last ballot word ------------------------------------------------------------------------

@pytest.mark.parametrize("n", [50, 63, 64, 65, 129])
def test_target_counts_around_a_ballot_word(hfpf_mod, session, n):
    sc, g, rows, occ, verts, tris = session
    cv, ct = S.chips(n)
    kw = dict(S.MAIN, max_subdivision=1, spacing=0.02, splat_radius=0)
    scores, rec, s = _both(g, rows, occ, cv, ct, S.ring(4, 0.3, target=(0.0, 0.0, 0.17)), "%d chips" % n, **kw)
    assert s["n_targets"] == n == s["coverage"]["n_samples"] and s["n_reachable"] > 0 and (rec["n_targets"] == 1).all()


def test_own_mesh_has_no_targets(hfpf_mod, session):
    sc, g, rows, occ, verts, tris = session
    ov, ot = g.extract_mesh()
    kw = dict(S.MAIN, max_distance=0.05, spacing=RES)
    scores, rec, s = _both(g, rows, occ, ov, ot[:3000], S.main_poses(), "own mesh, generous max_distance", **kw)
    assert s["n_targets"] == 0 and s["coverage"]["n_covered"] == s["coverage"]["n_in_bbox"] > 0 and s["n_selected"] == 0
    assert int(rec["n_targets"].sum()) == 0


def test_mixed_soup_with_invalid_triangles(hfpf_mod, session):
    sc, g, rows, occ, verts, tris = session
    a, b = 0.02, -0.015
    Rm = (np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]]) @
          np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]]))
    pose = np.hstack([Rm, [[0.003], [-0.002], [0.004]]])
    sv, st = S.soup(rows, pose)
    kw = dict(S.MAIN, spacing=RES, max_subdivision=24, two_sided=True)
    scores, rec, s = _both(g, rows, occ, sv, st, S.main_poses(), "soup", pose=pose, **kw)
    print("soup: %d samples, %d targets, %d reachable" % (s["coverage"]["n_samples"], s["n_targets"], s["n_reachable"]))
    assert s["coverage"]["n_tris_invalid"] == 78 and not rec[(rec["flags"] & 1) == 0].view(np.uint8).any(), "an invalid triangle's record is all zero"
    assert 0 < s["n_reachable"] < s["n_targets"]


# ---- 4. the model as an occluder, the splat ---------------------------------------------------------------------------------------------

def test_model_occludes_from_behind_the_back_plane(hfpf_mod, session):
    sc, g, rows, occ, verts, tris = session
    # z > 0.56, looking along -z: two straight behind the shapes, two from the sides, where the plane was not in the sphere's shadow
    behind = np.stack([S.look_at((0.05, 0.0, 0.95), (0.05, 0.0, 0.45)), S.look_at((-0.05, 0.03, 0.9), (0.0, 0.0, 0.45)),
                       S.look_at((0.6, 0.0, 0.75), (0.05, 0.0, 0.45)), S.look_at((-0.5, 0.05, 0.8), (-0.1, 0.0, 0.5))])
    kw = dict(S.MAIN, splat_radius=-1, max_splat_radius=4)
    free = _both(g, rows, occ, verts, tris, behind, "behind the back plane", **kw)
    model = _both(g, rows, occ, verts, tris, behind, "behind the back plane, the model occludes", model_occludes=True, **kw)
    culled = _both(g, rows, occ, verts, tris, behind, "behind the back plane, the model's front faces occlude", model_occludes=True, cull_backfaces=True, **kw)
    counted = _both(g, rows, occ, verts, tris, behind, "behind the back plane, rows of count >= 3 occlude", model_occludes=True, view_min_count=3.0, **kw)
    n = [int(x[0]["n_visible"].sum()) for x in (free, model, culled, counted)]
    print("visible from behind: %d without the model, %d with it, %d with its front faces only, %d with rows of count >= 3" % tuple(n))
    assert n[0] > n[1] >= 0 and n[0] > 0, "the back plane's rows hide the sphere's back"
    assert n[2] >= n[1], "rows that face away from the camera are culled: they hide no more"
    assert (free[0]["n_facing"] == model[0]["n_facing"]).all(), "the occluders do not change who faces the camera"


@pytest.mark.parametrize("splat_radius", [0, 3, -1])
def test_fixed_and_auto_splat_radius(hfpf_mod, session, splat_radius):
    sc, g, rows, occ, verts, tris = session
    kw = dict(S.MAIN, splat_radius=splat_radius, max_splat_radius=2, spacing=6 * RES, tolerance=RES, slope=0.01)
    scores, rec, s = _both(g, rows, occ, verts, tris, S.ring(4, 0.25), "splat_radius %d" % splat_radius, **kw)  # near: the auto radius reaches 1 and 2
    assert s["n_reachable"] > 0


# ---- 5. handles without a model ---------------------------------------------------------------------------------------------------------

def test_fresh_handle_and_frames_without_a_clean_pass(hfpf_mod, session):
    sc, g, rows, occ, verts, tris = session
    kw = dict(S.MAIN, spacing=4 * RES)
    with grid(hfpf_mod) as fresh:
        no_rows, no_occ = np.zeros(0, hfpf_mod.ROW_DTYPE), np.zeros((0, 3), np.int32)
        ref = S.reference(fresh, no_rows, no_occ, verts, 12, tris, IDENT, S.ring(6), **S.VIEW, **kw)
        got = fresh.plan_views(verts, tris, S.ring(6), IDENT, **S.VIEW, **kw)
        S.same_plan(got, ref, "a fresh handle")
        assert got[2]["n_targets"] == got[2]["coverage"]["n_in_bbox"] > 0, "every in-box sample is a target"
        S.same_plan(fresh.plan_views(verts, tris, S.ring(6), IDENT, model_occludes=True, **S.VIEW, **kw), ref, "a fresh handle has no rows to occlude")
        sc.integrate(fresh, 0)  # points, but no clean pass yet
        S.same_plan(fresh.plan_views(verts, tris, S.ring(6), IDENT, **S.VIEW, **kw), ref, "frames but no clean pass")


def test_both_forms_return_the_documented_empties(hfpf_mod, session):
    """No triangles (nothing to plan: every rank -1, a summary that holds n_views alone, no records), no views, and a handle without
    rows: the same bytes out of either form."""
    sc, g, rows, occ, verts, tris = session
    kw = dict(S.MAIN, spacing=4 * RES)
    none = np.zeros((0, 12))
    with uploaded(g, verts, tris) as (dv, dt):
        host = g.plan_views(verts, np.zeros((0, 3), np.uint32), S.ring(3), IDENT, **S.VIEW, **kw)
        dev = g.plan_views(dv, 0, S.ring(3), IDENT, device=True, n_verts=len(verts), vertex_stride=12, n_tris=0, **S.VIEW, **kw)
        assert len(host[1]) == 0 and dev[1] == 0 and host[0].tobytes() == dev[0].tobytes() and host[2] == dev[2]
        assert (host[0]["rank"] == -1).all() and not any(host[0][k].any() for k in host[0].dtype.names if k != "rank")
        s = host[2]
        assert s["n_views"] == 3 and not any(s[k] for k in s if k not in ("n_views", "coverage")) and not any(s["coverage"].values())
        host = g.plan_views(verts, tris, none, IDENT, **S.VIEW, **kw)
        dev = S.plan_device(g, hfpf_mod, dv, len(verts), 12, dt, len(tris), none, IDENT, **S.VIEW, **kw)
        assert len(dev[0]) == 0 and dev[1].tobytes() == host[1].tobytes() and dev[2] == host[2] and host[2]["n_targets"] > 0 == host[2]["n_selected"]
    with grid(hfpf_mod) as fresh:
        host = fresh.plan_views(verts, tris, S.ring(6), IDENT, **S.VIEW, **kw)
        with uploaded(fresh, verts, tris) as (dv, dt):
            dev = S.plan_device(fresh, hfpf_mod, dv, len(verts), 12, dt, len(tris), S.ring(6), IDENT, **S.VIEW, **kw)
        assert dev[0].tobytes() == host[0].tobytes() and dev[1].tobytes() == host[1].tobytes() and dev[2] == host[2]
        assert host[2]["n_targets"] == host[2]["coverage"]["n_in_bbox"] > 0, "every in-box sample is a target"


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------

def test_every_bad_arg_writes_nothing_and_leaves_the_handle_usable(hfpf_mod, session):
    H = hfpf_mod
    sc, g, rows, occ, verts, tris = session
    L, h = H.lib(), g._h
    v, t = S.chips(3)
    pose = np.ascontiguousarray(IDENT, np.float64).reshape(12)
    poses = np.ascontiguousarray(S.ring(2), np.float64).reshape(-1)
    out = dict(sc=np.frombuffer(b"\xab" * 80, H.VIEW_SCORE_DTYPE).copy(), t=C.c_void_p(0xAB), s=H.PlanSummary())
    C.memset(C.byref(out["s"]), 0xAB, C.sizeof(out["s"]))
    untouched = (out["sc"].tobytes(), bytes(out["s"]))
    dv, dt = g.device_alloc(64), g.device_alloc(64)
    kw = dict(S.MAIN, max_subdivision=1, spacing=0.02)

    def call(o=None, verts=v.ctypes.data, n_verts=9, stride=12, tris=t.ctypes.data, n_tris=3, pose=pose.ctypes.data, poses=poses.ctypes.data, n_views=2,
             scores=True, plan=True, s=True, device=False):
        o = o if o is not None else H.plan_opts(**S.VIEW, **kw)
        fn = L.hfpf_plan_views_device if device else L.hfpf_plan_views
        return fn(h, C.byref(o), verts, n_verts, stride, tris, n_tris, pose, poses, n_views, out["sc"].ctypes.data if scores else None,
                  C.byref(out["t"]) if plan else None, C.byref(out["s"]) if s else None)

    def opts(**fields):
        o = H.plan_opts(**S.VIEW, **kw)
        for k, val in fields.items():
            target = o
            *path, leaf = k.split("__")
            for part in path:
                target = getattr(target, part)
            setattr(target, leaf, val)
        return o

    bad_pose, bad_poses = pose.copy(), poses.copy()
    bad_pose[7], bad_poses[17] = np.inf, np.nan
    many = np.tile(pose, 4097)
    try:
        faults = [dict(o=opts(struct_size=200)), dict(o=opts(flags=4)), dict(o=opts(reserved=1)), dict(o=opts(reserved0=1)),
                  dict(o=opts(cover__radius=0)), dict(o=opts(cover__spacing=0.0)), dict(o=opts(cover__struct_size=48)),
                  dict(o=opts(view__width=0)), dict(o=opts(view__fx=0.0)), dict(o=opts(view__splat_radius=16)), dict(o=opts(view__flags=4)),
                  dict(o=opts(occluder_near=0.0)), dict(o=opts(occluder_near=0.06)), dict(o=opts(occluder_near=float("nan"))),
                  dict(o=opts(min_cos=1.5)), dict(o=opts(min_cos=float("nan"))), dict(o=opts(tolerance=0.0)), dict(o=opts(tolerance=1.5)),
                  dict(o=opts(slope=-0.5)), dict(o=opts(slope=1.5)), dict(o=opts(max_views=0)), dict(o=opts(max_views=257)),
                  dict(poses=many.ctypes.data, n_views=4097), dict(poses=None), dict(poses=bad_poses.ctypes.data),
                  dict(pose=None), dict(pose=bad_pose.ctypes.data), dict(stride=8), dict(stride=14), dict(verts=None), dict(tris=None),
                  dict(n_verts=2 ** 32 - 1), dict(n_tris=2 ** 32 - 1), dict(scores=False), dict(s=False),
                  dict(device=True, verts=dv + 2, tris=dt), dict(device=True, verts=dv, tris=dt + 1)]
        for f in faults + [dict(dict(device=True, verts=dv, tris=dt), **f) for f in faults if "device" not in f]:  # each through both forms
            assert call(**f) == -2, f
            assert out["t"].value == 0xAB and (out["sc"].tobytes(), bytes(out["s"])) == untouched, "a rejected call writes nothing: %r" % (f,)
        assert call(poses=None, n_views=0) == 0 and out["s"].n_targets == 3 and out["s"].n_views == 0, "no views need no poses"
        L.hfpf_free_plan(out["t"])
        out["t"] = C.c_void_p()
        assert call(plan=False) == 0 and out["t"].value is None and out["s"].n_views == 2  # the handle is still usable, the records are optional
        assert call() == 0 and out["t"].value and out["s"].n_targets == 3
        L.hfpf_free_plan(out["t"])
    finally:
        g.device_free(dv), g.device_free(dt)
    assert g.extract().tobytes() == rows.tobytes()


def test_capacity_refusal_at_2_to_the_35_pairs(hfpf_mod):
    # 2049 triangles of 4096 samples in an empty box: 2049 * 2^12 targets x 2^12 views = 2^35 + 2^24 pairs.  The refusal follows the
    # count of the targets and precedes the bitsets: nothing of that size is allocated.
    n = 2049
    tri = np.array([[-0.2, -0.2, 0.0], [0.2, -0.2, 0.0], [0.0, 0.2, 0.0]])
    verts = (tri[None] + np.array([0.0, 0.0, 0.3]) + np.arange(n)[:, None, None] * np.array([0.0, 0.0, 1e-4])).reshape(-1, 3).astype(np.float32)
    tris = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    poses = np.tile(S.ring(1), (4096, 1, 1))
    kw = dict(S.MAIN, spacing=RES)
    with grid(hfpf_mod) as fresh:
        with pytest.raises(hfpf_mod.HfpfError) as e:
            fresh.plan_views(verts, tris, poses, IDENT, tri_plan=False, **S.SMALL_VIEW, **kw)
        assert e.value.code == -3 and str(n * 4096) in str(e.value) and "4096 views" in str(e.value), str(e.value)
        # the device form refuses alike, and neither the scores nor the summary nor the records' pointer is written
        o, pose, flat = hfpf_mod.plan_opts(**S.SMALL_VIEW, **kw), np.ascontiguousarray(IDENT, np.float64).reshape(12), np.ascontiguousarray(poses).reshape(-1)
        out_sc, out_t, out_s = np.full(4096 * hfpf_mod.VIEW_SCORE_DTYPE.itemsize, 0xAB, np.uint8), C.c_void_p(0xAB), hfpf_mod.PlanSummary()
        C.memset(C.byref(out_s), 0xAB, C.sizeof(out_s))
        with uploaded(fresh, verts, tris) as (dv, dt):
            rc = hfpf_mod.lib().hfpf_plan_views_device(fresh._h, C.byref(o), dv, len(verts), 12, dt, n, pose.ctypes.data, flat.ctypes.data, 4096,
                                                       out_sc.ctypes.data, C.byref(out_t), C.byref(out_s))
        msg = hfpf_mod.lib().hfpf_last_error(fresh._h).decode()
        assert rc == -3 and str(n * 4096) in msg and "4096 views" in msg, msg
        assert (out_sc == 0xAB).all() and out_t.value == 0xAB and bytes(out_s) == b"\xab" * C.sizeof(out_s), "a refused call writes nothing"
        scores, rec, s = fresh.plan_views(verts[:9], tris[:3], poses[:2], IDENT, **S.SMALL_VIEW, **kw)  # the handle stays usable
        assert s["n_targets"] == 3 * 4096 and s["n_views"] == 2


# ---- 7. a plan is read-only, and a restored handle answers the same -------------------------------------------------------------------------

def test_plan_is_read_only_and_survives_a_restore(hfpf_mod, session, main_case):
    sc, g, rows, occ, verts, tris = session
    poses, ref, got = main_case
    before = (counters(g), g.extract().tobytes(), g.occupied().tobytes())
    kw = dict(S.MAIN, model_occludes=True)
    with_model = g.plan_views(verts, tris, poses, IDENT, **S.VIEW, **kw)
    assert (counters(g), g.extract().tobytes(), g.occupied().tobytes()) == before
    blob = g.snapshot()
    with grid(hfpf_mod) as g2:
        g2.restore(blob)
        for have, want, what in ((g2.plan_views(verts, tris, poses, IDENT, **S.VIEW, **S.MAIN), got, "main case"),
                                 (g2.plan_views(verts, tris, poses, IDENT, **S.VIEW, **kw), with_model, "the model occludes")):
            assert have[0].tobytes() == want[0].tobytes() and have[1].tobytes() == want[1].tobytes() and have[2] == want[2], "%s on the restored handle" % what
