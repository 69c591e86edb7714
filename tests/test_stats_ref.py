"""CPU: the engine's statistics contract (csrc/stats.hpp: integer sums of fixed-point contributions; csrc/kernels.hpp record_row:
a fixed f64 expression of those sums) stated twice without the engine -- the oracle's exact_moments side channel (C++) and
tests/stats_ref.py (numpy) -- and held against each other byte for byte, against the reference's Welford recurrence within the
tolerances of scenes.compare_rows, and against exact rational arithmetic on hand cases.  tests/test_gpu_exact_rows.py then holds
the kernels against the same rows."""
import math
from fractions import Fraction

import numpy as np
import pytest

import scenes
import stats_ref as R

NON_DEFAULT = dict(K=5, cylinder_radius=0.003, ball_radius=0.03)


CASE_NAMES = ("5mm", "1mm", "colour", "shifted_cov", "non_default", "dense")


def _case(name):
    """(scene, oracle config) of a named case."""
    small = dict(n_frames=5, W=160, H=120, resolution=0.001, fx=615.0, clean_every=2)
    if name == "5mm":
        return scenes.Scene(6, 160, 120, 0.005, clean_every=3), {}
    if name == "1mm":
        return scenes.Scene(6, 160, 120, 0.001, fx=615.0, clean_every=3), {}
    if name == "dense":
        return scenes.dense_scene()
    return scenes.Scene(**small), {"colour": dict(fuse_color=True), "shifted_cov": dict(pcl_shifted_cov=True), "non_default": NON_DEFAULT}[name]


_cache = {}


def _run(oracle_mod, synth_mod, name):
    """(Welford rows, exact rows, moment records, scales) of a case, computed once and never modified."""
    if name not in _cache:
        sc, cfg = _case(name)
        og = oracle_mod.OracleGrid(resolution=sc.resolution, bbox=sc.bbox, exact_moments=True, **cfg)
        ref = scenes.run(og, sc, "capture", color=bool(cfg.get("fuse_color")))
        out = (ref, og.extract_exact(), og.moments(), og.scales())
        og.close()
        for a in out:
            a.setflags(write=False)
        _cache[name] = out
    return _cache[name]


def _restated(name, ref, mom):
    sc, cfg = _case(name)
    kw = {k: cfg[k] for k in ("K", "ball_radius", "cylinder_radius") if k in cfg}
    nrm = np.stack([ref["nx"], ref["ny"], ref["nz"]], axis=1)
    return R.rows_from_moments(mom, nrm, sc.bbox[0::2], sc.resolution, color=bool(cfg.get("fuse_color")), **kw)


def _pre_clamp_variance_sign(w, sc4):
    """Sign of E[u^2] - E[u]^2 of one record in exact integers (the scales are powers of two)."""
    n, s1, s2 = int(w[0]), int(w[1]), int(w[2])
    fs, fss = int(sc4[0]), int(sc4[1])
    v = s2 * fs * fs * n - s1 * s1 * fss
    return (v > 0) - (v < 0)


# ---- the two restatements agree byte for byte; the exact rows mean what the reference's rows mean ----

@pytest.mark.parametrize("name", ["5mm", "1mm", "colour", "shifted_cov", "non_default"])
def test_extract_exact_equals_the_numpy_restatement_of_its_moments(oracle_mod, synth_mod, name):
    ref, exact, mom, sc4 = _run(oracle_mod, synth_mod, name)
    sc, cfg = _case(name)
    assert len(ref) > 1000
    assert np.array_equal(sc4, R.scales(cfg.get("K", 3), sc.resolution, cfg.get("ball_radius", 0.015), cfg.get("cylinder_radius", 0.001)))
    for f in ("ix", "iy", "iz"):
        assert np.array_equal(mom[f], ref[f]) and np.array_equal(exact[f], ref[f]), f
    for f in ("count", "nx", "ny", "nz", "rgb"):  # integer columns and normals are extract()'s
        assert np.array_equal(exact[f].view(np.uint32), ref[f].view(np.uint32)), f
    assert np.array_equal(mom["m"][:, 0], ref["count"].astype(np.int64)), "word 0 is not the count"
    if cfg.get("fuse_color"):
        assert (mom["m"][:, 5:] > 0).any() and len(np.unique(exact["rgb"])) > 1000
    else:
        assert not mom["m"][:, 5:].any()
    mine = _restated(name, ref, mom)
    bad = {f: int((mine[f].view(np.uint32) != exact[f].view(np.uint32)).sum()) for f in mine.dtype.names}
    assert mine.tobytes() == exact.tobytes(), "rows differing per column: %r" % {f: n for f, n in bad.items() if n}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_exact_rows_pass_compare_rows_against_the_recurrence(oracle_mod, synth_mod, name):
    """The exact side channel describes the same voxels as the reference's f32 Welford recurrence, within the tolerances the
    project already justifies for the engine."""
    ref, exact, mom, sc4 = _run(oracle_mod, synth_mod, name)
    scenes.compare_rows(ref, exact)
    scenes.compare_rows_exact(exact, exact, cylinder_radius=_case(name)[1].get("cylinder_radius", 0.001))  # and itself, trivially


def test_the_scenes_hold_the_hard_voxels(oracle_mod, synth_mod):
    """What the byte comparisons above (and the GPU ones on the same scenes) cover: one-member voxels, voxels without members,
    negative sums of u, variances that are negative before the clamp, words beyond 2^32."""
    ref, exact, mom, sc4 = _run(oracle_mod, synth_mod, "5mm")
    m = mom["m"]
    assert (m[:, 0] == 1).sum() > 100 and (m[:, 0] == 0).sum() > 100
    assert (m[:, 1] < 0).sum() > 100
    small_neg = (m[:, 1] < 0) & (m[:, 1] > -(1 << 20))  # fits in far fewer than 32 bits: a zero-extended low half would show
    assert small_neg.any()
    clamped = [i for i in np.flatnonzero(m[:, 0] >= 2) if _pre_clamp_variance_sign(m[i], sc4) < 0]
    assert len(clamped) >= 3
    assert all(exact["sdx"][i] == 0 and exact["sdy"][i] == 0 and exact["sdz"][i] == 0 for i in clamped)
    ref, exact, mom, sc4 = _run(oracle_mod, synth_mod, "dense")
    m = mom["m"]
    assert m[:, 0].max() >= 4096 and np.abs(m[:, 1:5]).max(axis=0).min() > 1 << 32
    assert (m[:, 1] < 0).any() and (m[:, 0] == 0).any()
    assert np.abs(m[:, 1:5]).max() < m[:, 0].max() * R.ONE_CONTRIBUTION


@pytest.mark.parametrize("name", ["5mm", "1mm", "dense"])
def test_serial_and_sharded_oracle_give_the_same_words_and_rows(oracle_mod, synth_mod, name):
    """Order freedom: the all-cores variant adds the members of a voxel in whatever order its threads arrive (its Welford floats
    differ run to run), the integer words and the rows made from them do not."""
    ref, exact, mom, sc4 = _run(oracle_mod, synth_mod, name)
    sc, cfg = _case(name)
    oracle_mod.set_threads(4)
    og = oracle_mod.OracleGrid(resolution=sc.resolution, bbox=sc.bbox, exact_moments=True, **cfg)
    for ev in sc.schedule():
        if ev[0] == "integrate":
            og.capture_mt(sc.frame(ev[1]), sc.poses[ev[1]])
        else:
            og.clean_mt()
    mom_mt, exact_mt = og.moments(mt=True), og.extract_exact(mt=True)
    og.close()
    assert mom_mt.tobytes() == mom.tobytes()
    assert exact_mt.tobytes() == exact.tobytes()


def test_exact_moments_off_by_default_and_refused_when_off(oracle_mod, synth_mod):
    sc, cfg = _case("5mm")
    og = oracle_mod.OracleGrid(resolution=sc.resolution, bbox=sc.bbox)
    assert og.cfg.exact_moments == 0
    rows = scenes.run(og, sc, "capture")
    with pytest.raises(AssertionError):
        og.moments()
    with pytest.raises(AssertionError):
        og.extract_exact()
    og.close()
    assert rows.tobytes() == _run(oracle_mod, synth_mod, "5mm")[0].tobytes()  # the option changes nothing extract() returns


# ---- the scales ----

def test_scales_on_either_side_of_a_power_of_two(oracle_mod):
    assert len(R.STRADDLES) >= 24
    for K, res, b_below, b_above, which in R.STRADDLES:
        for ball, side in ((b_below, -1), (b_above, 0)):
            bnd = R.bounds(K, res, ball, 0.001)
            sc4 = R.scales(K, res, ball, 0.001)
            og = oracle_mod.OracleGrid(resolution=res, bbox=scenes.BBOX_1M, K=K, ball_radius=ball, exact_moments=True)
            assert np.array_equal(og.scales(), sc4), (K, res, ball)
            og.close()
            for b, f in zip(bnd, sc4):
                m, e = math.frexp(float(f))
                assert m == 0.5, "scale %r is not a power of two" % f
                assert float(f) == math.ldexp(1.0, 26 - R.floor_log2(b)), (K, res, ball, b, f)
                assert 2.0 ** 26 <= b * float(f) < 2.0 ** 27
            # the largest values the bounds admit, as f32: every contribution stays below 2^27 in magnitude
            u = np.float32(bnd[0])
            if float(u) >= bnd[0]:
                u = np.nextafter(u, np.float32(0))
            d = np.nextafter(np.float32(bnd[2]), np.float32(0))
            f32 = [np.float32(v) for v in sc4]
            q = [np.rint(u * f32[0]), np.rint(-u * f32[0]), np.rint((u * u) * f32[1]), np.rint(d * f32[2]), np.rint((d * d) * f32[3])]
            assert all(abs(int(v)) < R.ONE_CONTRIBUTION for v in q), (K, res, ball, q)
            assert max(abs(int(v)) for v in q[:2]) >= R.ONE_CONTRIBUTION // 2 - 8  # and the scale of u wastes no bit


def test_rows_at_a_straddling_scale_pair(oracle_mod, synth_mod):
    """The same scene on either side of the power of two: fs differs by a factor two, the words of u follow, and each side's
    rows are the numpy restatement's byte for byte."""
    K, res, b_below, b_above, which = R.STRADDLE_SCENE
    sc = scenes.Scene(3, 160, 120, res, fx=615.0, clean_every=2)
    out = []
    for ball in (b_below, b_above):
        og = oracle_mod.OracleGrid(resolution=res, bbox=sc.bbox, K=K, ball_radius=ball, exact_moments=True)
        ref = scenes.run(og, sc, "capture")
        exact, mom, sc4 = og.extract_exact(), og.moments(), og.scales()
        og.close()
        nrm = np.stack([ref["nx"], ref["ny"], ref["nz"]], axis=1)
        mine = R.rows_from_moments(mom, nrm, sc.bbox[0::2], res, K=K, ball_radius=ball)
        assert len(ref) > 1000 and mine.tobytes() == exact.tobytes()
        scenes.compare_rows(ref, exact)
        out.append((sc4, mom))
    assert out[0][0][0] == 2 * out[1][0][0], "fs does not double across the power of two"
    assert np.abs(out[0][1]["m"][:, 1:3]).max() < out[0][1]["m"][:, 0].max() * R.ONE_CONTRIBUTION


# ---- hand cases against exact rational arithmetic ----

A = np.array([[0.1234567, -0.2345678, 0.4567891]], np.float32)
AB = np.array([[-0.011, 0.017, -0.022]], np.float32)
SC4 = R.scales()  # the defaults: K = 3, 5 mm, 15 mm ball, 1 mm cylinder


def _frac_row(m, a, ab, sc4):
    """The row expression in exact rationals (no rounding anywhere): x, y, z, var_u, mean_dist, var_dist."""
    n = int(m[0])
    em = Fraction(int(m[1]), int(sc4[0]) * n)
    xyz = [Fraction(float(a[0, i])) - (Fraction(1, 2) + em) * Fraction(float(ab[0, i])) for i in range(3)]
    vs = Fraction(int(m[2]), int(sc4[1]) * n) - em * em
    md = Fraction(int(m[3]), int(sc4[2]) * n)
    vd = Fraction(int(m[4]), int(sc4[3]) * n) - md * md
    return xyz, vs, md, vd


def test_hand_case_one_member():
    """cnt == 1: every product of the expression is exact in f64 (27-bit sums against 24-bit line coordinates), so the row is the
    correctly rounded value of the rational expression, and both variances are exactly zero."""
    s, d = np.float32(0.48291), np.float32(0.00071234)
    q = R.contribution(s, d, SC4)
    m = np.array([[1, int(q[0]), int(q[1]), int(q[2]), int(q[3]), 0, 0, 0]], np.int64)
    assert m[0, 1] < 0  # u = s - 0.5 is negative
    got = R.row_floats(m, A, AB, SC4)
    xyz, vs, md, vd = _frac_row(m[0], A, AB, SC4)
    for i, f in enumerate(("x", "y", "z")):
        assert got[f][0] == np.float32(float(xyz[i])), f
    assert got["mean_dist"][0] == np.float32(float(md))
    assert abs(float(got["mean_dist"][0]) - float(d)) <= 1.0 / float(SC4[2])  # the member's distance to one fixed-point step
    for f in ("sdx", "sdy", "sdz", "sd_dist"):
        assert got[f][0] == 0 and not np.signbit(got[f][0]), f
    assert vs != 0 and vd != 0  # it is the cnt == 1 rule that zeroes them, not the arithmetic


def test_hand_case_negative_sum_of_u():
    """Three members below the cell centre, one of them by a few fixed-point steps only: a small negative word 1."""
    s = np.array([0.5 - 3e-8, 0.5 - 5e-8, 0.5 - 2e-8], np.float32)
    d = np.array([0.0002, 0.0005, 0.0009], np.float32)
    q = R.contribution(s, d, SC4)
    m = np.array([[3] + [int(v.sum()) for v in q] + [0, 0, 0]], np.int64)
    assert -64 < m[0, 1] < 0
    got = R.row_floats(m, A, AB, SC4)
    xyz, vs, md, vd = _frac_row(m[0], A, AB, SC4)
    for i, f in enumerate(("x", "y", "z")):
        exact = float(xyz[i])
        assert abs(float(got[f][0]) - exact) <= abs(float(np.spacing(np.float32(exact)))) / 2 * 1.0001, f
        # the centroid lies on the a side of the cell centre (es < 0.5), by less than a f32 ulp here
        assert abs(exact - (float(A[0, i]) - 0.5 * float(AB[0, i]))) < 1e-8
    # Python-int words give the same bytes as int64 words
    again = R.row_floats(np.array([[int(v) for v in m[0]]], dtype=object), A, AB, SC4)
    assert all(again[f].tobytes() == got[f].tobytes() for f in R.FLOAT_COLUMNS)
    assert abs(float(got["mean_dist"][0]) - float(md)) <= float(md) * 2.0 ** -24
    assert abs(float(got["sd_dist"][0]) - float(vd)) <= float(vd) * 2.0 ** -23


def test_hand_case_variance_negative_before_the_clamp():
    """Two members with the same s: E[u^2] and E[u]^2 agree up to their fixed-point roundings, and here the difference comes out
    below zero; the clamp makes the three per-axis variances exactly +0, never a small negative number or a NaN."""
    rng = np.random.default_rng(5)
    for s in rng.uniform(0.3, 0.7, 4000).astype(np.float32):
        q = R.contribution(np.array([s, s], np.float32), np.array([0.0005, 0.0005], np.float32), SC4)
        m = np.array([[2] + [int(v.sum()) for v in q] + [0, 0, 0]], np.int64)
        if _frac_row(m[0], A, AB, SC4)[1] < 0:
            break
    else:
        raise AssertionError("no s in the sample gives a negative difference")
    xyz, vs, md, vd = _frac_row(m[0], A, AB, SC4)
    assert -Fraction(2, int(SC4[1])) < vs < 0  # within two fixed-point steps of u^2
    got = R.row_floats(m, A, AB, SC4)
    for f in ("sdx", "sdy", "sdz"):
        assert got[f][0] == 0 and not np.signbit(got[f][0]), f
    assert got["sd_dist"][0] >= 0


def test_a_voxel_without_members_is_the_zero_row():
    got = R.row_floats(np.zeros((1, 8), np.int64), A, AB, SC4)
    assert all(got[f].tobytes() == np.zeros(1, np.float32).tobytes() for f in R.FLOAT_COLUMNS)


# ---- what the exact comparison sees that the tolerances do not ----

@pytest.mark.parametrize("word,share", [(1, 1.0), (2, 1.0), (4, 1.0), (3, 0.125)])
def test_one_contribution_hides_in_compare_rows_but_not_in_compare_rows_exact(oracle_mod, synth_mod, word, share):
    """One typical contribution (the voxel's own mean contribution to that word) lost from, or doubled in, the largest voxel of the
    dense scene (n > 10,000): the row made from the altered words still passes every tolerance of compare_rows against the
    reference's recurrence, and fails compare_rows_exact.  Losing the mean contribution of n moves that mean by 1/n of itself:
    1e-5 m on the centroid (a 120 mm segment) hides it from a few hundred members on, 1e-3 on either variance from a few thousand
    on.  mean_dist (word 3, 2e-5 relative) would hide it from n = 50,000 on, where the reference's own f32 recurrence no longer
    keeps its centroid within 1e-5 (the scene at 16 times the density, n = 180,000, is off by 4e-5), so no scene can show that;
    at this n compare_rows sees a whole lost distance and misses an eighth of one, which is what word 3's case alters."""
    ref, exact, mom, sc4 = _run(oracle_mod, synth_mod, "dense")
    sc, cfg = _case("dense")
    i = int(np.argmax(mom["m"][:, 0]))
    n = int(mom["m"][i, 0])
    assert n > 10000
    typical = int(round(share * int(mom["m"][i, word]) / n))
    assert abs(typical) > 1000  # many fixed-point steps: not a rounding matter
    for sign in (-1, 1):
        altered = mom.copy()
        altered["m"][i, word] += sign * typical
        rows = _restated("dense", ref, altered)
        assert rows[i].tobytes() != exact[i].tobytes()
        assert np.delete(rows, i).tobytes() == np.delete(exact, i).tobytes()
        scenes.compare_rows(ref, rows)  # the tolerances do not see it
        with pytest.raises(AssertionError):
            scenes.compare_rows_exact(exact, rows, cylinder_radius=cfg["cylinder_radius"])
    if word == 3:  # a whole contribution is within compare_rows' reach at this count
        altered = mom.copy()
        altered["m"][i, word] -= int(round(int(mom["m"][i, word]) / n))
        with pytest.raises(AssertionError, match="mean_dist"):
            scenes.compare_rows(ref, _restated("dense", ref, altered))
