"""CPU: the depth-consistency contract (include/hfpf.h) as tests/consistency_ref.py restates it -- hand-built cases with one row and a
4 x 4 frame for every class and every boundary the contract names, the vectorised form against the scalar double loop, and every
rejected field of hfpf_check_consistency_opts through the built library (host code: no GPU)."""
import numpy as np
import pytest

import consistency_ref as CR

IDENT = np.eye(4)[:3]
K4 = (2.0, 2.0, 2.0, 2.0)  # a row on the optical axis lands on pixel (2, 2) of a 4 x 4 frame
KW = dict(window=0, z_range=(0.125, 4.0), tolerance=0.125, slope=0.0, min_cos=0.0)


def _row(H, xyz=(0.0, 0.0, 0.5), n=(0.0, 0.0, -1.0), count=5):
    r = np.zeros(1, H.ROW_DTYPE)
    r["x"], r["y"], r["z"] = xyz
    r["nx"], r["ny"], r["nz"] = n
    r["count"] = count
    return r


def _frame(centre, fill=np.nan):
    f = np.full((4, 4), fill, np.float32)
    f[2, 2] = centre
    return f


def _cls(rows, frame, pose=IDENT, K=K4, **kw):
    o = dict(KW, **kw)
    c = CR.classify(rows, frame, pose, K, **o)
    assert int(c[0]) == CR.scalar_class(rows[0], frame, pose, K, **o), "vectorised and scalar forms differ"
    return int(c[0])


def test_one_case_per_class(hfpf_mod):
    r = _row(hfpf_mod)
    assert _cls(r, _frame(0.5)) == CR.SUPPORT
    assert _cls(r, _frame(np.nan)) == CR.NO_DEPTH
    assert _cls(r, _frame(0.25)) == CR.OCCLUDED
    assert _cls(r, _frame(1.0)) == CR.THROUGH
    assert _cls(r, _frame(0.5), min_cos=0.5, pose=IDENT) == CR.SUPPORT
    assert _cls(_row(hfpf_mod, n=(0.0, 0.0, 1.0)), _frame(0.5)) == CR.IN_VIEW, "a back-facing row is in view and not tested"
    assert _cls(_row(hfpf_mod, xyz=(0.0, 0.0, 8.0)), _frame(0.5)) == 0, "behind z_far"
    assert _cls(_row(hfpf_mod, xyz=(0.0, 0.0, 0.125)), _frame(0.125)) == 0, "zc == z_near is outside"
    assert _cls(_row(hfpf_mod, xyz=(1.0, 0.0, 0.5)), _frame(0.5)) == 0, "u = 6 is outside a 4-pixel row"


def test_tolerance_boundaries_are_support(hfpf_mod):
    r = _row(hfpf_mod)
    assert _cls(r, _frame(0.625)) == CR.SUPPORT, "g == tol"
    assert _cls(r, _frame(0.375)) == CR.SUPPORT, "g == -tol"
    assert _cls(r, _frame(np.nextafter(np.float32(0.625), np.float32(1)))) == CR.THROUGH
    assert _cls(r, _frame(np.nextafter(np.float32(0.375), np.float32(0)))) == CR.OCCLUDED
    # tol = tolerance + slope * zc, exactly: 0.0625 + 0.125 * 0.5 = 0.125
    assert _cls(r, _frame(0.625), tolerance=0.0625, slope=0.125) == CR.SUPPORT
    assert _cls(r, _frame(0.625), tolerance=0.0625, slope=0.0) == CR.THROUGH


def test_window_rule(hfpf_mod):
    r = _row(hfpf_mod)
    f = _frame(2.0)          # the centre pixel is far behind the row ...
    assert _cls(r, f, window=0) == CR.THROUGH
    f[1, 3] = 0.5            # ... and a pixel of the 3 x 3 window supports it
    assert _cls(r, f, window=0) == CR.THROUGH and _cls(r, f, window=1) == CR.SUPPORT
    f[1, 3] = 0.25           # an occluder beside a far pixel
    assert _cls(r, f, window=1) == CR.OCCLUDED
    assert _cls(r, np.full((4, 4), np.nan, np.float32), window=2) == CR.NO_DEPTH, "all invalid"
    g = np.full((4, 4), np.nan, np.float32)
    g[0, 0] = 0.5            # two pixels from the centre: only window 2 reaches it
    assert _cls(r, g, window=1) == CR.NO_DEPTH and _cls(r, g, window=2) == CR.SUPPORT
    # a window that leaves the image: the row at pixel (0, 0), the supporting pixel at (1, 1)
    h = np.full((4, 4), np.nan, np.float32)
    h[1, 1] = 0.5
    assert _cls(_row(hfpf_mod, xyz=(-0.5, -0.5, 0.5)), h, window=1) == CR.SUPPORT


def test_pixel_rounding_at_half(hfpf_mod):
    """u = k + 0.5 rounds up: pu = floor(u + 0.5) = k + 1."""
    f = np.full((4, 4), np.nan, np.float32)
    f[2, 2] = 0.5
    K = (2.0, 2.0, 1.5, 2.0)  # u = 1.5 -> pu = 2
    assert _cls(_row(hfpf_mod), f, K=K) == CR.SUPPORT
    K = (2.0, 2.0, float(np.nextafter(1.5, 0.0)), 2.0)  # just below: pu = 1
    assert _cls(_row(hfpf_mod), f, K=K) == CR.NO_DEPTH
    K = (2.0, 2.0, -0.5, 2.0)  # u = -0.5 -> pu = 0: in view
    assert _cls(_row(hfpf_mod), f, K=K) == CR.NO_DEPTH
    K = (2.0, 2.0, float(np.nextafter(-0.5, -1.0)), 2.0)  # pu = -1
    assert _cls(_row(hfpf_mod), f, K=K) == 0


def test_facing_gate(hfpf_mod):
    f = _frame(0.5)
    assert _cls(_row(hfpf_mod, n=(1.0, 0.0, 0.0)), f, min_cos=0.0) == CR.IN_VIEW, "c == 0 fails c > 0"
    # d = (0, 0, 0.5), d2 = 0.25; n = (0, 0, -0.5): c = 0.25, c * c = 0.0625 = 0.5^2 * 0.25
    assert _cls(_row(hfpf_mod, n=(0.0, 0.0, -0.5)), f, min_cos=0.5) == CR.SUPPORT, "c * c == min_cos^2 * d2 passes"
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    assert _cls(_row(hfpf_mod, n=(0.0, 0.0, -below)), f, min_cos=0.5) == CR.IN_VIEW
    for n in ((1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, 0.0)):
        assert _cls(_row(hfpf_mod, n=n), f, min_cos=-1.0) == CR.SUPPORT, "min_cos < 0 switches the gate off"


def _random_case(H, n_rows, n_frames, W=24, Hh=16, seed=7):
    rng = np.random.default_rng(seed)
    rows = np.zeros(n_rows, H.ROW_DTYPE)
    rows["x"], rows["y"] = rng.uniform(-0.3, 0.3, n_rows), rng.uniform(-0.2, 0.2, n_rows)
    rows["z"] = rng.uniform(0.2, 0.9, n_rows)
    n = rng.normal(size=(n_rows, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    n[:, 2] = -np.abs(n[:, 2])
    rows["nx"], rows["ny"], rows["nz"] = n.T
    rows["count"] = rng.integers(0, 9, n_rows)
    frames = rng.integers(300, 900, (n_frames, Hh, W)).astype(np.uint16)
    frames[rng.random(frames.shape) < 0.2] = 0
    # a third of the pixels agree with the plane z = 0.5 to within the tolerance
    frames[rng.random(frames.shape) < 0.3] = 500
    poses = []
    for f in range(n_frames):
        p = np.eye(4)[:3].copy()
        p[:, 3] = rng.uniform(-0.02, 0.02, 3)
        poses.append(p)
    K = (20.0, 20.0, 11.5, 7.5)
    return rows, frames, poses, K


def test_scalar_loop_equals_the_vectorised_form(hfpf_mod):
    rows, frames, poses, K = _random_case(hfpf_mod, 300, 5)
    for window in (0, 1, 2):
        kw = dict(window=window, z_range=(0.25, 0.8), tolerance=0.02, slope=0.01, min_cos=0.3)
        got_rows, rec, s = CR.consistency(rows, frames, poses, K, min_through=1, through_ratio=1.0, **kw)
        want = CR.scalar_records(got_rows, frames, poses, K, 0.001, **kw)
        CR.finish(want)
        assert rec.tobytes() == want.tobytes(), "window %d" % window
        for cls in ("n_support", "n_through", "n_occluded"):
            assert rec[cls].sum() > 20, "the random case exercises %s" % cls
        assert s["pairs_tested"] == int(rec["n_tested"].sum()) and s["n_rows"] == len(rows)
    dropped, _, _ = CR.consistency(rows, frames, poses, K, min_count=4.0)
    assert 0 < len(dropped) < len(rows) and (dropped["count"] >= 4).all()


def test_u16_and_f32_frames_give_identical_records(hfpf_mod):
    rows, frames, poses, K = _random_case(hfpf_mod, 200, 3, seed=11)
    f32 = np.stack([CR.as_f32(f, 0.001) for f in frames])
    kw = dict(window=1, z_range=(0.25, 0.8), tolerance=0.004, slope=0.0, min_cos=-1.0)
    a = CR.consistency(rows, frames, poses, K, 0.001, **kw)
    b = CR.consistency(rows, f32, poses, K, 0.001, **kw)
    assert a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    assert np.isnan(f32).sum() == (frames == 0).sum() > 0


def test_depth_step_larger_than_the_row(hfpf_mod):
    rows, frames, poses, K = _random_case(hfpf_mod, 200, 2, seed=13)
    wide = np.full((2, 16, 40), 0xFFFF, np.uint16)
    wide[:, :, :24] = frames
    view = wide[:, :, :24]
    assert view.strides[1] == 80 and not view.flags["C_CONTIGUOUS"]
    kw = dict(window=2, z_range=(0.25, 0.8), tolerance=0.004)
    assert CR.consistency(rows, view, poses, K, **kw)[1].tobytes() == CR.consistency(rows, frames, poses, K, **kw)[1].tobytes()


def test_keep_rule_at_the_ratio():
    rec = np.zeros(5, CR.DTYPE)
    rec["n_tested"] = 6
    rec["n_through"] = (2, 3, 2, 0, 1)
    rec["n_support"] = (2, 2, 0, 4, 1)
    contra, s = CR.finish(rec, min_through=1, through_ratio=1.0)
    assert contra.tolist() == [False, True, True, False, False], "n_through == through_ratio * n_support keeps the row"
    assert s["n_contradicted"] == 2 and s["n_kept"] == 3 and s["n_supported"] == 4 and s["n_seen"] == 5
    assert rec["flags"].tolist() == [3, 7, 5, 3, 3]
    contra, _ = CR.finish(rec, min_through=3, through_ratio=1.0)
    assert contra.tolist() == [False, True, False, False, False], "fewer than min_through THROUGH frames never contradict"
    contra, _ = CR.finish(rec, min_through=0, through_ratio=0.0)
    assert contra.tolist() == [True, True, True, False, True], "min_through 0 counts as 1; ratio 0 needs one THROUGH frame"
    contra, _ = CR.finish(rec, min_through=1, through_ratio=1.5)
    assert contra.tolist() == [False, False, True, False, False], "3 > 1.5 * 2 is false"


def test_records_count_frames_and_keep_the_first_through():
    cls = np.array([[CR.SUPPORT, 0, CR.IN_VIEW], [CR.THROUGH, CR.OCCLUDED, CR.NO_DEPTH], [CR.THROUGH, CR.THROUGH, 0]])
    rec = CR.records_of(cls)
    assert rec["n_in_view"].tolist() == [3, 2, 2] and rec["n_tested"].tolist() == [3, 2, 1]
    assert rec["n_support"].tolist() == [1, 0, 0] and rec["n_through"].tolist() == [2, 1, 0] and rec["n_occluded"].tolist() == [0, 1, 0]
    assert rec["first_through"].tolist() == [1, 2, CR.NONE]
    assert CR.records_of(np.zeros((0, 2), np.int8))["first_through"].tolist() == [CR.NONE, CR.NONE], "no frames"


BAD = [("struct_size", 0), ("struct_size", 64), ("flags", 2), ("flags", 0x80000001), ("reserved", 1), ("window", -1), ("window", 3),
       ("min_count", float("nan")), ("z_near", 0.0), ("z_near", -1.0), ("z_near", float("nan")), ("z_near", 200.0), ("z_far", float("inf")),
       ("z_far", float("nan")), ("tolerance", 0.0), ("tolerance", -0.001), ("tolerance", 1.5), ("tolerance", float("nan")),
       ("tolerance", float("inf")), ("slope", -0.1), ("slope", 1.5), ("slope", float("nan")), ("min_cos", -1.5), ("min_cos", 1.5),
       ("min_cos", float("nan")), ("through_ratio", -0.5), ("through_ratio", float("nan")), ("through_ratio", float("inf"))]


def test_check_consistency_opts_accepts_the_ranges(hfpf_mod):
    assert hfpf_mod.check_consistency_opts(hfpf_mod.consistency_opts()) == 0
    assert hfpf_mod.check_consistency_opts(None) == -2
    for kw in (dict(window=2, drop=True), dict(tolerance=1.0, slope=1.0), dict(slope=0.0, min_cos=-1.0), dict(min_cos=1.0, through_ratio=0.0),
               dict(min_count=float("inf")), dict(min_through=0), dict(min_through=0xFFFFFFFF)):
        assert hfpf_mod.check_consistency_opts(hfpf_mod.consistency_opts(**kw)) == 0, kw


@pytest.mark.parametrize("field,value", BAD)
def test_check_consistency_opts_rejects(hfpf_mod, field, value):
    o = hfpf_mod.consistency_opts()
    setattr(o, field, value)
    assert hfpf_mod.check_consistency_opts(o) == -2, (field, value)
