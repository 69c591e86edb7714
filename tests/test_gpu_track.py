"""GPU: refining a frame's pose against the fused model (hfpf_track_depth, hfpf_track_depth_device, hfpf_track).  A track is
defined on the rows hfpf_extract returns, so its results are compared byte for byte with tests/track_ref.py run on the extracted
rows."""
import ctypes as C

import numpy as np
import pytest

import depth_ref
import track_ref as TR
from gpu_support import (TRACK_OPTS, Z_CLIP, Z_RANGE, grid, held_out, perturb, pose_errors, run, same_planes, same_track, track_reference,
                         two_handles, unchanged, uploaded)
from scenes import DepthScene

pytestmark = pytest.mark.gpu


def _as_f32(depth):
    d = depth.astype(np.float32) * np.float32(0.001)
    d[depth == 0] = np.nan
    return d


def _wide(cloud):
    """The records of a packed cloud in a 32-byte layout with x, y, z behind a pad word: the generic loader."""
    wide = np.zeros((cloud.nbytes // 16, 8), np.uint32)
    wide[:, 1:4] = cloud.view(np.uint32).reshape(-1, 4)[:, :3]
    return wide.view(np.uint8).reshape(-1)


PACKED = dict(point_step=16, off_x=0, off_y=4, off_z=8)
WIDE = dict(point_step=32, off_x=4, off_y=8, off_z=12)


def _bytes(res):
    pose, r = res
    return pose.tobytes() + r["information"].tobytes() + np.float64(r["rms"]).tobytes() + bytes(
        str((r["iterations"], r["flags"], r["inliers"], r["points_used"])), "ascii")


@pytest.fixture(scope="module")
def session(hfpf_mod, synth_mod):
    sc = DepthScene(12, 640, 480, clean_every=4)
    g = grid(hfpf_mod)
    run(g, sc)
    rows = g.extract().copy()
    yield sc, g, rows
    g.close()


# ---- 1. bit-exact against the numpy contract -------------------------------------------------------------------------

# fmt: a u16 or f32 depth image, or the same points as a packed or a 32-byte-record cloud (sampled as record i % stride == 0)
@pytest.mark.parametrize("stride,fmt", [(1, "u16"), (2, "f32"), (2, "u16"), (1, "f32"), (2, "packed"), (2, "wide")])
def test_bit_exact_against_track_ref(hfpf_mod, synth_mod, session, stride, fmt):
    sc, g, rows = session
    depth, K, true = held_out(synth_mod)
    guess = perturb(true, 2.0, (0.006, -0.005, 0.006))  # 1 cm, 2 degrees
    if fmt in ("u16", "f32"):
        img = depth if fmt == "u16" else _as_f32(depth)
        got = g.track_depth(img, guess, K, stride=stride, **TRACK_OPTS)
        ref = track_reference(rows, TR.depth_points(img, K, stride), guess, K, 640, 480)
    else:
        cloud = depth_ref.packed_cloud(depth, K)
        xyz = cloud.view(np.float32).reshape(-1, 4)[:, :3]
        got = g.track(cloud if fmt == "packed" else _wide(cloud), PACKED if fmt == "packed" else WIDE, guess, K, 640, 480,
                      stride=stride, **TRACK_OPTS)
        ref = track_reference(rows, TR.cloud_points(xyz, stride), guess, K, 640, 480)
    print("stride %d %s: %d iterations, flags %d, %d of %d used points inliers, rms %.2e, error %s -> %s" % (
        stride, fmt, got[1]["iterations"], got[1]["flags"], got[1]["inliers"], got[1]["points_used"], got[1]["rms"],
        pose_errors(guess, true), pose_errors(got[0], true)))
    same_track(got, ref, "stride %d, %s depth" % (stride, fmt))
    assert got[1]["iterations"] > 1 and got[1]["inliers"] > 1000


# The shared sample loop outside the sizes the tests above give it: kTrackMaxBlocks * 256 = 524,288 threads, one block = 256.

@pytest.fixture(scope="module")
def held_out_cloud(synth_mod):
    depth, K, true = held_out(synth_mod)
    return depth_ref.packed_cloud(depth, K), K, perturb(true, 2.0, (0.006, -0.005, 0.006))


@pytest.fixture(scope="module")
def doubled(session, held_out_cloud):
    """The held-out frame's cloud twice over (614,400 records) and its reference result, computed once for both forms."""
    cloud, K, guess = held_out_cloud
    both = np.concatenate([cloud.reshape(-1), cloud.reshape(-1)])
    xyz = both.view(np.float32).reshape(-1, 4)[:, :3]
    assert len(xyz) == 2 * 640 * 480 > 2048 * 256
    return both, track_reference(session[2], TR.cloud_points(xyz, 1), guess, K, 640, 480, max_iterations=2)


@pytest.mark.parametrize("fmt", ["packed", "wide"])
def test_more_samples_than_grid_threads(hfpf_mod, session, held_out_cloud, doubled, fmt):
    """Every thread of the full grid takes a second trip of the grid-stride loop."""
    sc, g, rows = session
    _, K, guess = held_out_cloud
    both, ref = doubled
    got = g.track(both if fmt == "packed" else _wide(both), PACKED if fmt == "packed" else WIDE, guess, K, 640, 480, stride=1,
                  **dict(TRACK_OPTS, max_iterations=2))
    print("%s: %d iterations, flags %d, %d of %d used points inliers" % (fmt, got[1]["iterations"], got[1]["flags"], got[1]["inliers"],
                                                                       got[1]["points_used"]))
    same_track(got, ref, "614,400 records, %s" % fmt)
    assert got[1]["points_used"] == ref["points_used"] > 2048 * 256 // 2


def test_fewer_samples_than_one_wave(hfpf_mod, session, held_out_cloud):
    """40 used points: three of the block's four waves contribute zeros.  Below min_inliers = 6 inliers the result must be the
    reference's TOO_FEW with the same sums."""
    sc, g, rows = session
    cloud, K, guess = held_out_cloud
    rec = cloud.view(np.float32).reshape(-1, 4)
    few = np.ascontiguousarray(rec[TR.used(rec[:, :3], Z_CLIP)][:40])
    assert len(few) == 40
    got = g.track(few.view(np.uint8).reshape(-1), PACKED, guess, K, 640, 480, stride=1, **TRACK_OPTS)
    ref = track_reference(rows, TR.cloud_points(few[:, :3], 1), guess, K, 640, 480)
    print("40 records: %d iterations, flags %d, %d of %d used points inliers" % (got[1]["iterations"], got[1]["flags"], got[1]["inliers"],
                                                                              got[1]["points_used"]))
    same_track(got, ref, "40 records")
    assert got[1]["points_used"] == 40 and (got[1]["inliers"] >= 6 or got[1]["flags"] == TR.TOO_FEW)


# ---- 2. accuracy ----------------------------------------------------------------------------------------------------
# Targets: translation error <= 1 mm and rotation error <= 0.1 degrees, and always at least 10x smaller than at the start.  The
# first MI355X run measured 0.046-0.049 mm / 0.015-0.024 degrees from these starts (and 0.042 mm / 0.012 degrees from the true
# pose): the targets leave room for a change of scene or schedule and still fail a wrong Jacobian, gate or update.
MAX_T_ERR, MAX_R_ERR = 1e-3, 0.1


@pytest.mark.parametrize("deg,shift", [(1.0, (0.006, -0.005, 0.006)), (3.0, (0.012, 0.01, -0.01)), (2.0, (0.0, 0.015, 0.0)),
                                       (1.5, (-0.01, 0.0, 0.012))])
def test_accuracy_at_640x480(hfpf_mod, synth_mod, session, deg, shift):
    sc, g, rows = session
    depth, K, true = held_out(synth_mod)
    guess = perturb(true, deg, shift)
    e0 = pose_errors(guess, true)
    pose, r = g.track_depth(depth, guess, K, **TRACK_OPTS)
    e1 = pose_errors(pose, true)
    print("start %.4f m / %.3f deg -> %.6f m / %.4f deg: %d iterations, flags %d, %d inliers, rms %.2e" % (
        *e0, *e1, r["iterations"], r["flags"], r["inliers"], r["rms"]))
    assert e1[0] * 10 <= e0[0] and e1[1] * 10 <= e0[1]
    assert e1[0] <= MAX_T_ERR and e1[1] <= MAX_R_ERR


def test_starting_at_the_true_pose_stays_there(hfpf_mod, synth_mod, session):
    sc, g, rows = session
    depth, K, true = held_out(synth_mod)
    pose, r = g.track_depth(depth, true, K, **TRACK_OPTS)
    e = pose_errors(pose, true)
    print("from the true pose: %.6f m / %.4f deg in %d iterations, flags %d" % (*e, r["iterations"], r["flags"]))
    assert r["flags"] == TR.CONVERGED and r["iterations"] <= 3
    assert e[0] < 2e-4


# ---- 3. equivalent inputs ---------------------------------------------------------------------------------------------

def test_cloud_host_and_device_depth_agree(hfpf_mod, synth_mod, session):
    sc, g, rows = session
    depth, K, true = held_out(synth_mod)
    guess = perturb(true, 1.0, (0.004, 0.004, -0.004))
    a = g.track_depth(depth, guess, K, **TRACK_OPTS)
    cloud = depth_ref.packed_cloud(depth, K)
    b = g.track(cloud, PACKED, guess, K, 640, 480, **TRACK_OPTS)
    c = g.track(_wide(cloud), WIDE, guess, K, 640, 480, **TRACK_OPTS)
    desc = hfpf_mod.depth_desc(640, 480, hfpf_mod.DEPTH_U16, 640 * 2, K)
    with uploaded(g, depth) as (ptr,):
        d = g.track_depth_device(desc, ptr, guess, **TRACK_OPTS)
    assert a[1]["inliers"] > 1000
    for what, other in (("packed cloud", b), ("32-byte cloud", c), ("device depth", d)):
        assert _bytes(other) == _bytes(a), what


# ---- 4. no side effects ---------------------------------------------------------------------------------------------

def test_tracks_change_nothing(hfpf_mod, synth_mod):
    sc = DepthScene(10, 320, 240, clean_every=3)
    depth, K, true = held_out(synth_mod, 320, 240)

    def look(g, i):
        g.track_depth(depth, perturb(true, 1.0, (0.005, 0.0, 0.0)), K, **dict(TRACK_OPTS, max_iterations=3))

    with two_handles(hfpf_mod, sc, look, lambda b: look(b, -1)) as (a, b, rb):
        ia = a.render(sc.poses[2], K, sc.W, sc.H, z_range=Z_RANGE, splat_radius=-1)
        same_planes(ia, b.render(sc.poses[2], K, sc.W, sc.H, z_range=Z_RANGE, splat_radius=-1), "a render of both handles")
        unchanged(a, b, rb)


# ---- 5. edges -------------------------------------------------------------------------------------------------------

def test_empty_and_uncleaned_handles_return_the_guess(hfpf_mod, synth_mod):
    sc = DepthScene(3, 160, 120, clean_every=0)
    depth, K, true = held_out(synth_mod, 160, 120)
    guess = perturb(true, 1.0, (0.01, 0.0, 0.0))
    with grid(hfpf_mod) as g:
        for label in ("empty", "integrated, never cleaned"):
            pose, r = g.track_depth(depth, guess, K, **TRACK_OPTS)
            assert r["flags"] == TR.TOO_FEW and r["inliers"] == 0 and r["iterations"] == 1, label
            assert pose.tobytes() == guess.tobytes(), label
            assert r["points_used"] > 1000, label
            for f in range(sc.n_frames):  # no clean pass: extract returns no rows yet
                sc.integrate(g, f)
        assert len(g.extract()) == 0
        g.clean()
        pose, r = g.track_depth(depth, guess, K, **TRACK_OPTS)
        assert r["flags"] != TR.TOO_FEW and r["inliers"] > 1000


def test_bad_arguments_are_refused_and_the_handle_stays_usable(hfpf_mod, synth_mod, session):
    H_ = hfpf_mod
    sc, g, rows = session
    L = H_.lib()
    depth, K, true = held_out(synth_mod, 160, 120)
    pose = np.ascontiguousarray(true, np.float64).reshape(12)
    want = g.track_depth(depth, true, K, **TRACK_OPTS)
    desc0 = H_.depth_desc(160, 120, H_.DEPTH_U16, 320, K)
    bad_opts = {"struct_size": ("struct_size", C.sizeof(H_.TrackOpts) - 8), "reserved": ("reserved", 1),
                "iterations 0": ("max_iterations", 0), "iterations 65": ("max_iterations", 65), "stride 0": ("stride", 0),
                "stride 17": ("stride", 17), "min_inliers 5": ("min_inliers", 5), "max_distance 0": ("max_distance", 0.0),
                "max_distance 1.5": ("max_distance", 1.5), "max_distance nan": ("max_distance", float("nan")),
                "damping -1": ("damping", -1.0), "damping inf": ("damping", float("inf")), "eps_rotation -1": ("eps_rotation", -1.0),
                "eps_translation nan": ("eps_translation", float("nan"))}
    bad_view = {"view struct_size": ("struct_size", 8), "view flags": ("flags", 8), "view width 0": ("width", 0),
                "view fx 0": ("fx", 0.0), "view z_near >= z_far": ("z_near", 5.0), "view radius 16": ("splat_radius", 16)}

    def opts():
        return H_.track_opts(K, 160, 120, **TRACK_OPTS)

    def call(o=None, desc=None, img=depth, p=pose, res=None):
        r = res if res is not None else H_.track_result()
        return L.hfpf_track_depth(g._h, C.byref(o or opts()), C.byref(desc or desc0), C.c_void_p(img.ctypes.data) if img is not None else None,
                                  p.ctypes.data if p is not None else None, C.byref(r))

    assert call() == 0
    for what, (field, val) in bad_opts.items():
        o = opts()
        setattr(o, field, val)
        assert call(o) == -2, what
    for what, (field, val) in bad_view.items():
        o = opts()
        setattr(o.view, field, val)
        assert call(o) == -2, what
    for what, (field, val) in {"desc struct_size": ("struct_size", 8), "desc format": ("depth_format", 7), "desc step": ("depth_step", 100),
                               "desc fx": ("fx", -1.0), "desc colour format": ("color_format", 9)}.items():
        d = H_.depth_desc(160, 120, H_.DEPTH_U16, 320, K)
        setattr(d, field, val)
        assert call(desc=d) == -2, what
    assert call(img=None) == -2, "NULL depth"
    assert call(p=None) == -2, "NULL pose"
    nan_pose = pose.copy()
    nan_pose[3] = np.nan
    assert call(p=nan_pose) == -2, "non-finite pose"
    r = H_.track_result()
    r.struct_size = 8
    assert call(res=r) == -2, "result struct_size"
    assert L.hfpf_track_depth(g._h, C.byref(opts()), C.byref(desc0), C.c_void_p(depth.ctypes.data), pose.ctypes.data, None) == -2
    assert L.hfpf_track_depth(g._h, None, C.byref(desc0), C.c_void_p(depth.ctypes.data), pose.ctypes.data, C.byref(H_.track_result())) == -2
    ptr = g.device_alloc(depth.nbytes + 2)
    try:
        assert L.hfpf_track_depth_device(g._h, C.byref(opts()), C.byref(desc0), C.c_void_p(ptr + 1), pose.ctypes.data,
                                         C.byref(H_.track_result())) == -2, "misaligned device image"
    finally:
        g.device_free(ptr)
    cloud = depth_ref.packed_cloud(depth, K)
    for what, (n, step, ox, oy, oz) in {"no points": (0, 16, 0, 4, 8), "step 18": (100, 18, 0, 4, 8), "off_y 6": (100, 16, 0, 6, 8),
                                        "off_z beyond step": (100, 16, 0, 4, 16)}.items():
        assert L.hfpf_track(g._h, C.byref(opts()), C.c_void_p(cloud.ctypes.data), n, step, ox, oy, oz, pose.ctypes.data,
                            C.byref(H_.track_result())) == -2, what
    assert L.hfpf_track(g._h, C.byref(opts()), None, 100, 16, 0, 4, 8, pose.ctypes.data, C.byref(H_.track_result())) == -2, "NULL cloud"
    # the handle is still usable, and two identical calls give identical bytes
    again = g.track_depth(depth, true, K, **TRACK_OPTS)
    assert _bytes(again) == _bytes(want) and _bytes(g.track_depth(depth, true, K, **TRACK_OPTS)) == _bytes(want)
