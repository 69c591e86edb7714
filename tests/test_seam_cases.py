"""CPU: every case of tests/seams.py is what it claims to be, from the oracle alone.  A GPU case of test_gpu_integrate_seams.py whose
cloud misses its seam -- too few tiles for the grid-stride loop, a frame without a partial tile, a model without rows, an interval
that clips nothing -- is a test of the common path: the preconditions are asserted here.

  rows        a case that claims rows has MIN_ROWS oracle rows with members and a finite normal, a base-model case MIN_ROWS_BASE
              (behind its first clean pass already)
  clips       between 5 % and 95 % of its points pass the z-clip and the bounding box
  many tiles  the launches that claim it have MANY_TILES tiles, and (tile loop) frames that end in a partial tile
  time        no oracle run takes more than ORACLE_SECONDS (capture and clean; 2.5 s for the slowest on an idle core)
and, per group, that the builders lay the same points out as they say."""
import os
import re

import numpy as np
import pytest

import crafted
import depth_ref as R
import seams as X

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "high-fidelity-pointcloud-fusion_amd", "csrc")
ORACLE_SECONDS = 8.0   # "a few seconds": three times the slowest run on an idle core, for a loaded machine


@pytest.fixture(scope="module", autouse=True)
def _drop_the_cases():
    yield
    X.forget_all()


def _claims(oracle_mod, case, colour=False):
    run = X.oracle_run(oracle_mod, case, colour)
    live = [X.live_rows(rows) for rows, _ in run["snaps"]]
    ctr = run["counters"][-1]
    share = ctr["inserted"] / ctr["presented"]
    print("%s: %.2f s, live rows behind the clean passes %r, %d points, %.3f pass both clips, tiles %r" % (
        case.name, run["seconds"], live, ctr["presented"], share, [op.tiles for op in case.launches]))
    assert run["seconds"] <= ORACLE_SECONDS, "%s: the oracle took %.1f s" % (case.name, run["seconds"])
    assert ctr["presented"] == sum(op.n_points * op.n_frames for op in case.launches)
    if case.kind == "empty":
        assert ctr["zclip_pass"] == 0 and ctr["inserted"] == 0 and all(len(rows) == 0 for rows, _ in run["snaps"]), "%s is not empty" % case.name
        return run
    assert live[-1] >= case.min_rows, "%s: %d live rows, claims %d" % (case.name, live[-1], case.min_rows)
    if case.kind == "base":
        assert live[0] >= X.MIN_ROWS_BASE, "%s: the base model has %d live rows" % (case.name, live[0])
    assert 0.05 <= share <= 0.95, "%s: %.3f of the points pass both clips" % (case.name, share)
    for i in case.many:
        op = case.ops[i]
        assert op.tiles >= X.MANY_TILES, "%s: launch %d has %d tiles" % (case.name, i, op.tiles)
        if case.partial:
            assert op.n_points % X.TILE != 0, "%s: launch %d has frames of whole tiles" % (case.name, i)
    return run


# ---- the engine's rules the cases are built on ---------------------------------------------------------------------------------------------

def test_rules_are_those_of_the_engine():
    plan = open(os.path.join(CSRC, "host_plan.hpp")).read()
    m = re.search(r"inline uint32_t tile_row_width\(uint32_t fw, uint32_t n_points\) \{ return (.*); \}", plan)
    assert m and m.group(1) == X.TILE_ROW_WIDTH_RULE, "tile_row_width changed: revisit seams.PATCH_SHAPES and seams.IGNORED_HINTS"
    host = open(os.path.join(CSRC, "hfpf.hip")).read()
    # one workgroup per tile up to integrate_grid = workgroups per CU x CUs: at most 8 x 256 on an MI355X
    assert "std::min<uint64_t>(n_tiles, (uint64_t)h->integrate_grid)" in host and "h->integrate_grid = std::max(1, per_cu) * std::max(1, cus);" in host
    assert X.INTEGRATE_GRID_MAX == crafted.INTEGRATE_GRID == 8 * 256 and X.MANY_TILES >= 4 * X.INTEGRATE_GRID_MAX
    # packed16 takes the 16-byte loads only for x, y, z, rgb at 0, 4, 8, 12 of 16-byte records, a 16-byte aligned base and stride
    assert re.search(r"lay\.point_step == 16 && lay\.off_x == 0 && lay\.off_y == 4 && lay\.off_z == 8 && \(\(uintptr_t\)base & 15\) == 0 &&\s*"
                     r"\(!with_rgb \|\| \(lay\.off_rgb == 12 && \(frame_stride & 15\) == 0\)\)", host), "packed16 changed: revisit the record-form cases"
    kernels = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert "const uint32_t tiles_per_frame = (n_pts + 255u) >> 8;" in kernels and X.TILE == 256


def test_patch_hints():
    for fw, (W, H, n) in X.PATCH_SHAPES.items():
        assert fw == W and X.tile_row_width(fw, W * H) == fw, "frame_width %d is not taken for %d x %d" % (fw, W, H)
        assert X.tiles(W * H, n) >= X.MANY_TILES
    n = 48 * 24
    for fw in X.IGNORED_HINTS:
        assert X.tile_row_width(fw, n) == 0, "frame_width %d is taken for 48 x 24" % fw
    assert 24 % 16 and n % 80 and 8 < 16 and 2000 > n and n % 24 == 0 and (n // 24) % 16 == 0 and 24 % 16
    # organised single frames: 16 x 16 takes the patch walk in the depth form, 8 x 8 must not
    assert X.tile_row_width(16, 256) == 16 and X.tile_row_width(8, 64) == 0


# ---- 1. tile loop ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_pts", list(X.SINGLE_SHAPES))
def test_single_frames(oracle_mod, synth_mod, n_pts):
    case = X.single_frame(n_pts)
    run = _claims(oracle_mod, case)
    single = case.launches[1]
    assert single.n_frames == 1 and single.n_points == n_pts and case.ops[1] is X.CLEAN
    # the counters see the lone frame even where it adds no row
    assert run["counters"][2]["presented"] - run["counters"][1]["presented"] == n_pts
    assert sorted(X.SINGLE_SHAPES) == [1, 63, 64, 65, 255, 256, 257, 511, 513]


@pytest.mark.parametrize("shape", list(X.MANY_SHAPES))
def test_many_tiles(oracle_mod, synth_mod, shape):
    case = X.many_tiles(shape)
    _claims(oracle_mod, case)
    tails = {"small": 16, "large": 1}
    for op in case.launches:
        assert op.n_points % X.TILE == tails[shape]
    for op, (order, ids) in zip(case.launches, X.shuffled_ids(case)):
        assert sorted(order) == list(range(op.n_frames)) and (np.diff(ids.astype(np.int64)) < 0).any(), "the ids are monotone"
        assert int(ids.max()) < case.caps["max_frames"]
    fr = case.launches[0].frames
    assert fr.depth is not None and fr.depth.shape[1:] == (fr.H, fr.W) and fr.W % 2 == 1, "an odd width with u16 samples"
    X.forget(case)


# ---- 3. patch walk -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", list(X.PATCH_SHAPES))
def test_patch_walk(oracle_mod, synth_mod, width):
    case = X.patch_walk(width)
    _claims(oracle_mod, case)
    assert case.launches[0].n_points % X.TILE == 0
    X.forget(case)


def test_patch_hints_to_ignore(oracle_mod, synth_mod):
    _claims(oracle_mod, X.patch_ignored())


# ---- 2. record forms -----------------------------------------------------------------------------------------------------------------------

def test_record_forms(oracle_mod, synth_mod):
    """Every layout holds the packed frames' points: the oracle, fed each layout's own bytes, gives the packed run's rows byte for
    byte (with colour where the layout has an rgb field)."""
    ref = {c: _claims(oracle_mod, X.record_form("packed16"), c) for c in (False, True)}
    assert len(np.unique(ref[True]["rows"]["rgb"])) > 100 and not ref[False]["rows"]["rgb"].any()
    for name, lay in X.LAYOUTS.items():
        case = X.record_form(name)
        offs = [lay[k] for k in ("off_x", "off_y", "off_z", "off_rgb")]
        assert lay["point_step"] % 4 == 0 and all(o % 4 == 0 for o in offs) and max(offs) + 4 <= lay["point_step"], "%s is no valid layout" % name
        for colour in ((False, True) if X.has_rgb(lay) else (False,)):
            run = _claims(oracle_mod, case, colour)
            assert run["rows"].tobytes() == ref[colour]["rows"].tobytes(), "%s, colour %r: the oracle's rows differ from the packed run's" % (name, colour)
        for op, op_ref in zip(case.launches, X.record_form("packed16").launches):
            want = op_ref.packed()
            if not X.has_rgb(lay):
                want[..., 3] = 0
            assert np.array_equal(op.packed(), want), "%s does not hold the packed records" % name
            assert op.n_points % X.TILE != 0 and op.n_points % 2 == 1
    steps = sorted(lay["point_step"] for lay in X.LAYOUTS.values())
    assert steps == [12, 16, 16, 16, 20, 32, 48]
    pad = np.array([X.PAD_WORD], np.uint32).view(np.float32)[0]
    assert np.isfinite(pad) and pad != 0, "the pad word must read as a valid float"


def test_relayout_round_trip():
    rng = np.random.default_rng(1)
    clouds = rng.integers(0, 1 << 32, (3, 37, 4), dtype=np.uint64).astype(np.uint32)
    for name, lay in X.LAYOUTS.items():
        raw = X.relayout(clouds, lay)
        assert raw.shape == (3, 37 * lay["point_step"])
        back = X.Launch(records=raw, layout=lay, poses=np.zeros((3, 3, 4))).packed()
        want = clouds.copy()
        if not X.has_rgb(lay):
            want[..., 3] = 0
        assert np.array_equal(back, want), name
        words = raw.view(np.uint32).reshape(3, 37, -1)
        used = {lay[k] // 4 for k in ("off_x", "off_y", "off_z", "off_rgb")}
        for w in range(words.shape[-1]):
            assert w in used or (words[..., w] == X.PAD_WORD).all(), "%s: word %d" % (name, w)


# ---- 4. depth images -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["u16", "f32"])
@pytest.mark.parametrize("shape", X.DEPTH_SHAPES, ids=["%dx%d" % s for s in X.DEPTH_SHAPES])
def test_depth_cases(oracle_mod, synth_mod, shape, fmt):
    case = X.depth_case(shape[0], shape[1], fmt)
    _claims(oracle_mod, case)
    fr = case.launches[1].frames
    assert fr.depth.dtype == (np.uint16 if fmt == "u16" else np.float32) and fr.depth.shape == (X.DEPTH_FRAMES, shape[1], shape[0])
    for f in range(fr.n):
        assert fr.clouds[f].tobytes() == R.packed_cloud(fr.depth[f], fr.K, fr.rgb[f], R.COLOR_RGB8).tobytes()
    if fmt == "f32" and fr.n_points > 41:
        assert np.isinf(fr.depth).any() and (fr.depth < 0).any() and np.isnan(fr.depth).any()
    # padded rows hold the image, every colour format the same colours
    for dpad, cpad, cf in ((0, 0, R.COLOR_RGB8), (2 if fmt == "u16" else 4, 5, R.COLOR_BGR8), (4, 4, R.COLOR_RGBA8), (8, 8, R.COLOR_BGRA8)):
        d, c, dstep, cstep = X.depth_images(fr, dpad, cpad, cf)
        bpp, cb = fr.depth.dtype.itemsize, (3 if cf in (R.COLOR_RGB8, R.COLOR_BGR8) else 4)
        assert dstep == fr.W * bpp + dpad and cstep == fr.W * cb + cpad
        img = np.ascontiguousarray(d[:, :, :fr.W * bpp]).view(fr.depth.dtype).reshape(fr.depth.shape)
        assert img.tobytes() == fr.depth.tobytes()
        col = np.ascontiguousarray(c[:, :, :fr.W * cb]).reshape(fr.n, fr.H, fr.W, cb)
        for f in range(fr.n):
            assert np.array_equal(R.colors(col[f], cf), fr.clouds[f][:, 3])


# ---- 5. config -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("z_clip", X.Z_CLIPS, ids=["%g_%g" % z for z in X.Z_CLIPS])
def test_z_clip_cases(oracle_mod, synth_mod, z_clip):
    case = X.zclip_case(*z_clip)
    run = _claims(oracle_mod, case)
    vals = X.bound_values(z_clip)
    assert len(vals) == (5 if np.isinf(z_clip[1]) else 3 if z_clip[0] == z_clip[1] else 6)
    for b in z_clip:   # on the bound, and one step either side
        c = np.float32(b)
        assert c in vals and np.nextafter(c, np.float32(-np.inf)) in vals and (np.isinf(c) or np.nextafter(c, np.float32(np.inf)) in vals)
    if z_clip == (0.25, 0.5):
        assert all(float(np.float32(b)) == b for b in z_clip), "both bounds are exact f32 values"
    else:
        assert any(float(np.float32(b)) != b for b in z_clip if np.isfinite(b)), "a bound that is no f32 value"
    for op in case.launches:
        z = op.packed()[..., 2].view(np.float32)
        for v in vals:
            assert ((z == v).sum(axis=1) >= 16).all(), "%r: z = %r is missing from a frame" % (z_clip, v)
    # the strict compares in f64 decide what the oracle counts
    z = np.concatenate([op.packed()[..., 2].view(np.float32).reshape(-1) for op in case.launches]).astype(np.float64)
    assert run["counters"][-1]["zclip_pass"] == int(((z > z_clip[0]) & (z < z_clip[1])).sum())


def test_three_calls(oracle_mod, synth_mod):
    case = X.call_points_case()
    _claims(oracle_mod, case)
    _claims(oracle_mod, case, True)
    sizes = [op.n_points * op.n_frames for op in case.launches]
    assert len(sizes) == 3 and X.largest_call(case) == sizes[1] > sizes[2] > sizes[0] and sizes[1] % 2 == 0
