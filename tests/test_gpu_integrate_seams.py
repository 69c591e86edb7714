"""GPU: k_integrate on the side that faces the caller -- the grid-stride loop and its next-tile prefetch over partial tiles and
frame boundaries, every record form the PointCloud2 contract allows and the bases and strides at which the 16-byte loads must be
refused, the 16 x 16 patch walk and the hints it must ignore, depth images with odd widths, padded rows and one-pixel rows and
columns, and the two hfpf_config fields that reach the kernel or its buffers (z_clip_min / z_clip_max, max_call_points).  The cases
are those of tests/seams.py; tests/test_seam_cases.py asserts on the CPU that each is what it claims to be.

The reference of every case is the oracle with exact moments, fed the same records frame by frame in frame-id order:
scenes.compare_rows_exact behind every clean pass (fourteen columns byte for byte, mean_dist and sd_dist within its derived bounds;
no tolerance of this file's own), the occupied list as a set, and points_presented, points_zclip_pass, points_in_bbox,
points_buffered, voxels_occupied and voxels_with_normal behind every call.  Where a case is the same cloud presented another way --
another record form, base, stride, entry point, frame order in memory, frame_width, max_call_points -- the rows and the contract
counters must also be those of the first presentation, byte for byte.  The test cannot see which point form the host picked; it
asserts the result only.

The tile-count assumption of the many-tile cases (seams.MANY_TILES): MI355X has 256 CUs and a CU holds at most 8 workgroups of 256
threads, so a launch has at most 2048 workgroups and in a call of 8192 tiles each workgroup walks four or more.

Layout rejections (a step or an offset that is no multiple of 4, an offset + 4 beyond point_step): test_gpu_edge.py holds ONE
combined case of hfpf_integrate (step 18 with odd offsets); the separate conditions, and the device form's base and stride, are
here."""
import time

import numpy as np
import pytest

import depth_ref as R
import gpu_support as G
import query_ref as Q
import scenes
import seams as X
import track_ref as TR

pytestmark = pytest.mark.gpu

CAPS = dict(max_bricks=60000, max_log_points=8 << 20, max_normals=1 << 20, max_frames=4096)
ORACLE_COUNTERS = (("presented", "points_presented"), ("zclip_pass", "points_zclip_pass"), ("inserted", "points_in_bbox"),
                   ("buffered", "points_buffered"), ("occupied", "voxels_occupied"), ("normals", "voxels_with_normal"))
FILL = 0xA5   # every byte of a buffer that is no frame


@pytest.fixture(scope="module", autouse=True)
def _file_time():
    """When the file's first test began (test_file_time, the last one, prints what the file took); drops the cases and oracle runs
    the file built."""
    yield time.perf_counter()
    X.forget_all()
    _first.clear()


# ---- presentations: one integrate call (or one per frame) for a seams.Launch ------------------------------------------------------------

def _pick(op, order):
    """(packed records, poses) of the launch with its frames in `order` in memory."""
    clouds, poses = op.packed(), op.poses
    return (clouds, poses) if order is None else (clouds[order], poses[order])


def _raw(op, layout, order):
    """(bytes (n_frames, n_points * step), layout, poses): the launch's own records, or its points laid out in `layout`."""
    if layout is None:
        raw = np.stack(op.records)
        return (raw if order is None else raw[order]), op.layout, (op.poses if order is None else op.poses[order])
    clouds, poses = _pick(op, order)
    return X.relayout(clouds, layout), layout, poses


def cloud_device(layout=None, base_off=0, stride_pad=0):
    """hfpf_integrate_device: the frames base_off bytes into an allocation, stride_pad bytes between them."""
    def present(g, op, order=None, ids=None):
        raw, lay, poses = _raw(op, layout, order)
        stride = raw.shape[1] + stride_pad
        buf = np.full(base_off + op.n_frames * stride + 64, FILL, np.uint8)
        buf[base_off:base_off + op.n_frames * stride].reshape(op.n_frames, stride)[:, :raw.shape[1]] = raw
        with G.uploaded(g, buf) as (dev,):
            g.integrate_device(dev + base_off, op.n_frames, stride, op.n_points, poses, frame_ids=ids, **lay)
            g.sync()
    return present


def cloud_host(layout=None, pinned=False):
    """hfpf_integrate / hfpf_integrate_pinned, frame by frame."""
    def present(g, op, order=None, ids=None):
        assert order is None and ids is None
        raw, lay, poses = _raw(op, layout, None)
        bufs = []
        for f in range(op.n_frames):
            if pinned:
                b = g.host_alloc(raw.shape[1])
                b[:] = raw[f]
                bufs.append(b)
                g.integrate_pinned(b, poses[f], n_points=op.n_points, **lay)
            else:
                g.integrate(raw[f], poses[f], n_points=op.n_points, **lay)
        for b in bufs:
            g.host_free(b)   # (waits for the frames that read it)
    return present


def _image_views(fr, d, c, f, color_format):
    bpp, cb = fr.depth.dtype.itemsize, R_BPP[color_format]
    depth = np.ndarray((fr.H, fr.W), fr.depth.dtype, buffer=d[f], strides=(d.shape[2], bpp))
    color = np.ndarray((fr.H, fr.W, cb), np.uint8, buffer=c[f], strides=(c.shape[2], cb, 1))
    return depth, color


R_BPP = {R.COLOR_RGB8: 3, R.COLOR_BGR8: 3, R.COLOR_RGBA8: 4, R.COLOR_BGRA8: 4}


def depth_host(depth_pad=0, color_pad=0, color_format=R.COLOR_RGB8, pinned=False):
    """hfpf_integrate_depth / _pinned, frame by frame, rows padded by depth_pad and color_pad bytes."""
    def present(g, op, order=None, ids=None):
        assert order is None and ids is None
        fr = op.frames
        d, c, _, _ = X.depth_images(fr, depth_pad, color_pad, color_format, FILL)
        bufs = []
        if pinned:
            pd, pc = g.host_alloc(d.nbytes), g.host_alloc(c.nbytes)
            pd[:], pc[:] = d.reshape(-1), c.reshape(-1)
            bufs, d, c = [pd, pc], pd.reshape(d.shape), pc.reshape(c.shape)
        for f in range(fr.n):
            depth, color = _image_views(fr, d, c, f, color_format)
            (g.integrate_depth_pinned if pinned else g.integrate_depth)(depth, fr.poses[f], fr.K, color=color, color_format=color_format)
        for b in bufs:
            g.host_free(b)
    return present


def depth_device(hfpf_mod, depth_pad=0, color_pad=0, color_format=R.COLOR_RGB8, depth_stride_pad=0, color_stride_pad=0):
    """hfpf_integrate_depth_device: padded rows, and depth_stride_pad / color_stride_pad bytes between the frames."""
    def present(g, op, order=None, ids=None):
        fr = op.frames
        d, c, dstep, cstep = X.depth_images(fr, depth_pad, color_pad, color_format, FILL)
        poses = fr.poses
        if order is not None:
            d, c, poses = d[order], c[order], poses[order]
        dstride, cstride = fr.H * dstep + depth_stride_pad, fr.H * cstep + color_stride_pad
        bd, bc = np.full(fr.n * dstride + 64, FILL, np.uint8), np.full(fr.n * cstride + 64, FILL, np.uint8)
        bd[:fr.n * dstride].reshape(fr.n, dstride)[:, :fr.H * dstep] = d.reshape(fr.n, -1)
        bc[:fr.n * cstride].reshape(fr.n, cstride)[:, :fr.H * cstep] = c.reshape(fr.n, -1)
        fmt = hfpf_mod.DEPTH_U16 if fr.depth.dtype == np.uint16 else hfpf_mod.DEPTH_F32
        desc = hfpf_mod.depth_desc(fr.W, fr.H, fmt, dstep, fr.K, color_format, cstep)
        with G.uploaded(g, bd, bc) as (dd, dc):
            g.integrate_depth_device(desc, dd, dstride, fr.n, poses, dev_color=dc, color_frame_stride=cstride, frame_ids=ids)
            g.sync()
    return present


# ---- sessions and their comparison ---------------------------------------------------------------------------------------------------------

def _session(hfpf_mod, case, present, colour=False, shuffled=None, **kw):
    """The case's schedule on a fresh handle: dict of counters (behind every op), snaps ((rows, occupied) behind every clean pass)
    and the contract counters at the end.  shuffled: seams.shuffled_ids(case), per launch (order in memory, explicit ids)."""
    caps = dict(CAPS, **case.caps)
    with hfpf_mod.OccupancyGrid(resolution=case.resolution, bbox=X.BBOX, z_clip=case.z_clip, fuse_color=colour, **caps, **kw) as g:
        out = dict(counters=[], snaps=[])
        k = 0
        for op in case.ops:
            if op is X.CLEAN:
                g.clean()
                out["snaps"].append((g.extract().copy(), g.occupied().copy()))
            else:
                present(g, op, *(shuffled[k] if shuffled else ()))
                k += 1
            out["counters"].append(g.counters())
        out["contract"] = G.contract_counters(g)
    return out


_first = {}   # (case, colour) -> (what, rows, contract) of the first presentation


def _check(oracle_mod, case, run, what, colour=False):
    ref = X.oracle_run(oracle_mod, case, colour)
    what = "%s, %s%s" % (case.name, what, ", colour" if colour else "")
    assert len(run["snaps"]) == len(ref["snaps"])
    for k, ((rows, occ), (rrows, rocc)) in enumerate(zip(run["snaps"], ref["snaps"])):
        print("%s, clean pass %d:" % (what, k), end=" ")
        rep = scenes.compare_rows_exact(rrows, rows)
        assert rep["exact_bytes_differing"] == 0
        assert np.array_equal(X.occupied_keys(occ), X.occupied_keys(rocc)), "%s: occupied sets differ behind clean pass %d" % (what, k)
    for i, (c_ref, c) in enumerate(zip(ref["counters"], run["counters"])):
        for a, b in ORACLE_COUNTERS:
            assert c_ref[a] == c[b], "%s: behind op %d: %s %d, the oracle's %s %d" % (what, i, b, c[b], a, c_ref[a])
    members = int(ref["rows"]["count"].astype(np.int64).sum())
    got = run["contract"]["dep_pairs_member"] + run["contract"]["replay_members"]
    assert got == members, "%s: %d members, the oracle's rows count %d" % (what, got, members)
    if colour and len(ref["rows"]) > 1000:
        assert len(np.unique(run["snaps"][-1][0]["rgb"])) > 100, "%s: no colours" % what
    first = _first.setdefault((case.name, colour), (what, run["snaps"][-1][0], run["contract"]))
    assert first[1].tobytes() == run["snaps"][-1][0].tobytes(), "%s: rows differ from those of: %s" % (what, first[0])
    assert first[2] == run["contract"], "%s: contract counters %r; %r of: %s" % (what, run["contract"], first[2], first[0])


def _go(hfpf_mod, oracle_mod, case, present, what, colour=False, **kw):
    _check(oracle_mod, case, _session(hfpf_mod, case, present, colour, **kw), what, colour)


# ---- 1. tile loop ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_pts", list(X.SINGLE_SHAPES))
def test_single_frames(hfpf_mod, oracle_mod, synth_mod, n_pts):
    """One frame of n_pts points behind the first clean pass of the base model: packed, strided and depth forms through the host,
    the pinned and the device entry points."""
    case = X.single_frame(n_pts)
    H = hfpf_mod
    for what, present in (("packed, host", cloud_host()), ("packed, pinned", cloud_host(pinned=True)), ("packed, device", cloud_device()),
                          ("strided, host", cloud_host(X.PCL32)), ("strided, pinned", cloud_host(X.PCL32, pinned=True)),
                          ("strided, device", cloud_device(X.PCL32)), ("depth, host", depth_host()), ("depth, pinned", depth_host(pinned=True)),
                          ("depth, device", depth_device(H))):
        _go(H, oracle_mod, case, present, what)


MANY_VARIANTS = {
    # name -> (presentations, colour, engine keywords, shuffled ids)
    "forms": (("packed", "strided", "depth"), False, {}, False),
    "ids": (("packed", "strided", "depth"), False, {}, True),
    "strides": (("packed +48", "packed +4", "strided +36", "depth +6 +7"), False, {}, False),
    "unbinned": (("packed", "strided", "depth"), False, dict(binned_update=False), False),
    "colour": (("packed", "strided", "depth"), True, {}, False),
}


def _many_presentation(hfpf_mod, name):
    return {"packed": lambda: cloud_device(), "strided": lambda: cloud_device(X.PCL32), "depth": lambda: depth_device(hfpf_mod),
            "packed +48": lambda: cloud_device(stride_pad=48),        # padding between the frames, still 16-byte records on 16-byte frames
            "packed +4": lambda: cloud_device(stride_pad=4),          # frames at 4, 8, 12, 0 (mod 16): the 16-byte loads must be refused
            "strided +36": lambda: cloud_device(X.PCL32, stride_pad=36),
            "depth +6 +7": lambda: depth_device(hfpf_mod, depth_stride_pad=6, color_stride_pad=7)}[name]()


@pytest.mark.parametrize("variant", list(MANY_VARIANTS))
@pytest.mark.parametrize("shape", list(X.MANY_SHAPES))
def test_many_tiles(hfpf_mod, oracle_mod, synth_mod, shape, variant):
    """Two hfpf_integrate_device calls of at least 8192 tiles whose frames end in a partial tile (272 points: a frame boundary and a
    16-lane tail every second tile; 32769 points: a one-lane tail), the session's first call and a second behind a clean pass.  At
    most 2048 workgroups run (256 CUs x 8 workgroups of 256 threads), so each walks four tiles or more: the prefetch guard
    pre_i < n_pts, a prefetch that crosses into the next frame behind a partial tile, and a stale `pre` behind a skipped load."""
    case = X.many_tiles(shape)
    names, colour, kw, shuffle = MANY_VARIANTS[variant]
    for op in case.launches:
        assert op.tiles >= X.MANY_TILES >= 4 * X.INTEGRATE_GRID_MAX and op.n_points % X.TILE
    for name in names:
        _go(hfpf_mod, oracle_mod, case, _many_presentation(hfpf_mod, name), "%s (%s)" % (name, variant), colour,
            shuffled=X.shuffled_ids(case) if shuffle else None, **kw)


# ---- 2. record forms -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(X.LAYOUTS))
def test_record_forms(hfpf_mod, oracle_mod, synth_mod, name):
    """Every layout of seams.LAYOUTS as hfpf_synth.frame writes it, through hfpf_integrate and hfpf_integrate_device, with and
    without colour where the layout has an rgb field; the rows are those of the packed records."""
    case, lay = X.record_form(name), X.LAYOUTS[name]
    for colour in ((False, True) if X.has_rgb(lay) else (False,)):
        ref = X.oracle_run(oracle_mod, X.record_form("packed16"), colour)
        for what, present in (("host", cloud_host()), ("device", cloud_device()), ("device, frames +12", cloud_device(stride_pad=12))):
            run = _session(hfpf_mod, case, present, colour)
            _check(oracle_mod, case, run, what, colour)
            rep = scenes.compare_rows_exact(ref["rows"], run["snaps"][-1][0])
            assert rep["exact_bytes_differing"] == 0, "%s: not the rows of the packed records" % name


@pytest.mark.parametrize("colour", [False, True])
def test_packed_records_off_the_16_byte_grid(hfpf_mod, oracle_mod, synth_mod, colour):
    """Packed 16-byte records at +4, +8 and +12 bytes inside a larger allocation, and at an aligned base with a frame stride of
    4 (mod 16): byte-identical to the aligned run (the first presentation)."""
    case = X.record_form("packed16")
    _go(hfpf_mod, oracle_mod, case, cloud_device(), "aligned", colour)
    for off in (4, 8, 12):
        _go(hfpf_mod, oracle_mod, case, cloud_device(base_off=off), "base +%d" % off, colour)
        _go(hfpf_mod, oracle_mod, case, cloud_device(base_off=off, stride_pad=16 - off), "base +%d, frames +%d" % (off, 16 - off), colour)
    for pad in (4, 8, 12, 20):
        _go(hfpf_mod, oracle_mod, case, cloud_device(stride_pad=pad), "frames +%d" % pad, colour)


@pytest.fixture(scope="module")
def layout_model(hfpf_mod, synth_mod):
    """The record-form scene fused with colour, kept open for track and query."""
    case = X.record_form("packed16")
    g = hfpf_mod.OccupancyGrid(resolution=case.resolution, bbox=X.BBOX, fuse_color=True, **CAPS)
    for op in case.ops:
        if op is X.CLEAN:
            g.clean()
        else:
            cloud_device()(g, op)
    rows, occ = g.extract().copy(), g.occupied().copy()
    assert case.resolution == G.RES and X.Z_CLIP == G.Z_CLIP and X.BBOX == G.BBOX
    yield g, rows, occ
    g.close()


def test_track_and_query_read_every_layout(hfpf_mod, synth_mod, layout_model):
    """hfpf_track, hfpf_query and hfpf_query_device share PointLayout<FORM> and load_point with integrate: a held-out frame in every
    layout, and as packed records off the 16-byte grid, against track_ref and query_ref as test_gpu_track.py and test_gpu_query.py
    compare them."""
    g, rows, occ = layout_model
    W, H = X.LAYOUT_SHAPE
    K = (X.FX, X.FX, W / 2.0 - 0.5, H / 2.0 - 0.5)
    packed, true = X.held_out_records()
    xyz = np.ascontiguousarray(packed.view(np.float32).reshape(-1, 4)[:, :3])
    guess = G.perturb(true, 1.0, (0.003, -0.002, 0.003))
    opts = dict(G.TRACK_OPTS, max_iterations=4)
    t_ref = G.track_reference(rows, TR.cloud_points(xyz, 1), guess, K, W, H, max_iterations=4)
    kw = dict(radius=2, min_count=1.0, zclip=True)
    q_ref = Q.query(rows, occ, xyz, true, tuple(g.cfg.bbox), g.dims[1], G.Z_CLIP, radius=2, min_count=1.0, zclip=True)
    assert t_ref["inliers"] > 1000 and (q_ref[0]["flags"] & Q.FOUND != 0).sum() > 1000
    for name, lay in X.LAYOUTS.items():
        rec, pose = X.held_out_records(lay)
        assert pose.tobytes() == true.tobytes()
        G.same_track(g.track(rec, lay, guess, K, W, H, **opts), t_ref, "track, %s" % name)
        G.same_query(g.query(rec, true, layout=lay, **kw), q_ref, "query, %s" % name)
        for off in (0, 4, 8, 12):
            buf = np.full(off + len(rec) + 64, FILL, np.uint8)
            buf[off:off + len(rec)] = rec
            with G.uploaded(g, buf) as (dev,):
                G.same_query(g.query_device(dev + off, len(xyz), true, layout=lay, **kw), q_ref, "query_device, %s at +%d" % (name, off))


def test_layouts_are_refused_and_the_handle_stays_usable(hfpf_mod, oracle_mod, synth_mod):
    """HFPF_ERR_BAD_ARG for a step or an offset that is no multiple of 4 and for an offset + 4 beyond point_step (host and device
    forms), and for a device base or frame stride off the 4-byte grid; the session between the refusals is the aligned one."""
    case = X.record_form("packed16")
    L = hfpf_mod.lib()
    bad = {"step 18": (18, 0, 4, 8, 12), "step 14": (14, 0, 4, 8, 8), "off_x 2": (16, 2, 4, 8, 12), "off_y 6": (16, 0, 6, 8, 12),
           "off_z 9": (16, 0, 4, 9, 12), "off_rgb 14": (20, 0, 4, 8, 14), "off_x + 4 beyond": (16, 16, 4, 8, 12),
           "off_z + 4 beyond": (12, 0, 4, 12, 0), "off_rgb + 4 beyond": (16, 0, 4, 8, 16), "off_y + 4 beyond step 8": (8, 0, 8, 4, 0)}

    def refusals(g, op):
        raw = np.stack(op.records)
        pose = np.ascontiguousarray(op.poses[0], np.float64).reshape(12)
        before = g.counters()
        with G.uploaded(g, raw) as (dev,):
            for what, (step, ox, oy, oz, orgb) in bad.items():
                assert L.hfpf_integrate(g._h, raw.ctypes.data, 100, step, ox, oy, oz, orgb, pose.ctypes.data) == -2, what
                assert L.hfpf_integrate_device(g._h, dev, 1, 100 * 48, 100, step, ox, oy, oz, orgb, pose.ctypes.data, None) == -2, what
            assert L.hfpf_integrate_device(g._h, dev + 2, 1, 1600, 100, 16, 0, 4, 8, 12, pose.ctypes.data, None) == -2, "base + 2"
            assert L.hfpf_integrate_device(g._h, dev, 2, 1602, 100, 16, 0, 4, 8, 12, np.tile(pose, 2).ctypes.data, None) == -2, "stride 1602"
        assert g.counters() == before, "a refused call changed the counters"

    def present(g, op, order=None, ids=None):
        refusals(g, op)
        cloud_device()(g, op)
        refusals(g, op)

    for colour in (False, True):
        _go(hfpf_mod, oracle_mod, case, present, "between refused calls", colour)


# ---- 3. patch walk -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", list(X.PATCH_SHAPES))
def test_patch_walk(hfpf_mod, oracle_mod, synth_mod, width):
    """frame_width = the frames' width in a call of at least 8192 tiles: byte-identical to frame_width = 0, exact against the oracle."""
    case = X.patch_walk(width)
    assert X.tile_row_width(width, case.launches[0].n_points) == width and case.launches[0].tiles >= X.MANY_TILES
    for fw in (0, width):
        _go(hfpf_mod, oracle_mod, case, cloud_device(), "packed, frame_width %d" % fw, frame_width=fw)
        _go(hfpf_mod, oracle_mod, case, cloud_device(X.PCL32), "strided, frame_width %d" % fw, frame_width=fw)
    if width == 48:   # (one oracle run with colour is enough: the walk does not depend on it)
        _go(hfpf_mod, oracle_mod, case, cloud_device(), "packed, frame_width %d" % width, True, frame_width=width)
    X.forget(case)


def test_patch_hints_that_change_nothing(hfpf_mod, oracle_mod, synth_mod):
    """48 x 24 frames: rows that are no multiple of 16, a width that does not divide n_points, a width below 16, above n_points, and
    one that is no multiple of 16."""
    case = X.patch_ignored()
    for fw in (0,) + X.IGNORED_HINTS:
        assert fw == 0 or X.tile_row_width(fw, case.launches[0].n_points) == 0
        _go(hfpf_mod, oracle_mod, case, cloud_device(), "packed, frame_width %d" % fw, frame_width=fw)
    _go(hfpf_mod, oracle_mod, case, cloud_device(X.PCL32), "strided, frame_width 48", frame_width=48)
    _go(hfpf_mod, oracle_mod, case, cloud_host(), "host, frame_width 24", frame_width=24)


# ---- 4. depth images -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["u16", "f32"])
@pytest.mark.parametrize("shape", X.DEPTH_SHAPES, ids=["%dx%d" % s for s in X.DEPTH_SHAPES])
def test_depth_images(hfpf_mod, oracle_mod, synth_mod, shape, fmt):
    """Depth + colour images of one pixel, one-pixel rows, one-pixel columns and odd widths, u16 and f32, through the host, the pinned
    and the device entry points: rows of exactly the width and padded by 2, 4 and 6 bytes (u16 depth and 3-byte colours; a step
    must be a multiple of a 4-byte sample, so f32 depth rows are padded by 4, 8 and 12 and 4-byte colour rows by 4 and 8), device
    frames at strides that are multiples of the sample size and not of 16.  The first presentation is the equivalent cloud."""
    case = X.depth_case(shape[0], shape[1], fmt)
    H = hfpf_mod
    W, Hh = shape
    _go(H, oracle_mod, case, cloud_device(), "the equivalent cloud", True)
    dpads = (0, 2, 4, 6) if fmt == "u16" else (0, 4, 8, 12)
    formats = (R.COLOR_RGB8, R.COLOR_BGRA8, R.COLOR_BGR8, R.COLOR_RGBA8)
    bpp = 2 if fmt == "u16" else 4
    for i, dpad in enumerate(dpads):
        cf = formats[i]
        cpad = (0, 2, 4, 6)[i] if R_BPP[cf] == 3 else (0, 4, 4, 8)[i]
        what = "rows +%d / +%d, colour format %d" % (dpad, cpad, cf)
        _go(H, oracle_mod, case, depth_host(dpad, cpad, cf), "host, " + what, True)
        _go(H, oracle_mod, case, depth_host(dpad, cpad, cf, pinned=True), "pinned, " + what, True)
        # a frame stride that is a multiple of the sample size and no multiple of 16
        dsp = next(p for p in range(bpp, 64, bpp) if (Hh * (W * bpp + dpad) + p) % 16)
        csp = next(p for p in range(1 if R_BPP[cf] == 3 else 4, 64, 1 if R_BPP[cf] == 3 else 4) if (Hh * (W * R_BPP[cf] + cpad) + p) % 16)
        _go(H, oracle_mod, case, depth_device(H, dpad, cpad, cf), "device, " + what, True)
        _go(H, oracle_mod, case, depth_device(H, dpad, cpad, cf, dsp, csp), "device, frames +%d / +%d, %s" % (dsp, csp, what), True)
    _go(H, oracle_mod, case, depth_device(H), "device, colourless session", False)


# ---- 5. config -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("z_clip", X.Z_CLIPS, ids=["%g_%g" % z for z in X.Z_CLIPS])
def test_z_clip(hfpf_mod, oracle_mod, synth_mod, z_clip):
    """z_clip_min / z_clip_max: points exactly on each bound and one f32 step either side, through hfpf_probe_points (flag bit 0
    against z > min and z < max in f64) and through integrate against the oracle with the same interval."""
    case = X.zclip_case(*z_clip)
    lo, hi = z_clip
    rng = np.random.default_rng(0x2C)
    z = np.concatenate([X.bound_values(z_clip), np.float32([0.0, -0.0, np.nan, np.inf, -np.inf, 0.28, 0.6, 0.3, 0.45]),
                        rng.uniform(-1.5, 1.5, 4096).astype(np.float32)]).astype(np.float32)
    xyz = np.stack([np.zeros_like(z), np.zeros_like(z), z], axis=1)
    with hfpf_mod.OccupancyGrid(resolution=case.resolution, bbox=X.BBOX, z_clip=z_clip, **CAPS) as g:
        _, _, flags = g.probe_points(np.eye(4)[:3], xyz)
    z64 = z.astype(np.float64)
    with np.errstate(invalid="ignore"):
        want = (z64 > lo) & (z64 < hi)
    bad = np.flatnonzero(((flags & 1) != 0) != want)
    assert bad.size == 0, "z_clip %r: %d flags differ, first z = %r: %d" % (z_clip, bad.size, z[bad[0]], flags[bad[0]])
    assert case.kind == "empty" or 0 < want.sum() < len(want)
    for what, present in (("packed, device", cloud_device()), ("strided, device", cloud_device(X.PCL32)), ("packed, host", cloud_host()),
                          ("strided, host", cloud_host(X.LAYOUTS["tail48"]))):
        run = _session(hfpf_mod, case, present)
        _check(oracle_mod, case, run, what)
        if case.kind == "empty":
            assert len(run["snaps"][-1][0]) == 0 and run["counters"][-1]["points_zclip_pass"] == 0 and run["counters"][-1]["points_presented"] > 0
    _go(hfpf_mod, oracle_mod, case, cloud_device(), "packed, device", True)


@pytest.mark.parametrize("colour", [False, True])
def test_max_call_points(hfpf_mod, oracle_mod, synth_mod, colour):
    """max_call_points = 0 (bins grown on demand), half of, exactly and twice the largest call of a three-call session: rows, occupied
    list and result counters byte-identical across the four, exact against the oracle."""
    case = X.call_points_case()
    largest = X.largest_call(case)
    for mcp in (0, largest // 2, largest, 2 * largest):
        _go(hfpf_mod, oracle_mod, case, cloud_device(), "max_call_points %d" % mcp, colour, max_call_points=mcp)
    _go(hfpf_mod, oracle_mod, case, cloud_device(X.PCL32), "strided, max_call_points %d" % largest, colour, max_call_points=largest)
    _go(hfpf_mod, oracle_mod, case, cloud_device(), "packed, un-binned, max_call_points %d" % largest, colour, max_call_points=largest,
        binned_update=False)


# ---- the file's time (the last test) ---------------------------------------------------------------------------------------------------

def test_file_time(_file_time, capsys):
    """Prints what the tests of this file took together, past the capture.  The file is meant to stay well under a minute."""
    with capsys.disabled():
        print("\ntest_gpu_integrate_seams.py: %.1f s" % (time.perf_counter() - _file_time))
