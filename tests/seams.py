"""The seams of k_integrate that face the caller (imported by tests only): how many points a frame has, how many tiles a call has,
where the records lie in memory, which of the three point forms the host picks, and the two hfpf_config fields that reach the kernel
or its buffers (z_clip_min / z_clip_max, max_call_points).  This module holds the case table and the builders; it defines no test
and no fixture.  tests/test_seam_cases.py asserts on the CPU, from the oracle alone, that every case is what it claims to be;
tests/test_gpu_integrate_seams.py runs every case on the engine against the oracle's exact rows.

A case is a schedule of LAUNCHES (one integrate call each: frames of one shape, their poses and, in one variant, explicit frame ids)
and clean passes.  The frames are small views of the synthetic scene of hfpf_synth (fx = 615: a pixel is 0.7 mm wide on the
surfaces, so a 17 x 16 frame covers a patch of about 12 x 12 voxels of 1 mm) from cameras that orbit the scene's centre by a few
degrees and centimetres (wider in the many-tile cases: WIDE_ORBIT), so that thousands of small frames lay a dense model of ten to a
hundred thousand voxels.  One pixel in ten has no reading (HOLES), so that no case passes more than 95 % of its points through both
clips.

Frames rendered as DEPTH images carry three presentations of the same points: the image itself, the packed 16-byte cloud
tests/depth_ref.py defines it to be, and that cloud laid out in any other record form (relayout; the bytes between the fields are
filled with a pattern that is a small valid float, so that a load from the wrong place changes the result).  All of them must give
the same bytes, and one oracle run -- fed the packed cloud frame by frame, in frame-id order -- serves them all.

The tile-count assumption.  A launch of k_integrate has min(n_tiles, integrate_grid) workgroups, integrate_grid = workgroups per CU
x CUs.  MI355X has 256 CUs and a CU holds at most 8 workgroups of 256 threads (2048 threads = 32 waves of 64), so integrate_grid is
at most INTEGRATE_GRID_MAX = 2048, and in a call of MANY_TILES = 8192 tiles or more every workgroup walks at least four tiles: the
grid-stride loop and its next-tile prefetch run, whatever the occupancy the compiler reached."""
import time

import numpy as np

import depth_ref as R
import hfpf_synth as S
import scenes

BBOX = scenes.BBOX_1M
FX = 615.0
HOLES = 100                 # per mille of pixels without a reading
Z_CLIP = (0.28, 0.6)        # the handle's default (node.cpp:92-93)
TILE = 256                  # points of one tile of k_integrate
INTEGRATE_GRID_MAX = 2048   # 256 CUs x 8 workgroups of 256 threads
MANY_TILES = 4 * INTEGRATE_GRID_MAX
MIN_ROWS, MIN_ROWS_BASE = 1000, 200
PAD_WORD = 0xA5A5A5A5       # as a float -2.9e-16: read as x or y it moves a point, read as z it fails the z-clip
SEED, POSE_SEED = 0x5EA3, 0x5E3
CLEAN = "clean"

PACKED16 = dict(S.LAYOUT_PACKED16)
PCL32 = dict(S.LAYOUT_PCL32)


def tiles(n_points, n_frames=1):
    return (n_points + TILE - 1) // TILE * n_frames


# csrc/host_plan.hpp, the body of tile_row_width (test_seam_cases.py reads it again out of the text), and its restatement
TILE_ROW_WIDTH_RULE = "(fw >= 16 && fw % 16 == 0 && n_points % fw == 0 && (n_points / fw) % 16 == 0) ? fw : 0u"


def tile_row_width(fw, n_points):
    """The row width of the 16 x 16 patch walk, or 0: the linear walk."""
    return fw if fw >= 16 and fw % 16 == 0 and n_points % fw == 0 and (n_points // fw) % 16 == 0 else 0


# ---- frames ----------------------------------------------------------------------------------------------------------------------------

def as_f32(depth_u16):
    """A uint16 depth image in metres as f32: no reading = NaN, and a sprinkle of the values a driver can deliver instead (inf, a
    negative depth) on a fixed lattice of pixels."""
    d = depth_u16.astype(np.float32) * np.float32(0.001)
    d[depth_u16 == 0] = np.nan
    flat = d.reshape(-1)
    flat[5::37] = np.inf
    flat[11::41] = -0.4
    return d


class Frames:
    """n frames of W x H pixels: frame f is the synthetic scene seen from pose(POSE_SEED, first + f).  depth = "u16" | "f32": rendered
    as depth + RGB8 images (self.depth (n, H, W), self.rgb (n, H, W, 3), self.K) and self.clouds = the packed clouds depth_ref makes of
    them; depth = None: rendered as packed clouds directly (hfpf_synth.frame).  self.clouds: (n, W * H, 4) uint32."""

    def __init__(self, n, W, H, first=0, depth="u16", max_angle=10.0, jitter=0.02, holes=HOLES):
        self.n, self.W, self.H, self.first, self.fmt = n, W, H, first, depth
        self.n_points = W * H
        self.poses = np.stack([S.pose(POSE_SEED, first + f, max_angle, jitter) for f in range(n)])
        if depth is None:
            self.depth = self.rgb = self.K = None
            self.clouds = np.stack([S.frame(SEED, first + f, W, H, self.poses[f], fx=FX, nan_permille=holes).view(np.uint32).reshape(-1, 4)
                                    for f in range(n)])
        else:
            fr = [S.depth_frame(SEED, first + f, W, H, self.poses[f], fx=FX, nan_permille=holes) for f in range(n)]
            self.K = fr[0][2]
            self.depth = np.stack([d for d, _, _ in fr])
            self.rgb = np.stack([c for _, c, _ in fr])
            if depth == "f32":
                self.depth = np.stack([as_f32(d) for d in self.depth])
            self.clouds = np.stack([R.packed_cloud(self.depth[f], self.K, self.rgb[f], R.COLOR_RGB8).view(np.uint32).reshape(-1, 4)
                                    for f in range(n)])
        for a in (self.clouds, self.poses, self.depth, self.rgb):
            if a is not None:
                a.setflags(write=False)


def relayout(clouds, layout, pad_word=PAD_WORD):
    """Packed records (..., n, 4) uint32 -> the same records in `layout`, (..., n * point_step) uint8; every byte outside the four
    fields holds PAD_WORD's.  A layout without room for rgb (off_rgb naming another field) drops the colour."""
    clouds = np.asarray(clouds, np.uint32)
    words = layout["point_step"] // 4
    out = np.full(clouds.shape[:-1] + (words,), pad_word, np.uint32)
    out[..., layout["off_rgb"] // 4] = clouds[..., 3]     # first: x, y or z overwrite it where the layout has no rgb field
    for k, name in enumerate(("off_x", "off_y", "off_z")):
        out[..., layout[name] // 4] = clouds[..., k]
    return out.view(np.uint8).reshape(clouds.shape[:-2] + (clouds.shape[-2] * layout["point_step"],))


def has_rgb(layout):
    return layout["off_rgb"] not in (layout["off_x"], layout["off_y"], layout["off_z"])


def depth_images(fr, depth_pad=0, color_pad=0, color_format=R.COLOR_RGB8, fill=0xA5):
    """The frames' images with padded rows: (depth (n, H, depth_step) uint8, colour (n, H, color_step) uint8, depth_step, color_step).
    The pad bytes hold `fill`.  color_format: RGB8, BGR8, RGBA8 or BGRA8 of depth_ref (alpha = 0x5A)."""
    bpp = fr.depth.dtype.itemsize
    dstep = fr.W * bpp + depth_pad
    d = np.full((fr.n, fr.H, dstep), fill, np.uint8)
    d[:, :, :fr.W * bpp] = np.ascontiguousarray(fr.depth).view(np.uint8).reshape(fr.n, fr.H, fr.W * bpp)
    c = fr.rgb if color_format in (R.COLOR_RGB8, R.COLOR_RGBA8) else fr.rgb[..., ::-1]
    if color_format in (R.COLOR_RGBA8, R.COLOR_BGRA8):
        c = np.concatenate([c, np.full(c.shape[:-1] + (1,), 0x5A, np.uint8)], axis=-1)
    cb = c.shape[-1]
    cstep = fr.W * cb + color_pad
    col = np.full((fr.n, fr.H, cstep), fill, np.uint8)
    col[:, :, :fr.W * cb] = np.ascontiguousarray(c).reshape(fr.n, fr.H, fr.W * cb)
    return d, col, dstep, cstep


# ---- launches and cases ----------------------------------------------------------------------------------------------------------------

class Launch:
    """One integrate call.  frames: a Frames (records = its packed clouds) or, with `records`, per-frame byte arrays in `layout` as the
    oracle is to read them.  ids: explicit frame ids or None (the engine numbers the frames of a session as they arrive)."""

    def __init__(self, frames=None, records=None, layout=None, poses=None, ids=None, tag=""):
        self.frames, self.tag = frames, tag
        self.layout = dict(layout or PACKED16)
        if records is None:
            records = frames.clouds.view(np.uint8).reshape(frames.n, -1)
            poses = frames.poses
        self.records = [np.ascontiguousarray(r).view(np.uint8).reshape(-1) for r in records]
        self.poses = np.asarray(poses, np.float64).reshape(len(self.records), 3, 4)
        self.ids = None if ids is None else [int(i) for i in ids]
        assert len({len(r) for r in self.records}) == 1 and len(self.records[0]) % self.layout["point_step"] == 0
        assert self.ids is None or len(self.ids) == len(self.records)

    @property
    def n_frames(self):
        return len(self.records)

    @property
    def n_points(self):
        return len(self.records[0]) // self.layout["point_step"]

    @property
    def tiles(self):
        return tiles(self.n_points, self.n_frames)

    def oracle_order(self):
        """The frames as a sequential capture takes them: by frame id (the smallest id that touched a cell is its viewpoint)."""
        return range(self.n_frames) if self.ids is None else np.argsort(self.ids, kind="stable")

    def packed(self):
        """(n_frames, n_points, 4) uint32: the records as packed x, y, z, rgb (rgb = 0 where the layout has none)."""
        lay, w = self.layout, self.layout["point_step"] // 4
        rec = np.stack(self.records).view(np.uint32).reshape(self.n_frames, self.n_points, w)
        out = np.stack([rec[..., lay["off_x"] // 4], rec[..., lay["off_y"] // 4], rec[..., lay["off_z"] // 4],
                        rec[..., lay["off_rgb"] // 4] if has_rgb(lay) else np.zeros(rec.shape[:2], np.uint32)], axis=-1)
        return np.ascontiguousarray(out)


class Case:
    """ops: Launch | CLEAN.  kind: "rows" (claims MIN_ROWS rows with members), "base" (a small base model: MIN_ROWS_BASE) or "empty"
    (claims that nothing passes).  many: indices of the launches that claim MANY_TILES tiles.  partial: those launches' frames also
    end in a partial tile.  config: keywords of OracleGrid and OccupancyGrid alike."""

    def __init__(self, name, ops, kind="rows", resolution=0.001, z_clip=Z_CLIP, many=(), partial=True, caps=None):
        self.name, self.ops, self.kind, self.resolution, self.z_clip = name, list(ops), kind, resolution, tuple(z_clip)
        self.many, self.partial, self.caps = tuple(many), partial, dict(caps or {})

    @property
    def launches(self):
        return [op for op in self.ops if op is not CLEAN]

    @property
    def min_rows(self):
        return {"rows": MIN_ROWS, "base": MIN_ROWS_BASE, "empty": 0}[self.kind]


# ---- the oracle, once per case and colour (read-only afterwards) -------------------------------------------------------------------------

_runs = {}


def rows_now(og):
    og.extract()
    return og.extract_exact()


def oracle_run(oracle_mod, case, colour=False):
    """The oracle (exact moments) through the case's schedule: dict of
    counters   the oracle's counters behind every op
    snaps      (rows, occupied) behind every clean pass, in order
    rows, occ  the last of them
    seconds    capture and clean time."""
    key = (case.name, bool(colour))
    if key in _runs:
        return _runs[key]
    og = oracle_mod.OracleGrid(resolution=case.resolution, bbox=BBOX, exact_moments=True, z_clip=case.z_clip, fuse_color=bool(colour))
    out = dict(counters=[], snaps=[], seconds=0.0)
    for op in case.ops:
        t0 = time.perf_counter()
        if op is CLEAN:
            og.clean()
        else:
            lay = op.layout
            kw = dict(point_step=lay["point_step"], off_x=lay["off_x"], off_y=lay["off_y"], off_z=lay["off_z"])
            if colour and has_rgb(lay):
                kw["off_rgb"] = lay["off_rgb"]
            for f in op.oracle_order():
                og.capture(op.records[f], op.poses[f], **kw)
        out["seconds"] += time.perf_counter() - t0
        out["counters"].append(og.counters())
        if op is CLEAN:
            rows, occ = rows_now(og), og.occupied()
            rows.setflags(write=False), occ.setflags(write=False)
            out["snaps"].append((rows, occ))
    og.close()
    out["rows"], out["occ"] = out["snaps"][-1]
    _runs[key] = out
    return out


def forget(case):
    """Drops the case's oracle runs (the many-tile ones hold a few hundred MB of frames and rows between them)."""
    for key in [k for k in _runs if k[0] == case.name]:
        del _runs[key]


def forget_all():
    """Drops every built case and oracle run (at the end of a test file: the process goes on to other files)."""
    _runs.clear()
    _cache.clear()


def occupied_keys(occ):
    occ = np.asarray(occ, np.int64).reshape(-1, 3)
    return np.sort((occ[:, 2] << 42) | (occ[:, 1] << 21) | occ[:, 0])


def live_rows(rows):
    """Rows with members and a finite normal."""
    return int(((rows["count"] > 0) & np.isfinite(rows["nx"]) & np.isfinite(rows["ny"]) & np.isfinite(rows["nz"])).sum())


# ---- the case table ----------------------------------------------------------------------------------------------------------------------
# Every builder is cached by its arguments: the CPU file and the GPU file each build a case once.

_cache = {}


def _cached(fn):
    def wrapped(*a):
        key = (fn.__name__,) + a
        if key not in _cache:
            _cache[key] = fn(*a)
        return _cache[key]
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


@_cached
def base_frames():
    """The small base model: eight 64 x 48 frames."""
    return Frames(8, 64, 48, first=9000)


# 1. tile loop ---------------------------------------------------------------------------------------------------------------------------

# n_pts -> (W, H): below, at and above one tile and two, and one wave; 8 x 8 and 16 x 16 are organised frames whose depth form
# takes the 16 x 16 patch walk (256) or must not (64: eight rows)
SINGLE_SHAPES = {1: (1, 1), 63: (9, 7), 64: (8, 8), 65: (13, 5), 255: (17, 15), 256: (16, 16), 257: (257, 1), 511: (73, 7), 513: (27, 19)}


@_cached
def single_frame(n_pts):
    """The base model, a clean pass, ONE frame of n_pts points, a clean pass."""
    W, H = SINGLE_SHAPES[n_pts]
    return Case("single frame of %d" % n_pts, [Launch(base_frames(), tag="base"), CLEAN, Launch(Frames(1, W, H, first=9100 + n_pts), tag="single"), CLEAN],
                kind="base")


MANY_SHAPES = {"small": (4100, 17, 16), "large": (64, 331, 99)}   # 272 points: a 16-lane tail every second tile; 32769: a one-lane tail
# A call of one to two million points that are all buffered (the session's first call: no cell has a normal yet) must not crowd them
# into a few bricks: a brick's parked points go to ONE of the point log's 64 append regions (k_buffer), max_log_points / 64 entries
# each.  The cameras of the many-tile cases therefore orbit wider (a brick then holds at most 25,000 points of a call, a region
# 30,000 on average), and their log has 262,144 entries a region.
WIDE_ORBIT = dict(max_angle=15.0, jitter=0.06)
MANY_CAPS = dict(max_log_points=16 << 20)


@_cached
def many_tiles(shape):
    """Two calls of MANY_TILES tiles whose frames end in a partial tile: the session's first call (no plan: the dry run), a clean
    pass, and a second call behind it (bin plan, k_buffer, k_update_cells), a clean pass."""
    n, W, H = MANY_SHAPES[shape]
    ops = [Launch(Frames(n, W, H, first=0, **WIDE_ORBIT), tag="first call"), CLEAN, Launch(Frames(n, W, H, first=n, **WIDE_ORBIT), tag="second call"), CLEAN]
    # the large frames see 24 x 7 cm of the scene: at 2 mm the oracle takes a third of the time it takes at 1 mm, for 30,000 rows
    return Case("many tiles, %s frames" % shape, ops, many=(0, 2), caps=dict(MANY_CAPS, max_frames=4 * n), resolution=0.002 if shape == "large" else 0.001)


def shuffled_ids(case, seed=0x1D5):
    """The case with its frames in another order in memory and the explicit, non-monotone ids that name the same sequence: per launch
    (order, ids) such that frame order[k] of the case's launch sits at position k and carries the id it has in the case."""
    out, first = [], 0
    for op in case.launches:
        order = np.random.default_rng(seed + first).permutation(op.n_frames)
        out.append((order, (first + order).astype(np.uint32)))
        first += op.n_frames
    return out


# 3. patch walk ----------------------------------------------------------------------------------------------------------------------------

PATCH_SHAPES = {16: (16, 16, 8192), 32: (32, 16, 4096), 48: (48, 32, 1366)}   # frame_width -> (W, H, frames): 1, 2 and 6 tiles a frame


@_cached
def patch_walk(width):
    """One call of MANY_TILES tiles of organised W x H frames (packed clouds), a clean pass."""
    W, H, n = PATCH_SHAPES[width]
    return Case("patch walk, %d x %d" % (W, H), [Launch(Frames(n, W, H, first=20000, depth=None, **WIDE_ORBIT), tag="patches"), CLEAN], many=(0,), partial=False,
                caps=dict(MANY_CAPS, max_frames=n))


# frames of 48 x 24 = 1152 points: hints the host must ignore -- rows not a multiple of 16; a width that does not divide n_points;
# a width below 16; a width above n_points; a width that is no multiple of 16 (24 divides 1152 into 48 rows)
IGNORED_HINTS = (48, 80, 8, 2000, 24, 32)


@_cached
def patch_ignored():
    ops = [Launch(Frames(96, 48, 24, first=21000, depth=None), tag="48 x 24"), CLEAN, Launch(Frames(96, 48, 24, first=21100, depth=None), tag="48 x 24"), CLEAN]
    return Case("patch hints to ignore, 48 x 24", ops, caps=dict(max_frames=256))


# 2. record forms ------------------------------------------------------------------------------------------------------------------------

LAYOUTS = {
    "packed16": PACKED16,
    "xyz12": dict(point_step=12, off_x=0, off_y=4, off_z=8, off_rgb=8),          # xyz only: off_rgb names a valid field, colour off
    "zyx16": dict(point_step=16, off_x=8, off_y=4, off_z=0, off_rgb=12),
    "rgb_first16": dict(point_step=16, off_x=4, off_y=8, off_z=12, off_rgb=0),
    "step20": dict(point_step=20, off_x=0, off_y=4, off_z=8, off_rgb=16),
    "pcl32": PCL32,
    "tail48": dict(point_step=48, off_x=32, off_y=36, off_z=40, off_rgb=44),
}
LAYOUT_RES = 0.002          # gpu_support.RES: the track and query references of the GPU tests are written for it
LAYOUT_SHAPE = (131, 97)    # 12707 points: odd, 49 full tiles and one of 163
LAYOUT_FRAMES = 10


def synth_records(layout, first, n, W, H):
    """n frames of hfpf_synth.frame(layout=...) and their poses; the bytes the generator leaves zero between the fields are
    overwritten with PAD_WORD's.  The generator writes the colour last, so a layout without an rgb field (off_rgb naming x, y or z)
    is laid out from the packed frame instead."""
    poses = np.stack([S.pose(POSE_SEED, first + f, 10.0, 0.02) for f in range(n)])
    words = layout["point_step"] // 4
    used = {layout[k] // 4 for k in ("off_x", "off_y", "off_z", "off_rgb")}
    recs = []
    for f in range(n):
        if not has_rgb(layout):
            packed = S.frame(SEED, first + f, W, H, poses[f], fx=FX, nan_permille=HOLES).view(np.uint32).reshape(-1, 4)
            recs.append(relayout(packed, layout))
            continue
        rec = S.frame(SEED, first + f, W, H, poses[f], fx=FX, nan_permille=HOLES, layout=layout).view(np.uint32).reshape(-1, words).copy()
        for w in range(words):
            if w not in used:
                rec[:, w] = PAD_WORD
        recs.append(rec.view(np.uint8).reshape(-1))
    return recs, poses


@_cached
def record_form(name):
    """Five frames of 131 x 97 records in LAYOUTS[name], a clean pass, five more, a clean pass."""
    lay = LAYOUTS[name]
    W, H = LAYOUT_SHAPE
    half = LAYOUT_FRAMES // 2
    ops = []
    for k in range(2):
        recs, poses = synth_records(lay, 30000 + k * half, half, W, H)
        ops += [Launch(records=recs, layout=lay, poses=poses, tag=name), CLEAN]
    return Case("record form %s" % name, ops, resolution=LAYOUT_RES)


def held_out_records(layout=PACKED16):
    """A frame of the record-form scene that no case integrates: (records, pose) for track and query."""
    recs, poses = synth_records(layout, 30100, 1, *LAYOUT_SHAPE)
    return recs[0], poses[0]


# 4. depth images --------------------------------------------------------------------------------------------------------------------------

DEPTH_SHAPES = ((1, 1), (1, 257), (257, 1), (17, 13), (33, 31))   # W x H: one pixel, one-pixel rows, one-pixel columns, odd widths
DEPTH_FRAMES = 6


@_cached
def depth_case(W, H, fmt):
    """The base model, a clean pass, six depth frames of W x H in `fmt` ("u16" | "f32"), a clean pass."""
    ops = [Launch(base_frames(), tag="base"), CLEAN, Launch(Frames(DEPTH_FRAMES, W, H, first=40000 + 100 * W + H, depth=fmt), tag="%d x %d %s" % (W, H, fmt)), CLEAN]
    return Case("depth %d x %d %s" % (W, H, fmt), ops, kind="base")


# 5. config --------------------------------------------------------------------------------------------------------------------------------

Z_CLIPS = ((0.25, 0.5), (0.3, 0.3), (0.6, 0.28), (-1.0, 0.45), (0.28, float("inf")))
ZCLIP_SHAPE = (96, 72, 12)   # W, H, frames


def f32_steps(v):
    """The f32 values at, one step below and one step above the double v (v itself rounded to nearest; inf stays inf and has no
    step above; the step below it is the largest finite float)."""
    c = np.float32(v)
    out = [np.nextafter(c, np.float32(-np.inf)), c]
    if np.isfinite(c):
        out.append(np.nextafter(c, np.float32(np.inf)))
    return [np.float32(x) for x in out]


def bound_values(z_clip):
    """Every z a boundary test wants for this interval: on each bound and one f32 step either side."""
    return np.array(sorted({float(x) for b in z_clip for x in f32_steps(b)}), np.float32)


@_cached
def zclip_case(lo, hi):
    """Twelve 96 x 72 frames in two epochs under z_clip = (lo, hi).  In every frame the z of the first records with a reading is
    replaced by the boundary values (x and y stay: the point moves along the camera's axis), each value in 16 records."""
    W, H, n = ZCLIP_SHAPE
    vals = np.repeat(bound_values((lo, hi)), 16)
    ops = []
    for k in range(2):
        fr = Frames(n // 2, W, H, first=50000 + k * (n // 2), depth=None)
        clouds = fr.clouds.copy()
        for f in range(fr.n):
            ok = np.flatnonzero(np.isfinite(clouds[f, :, 2].view(np.float32)))[:len(vals)]
            clouds[f, ok, 2] = vals[:len(ok)].view(np.uint32)
        ops += [Launch(records=clouds.view(np.uint8).reshape(fr.n, -1), poses=fr.poses, tag="z on the bounds"), CLEAN]
    empty = not (lo < hi)
    return Case("z_clip (%g, %g)" % (lo, hi), ops, kind="empty" if empty else "rows", z_clip=(lo, hi))


CALL_FRAMES = (8, 24, 16)   # a three-call session; the largest call is the second


@_cached
def call_points_case():
    ops, first = [], 60000
    for n in CALL_FRAMES:
        ops += [Launch(Frames(n, 64, 48, first=first, depth=None), tag="%d frames" % n), CLEAN]
        first += n
    return Case("three calls", ops)


def largest_call(case):
    return max(op.n_points * op.n_frames for op in case.launches)


def all_cases():
    """Every case of the table (name -> builder call), for the CPU test."""
    out = [single_frame(n) for n in SINGLE_SHAPES]
    out += [many_tiles(s) for s in MANY_SHAPES]
    out += [patch_walk(w) for w in PATCH_SHAPES] + [patch_ignored()]
    out += [record_form(n) for n in LAYOUTS]
    out += [depth_case(W, H, fmt) for W, H in DEPTH_SHAPES for fmt in ("u16", "f32")]
    out += [zclip_case(lo, hi) for lo, hi in Z_CLIPS] + [call_points_case()]
    return out
