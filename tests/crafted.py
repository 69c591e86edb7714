"""Clouds that drive the hot path to its internal limits (imported by tests only).

The sensor-like scenes of tests/scenes.py give a brick ~150 points a frame, spread over a tilted sheet of cells; the limits of
k_update_cells, k_buffer and k_integrate (ENGINE below) are field widths, LDS capacities and form switches that such scenes reach by
chance.  Here a cloud is built from a map cell -> number of points, in the conventions of lattice.cloud (the dyadic box of
tests/faces.py, the camera 0.3125 m below the box's minimum corner, packed 16-byte records), on a base surface of flat sheets one cell
thick, so that a chosen TARGET BRICK T lies in the interior of the sheets with its neighbours along the normal.

Every case is a schedule of LAUNCHES (one hfpf_integrate_device call each: a list of frames of equal length, their poses and, where
the case needs them, explicit frame ids) and clean passes.  What a case is for -- the fill of T, the rounds it takes, the work items of
a round, the records with members -- is computed from the oracle alone (figures), asserted on the CPU in test_crafted_models.py and
compared with the engine's counters in test_gpu_crafted.py.

The base surface.  Sheets normal to z over x 32..55, y 24..47 (24 x 24 cells; T = cells 40..47 x 32..39 x 40..47, brick (5, 4, 5)).
A stencil is 5 x 5 x 5, so a sheet three cells from the next sees only itself (25 cells: the default gate passes, the normal is +-z),
and a record's line covers 2K + 1 = 7 cells: an occupied cell collects a dependant from every sheet within three layers.  Two epochs
-- layers 37, 40, 43, 46, 49, clean, then layers 38, 41, 44, 47, 50, clean -- give every sheet cell of T four or five dependants
(the second epoch's stencils hold two or three flat layers: still +-z).  A solid block would not do: its interior stencils are isotropic
and the normals come out NaN."""
import numpy as np

import faces
import lattice as L

# ---- the engine's constants the cases are built on (test_crafted_models.py reads them again out of the text of kernels.hpp) ----------
# csrc/kernels.hpp:  HFPF_UPD_DENSE_SHAPE / HFPF_UPD_WIDE_SHAPE  "#define ... threads, CAP, SLOTS, DESC, waves"   (struct UpdShape)
#                    kUpdDenseColor / kUpdWideColor               the two shapes with colour
#                    HFPF_UPD2_CHUNK                              points of a cell one work item takes
#                    kBufLdsMin                                   k_buffer: runs at least this long chain in LDS
#                    kOccStage                                    k_integrate: newly occupied cells a wave stages
# csrc/hfpf.hip:     "max_frames must be <= 2^23"                 a parked point carries its frame id in 23 bits (lcell | fid << 9)
ENGINE = {
    "dense": dict(cap=2048, slots=352, desc=1280),
    "wide": dict(cap=1536, slots=512, desc=1024),
    "dense_colour": dict(cap=1024, slots=352, desc=1024),
    "wide_colour": dict(cap=1024, slots=512, desc=1024),
}
CHUNK = 8
BUF_LDS_MIN = 256
OCC_STAGE = 256
MAX_FRAMES = 1 << 23
BRICK = 8           # cells an axis (tables.hpp kBrickCells = 512)
INTEGRATE_GRID = 2048   # workgroups of k_integrate the occupancy case is sized for (hfpf.hip: integrate_grid = workgroups per CU x CUs)

RES = faces.DYADIC_RES
BBOX = faces.DYADIC_BBOX
DIMS = L.DIMS
CAMERA_DEPTH = L.CAMERA_DEPTH

T_BRICK = (5, 4, 5)
T_LO = np.array([40, 32, 40])
SHEET_X, SHEET_Y = (32, 56), (24, 48)
LAYERS_A = (37, 40, 43, 46, 49)
LAYERS_B = (38, 41, 44, 47, 50)


def local_index(c):
    """tables.hpp local_index: the bits of x, y, z interleaved, x highest."""
    c = np.asarray(c, np.int64) & 7
    out = np.zeros(c.shape[:-1], np.int64)
    for bit in range(3):
        out |= (((c[..., 0] >> bit) & 1) << (3 * bit + 2)) | (((c[..., 1] >> bit) & 1) << (3 * bit + 1)) | (((c[..., 2] >> bit) & 1) << (3 * bit))
    return out


def brick_of(cells):
    return np.asarray(cells, np.int64) // BRICK


def sheet(layers, x=SHEET_X, y=SHEET_Y):
    """The cells of flat sheets normal to z, (n, 3) int64."""
    ax = [np.arange(*x), np.arange(*y), np.asarray(layers)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def t_cells(layers):
    """The cells of T in the given z-layers (global), in local-index order."""
    c = sheet(layers, (T_LO[0], T_LO[0] + 8), (T_LO[1], T_LO[1] + 8))
    return c[np.argsort(local_index(c), kind="stable")]


# ---- the cloud builder ---------------------------------------------------------------------------------------------------------------

def pose_of(flip=False, bbox=BBOX, dims=DIMS, res=RES):
    """The camera of lattice.cloud (no rotation, CAMERA_DEPTH below the box's minimum corner) or, flipped, one that looks down from
    CAMERA_DEPTH above its maximum corner (a half turn about x): the viewpoints lie on opposite sides of every sheet."""
    lo, _ = faces.lo_hi(bbox)
    if not flip:
        return np.hstack([np.eye(3), (lo - np.array([0.0, 0.0, CAMERA_DEPTH])).reshape(3, 1)])
    t = lo + np.array([0.0, dims[1] * res, dims[2] * res + CAMERA_DEPTH])
    return np.hstack([np.diag([1.0, -1.0, -1.0]), t.reshape(3, 1)])


def points(cells, seed, spread=0.45, flip=False, bbox=BBOX, dims=DIMS, res=RES):
    """(records, pose): one packed 16-byte record (x, y, z, rgb) per row of `cells`, in their order, at the cell centre plus a
    reproducible uniform jitter of +-spread cells an axis, in the frame of the camera pose_of(flip).  A record's cylinder has a
    radius of 1 mm = 0.512 cells about the line through the cell centre: at spread 0.45 about four in five of a cell's points lie
    inside it, the corners of the square outside.  rgb is a random 24-bit colour."""
    rng = np.random.default_rng(seed)
    cells = np.asarray(cells, np.float64).reshape(-1, 3)
    local = (cells + 0.5 + rng.uniform(-spread, spread, cells.shape)) * float(res)   # from the box's minimum corner
    rec = np.zeros((len(cells), 4), np.float32)
    if flip:
        local = np.array([0.0, dims[1] * res, dims[2] * res + CAMERA_DEPTH]) + local * np.array([1.0, -1.0, -1.0])
    else:
        local[:, 2] += CAMERA_DEPTH
    rec[:, :3] = local
    rec[:, 3] = rng.integers(0, 1 << 24, len(cells)).astype(np.uint32).view(np.float32)
    return np.ascontiguousarray(rec), pose_of(flip, bbox, dims, res)


def from_counts(cells, counts, seed, **kw):
    """points() for counts[i] points in cells[i], in a reproducible random order."""
    cells, counts = np.asarray(cells, np.int64).reshape(-1, 3), np.asarray(counts, np.int64)
    assert len(cells) == len(counts) and (counts >= 0).all()
    per_point = np.repeat(cells, counts, axis=0)
    per_point = per_point[np.random.default_rng(seed ^ 0x5EED).permutation(len(per_point))]
    return points(per_point, seed, **kw)


# ---- schedules -------------------------------------------------------------------------------------------------------------------------

class Launch:
    """One integrate call: frames (record arrays of equal length), their poses, explicit frame ids or None."""

    def __init__(self, frames, poses, ids=None, tag=""):
        self.frames, self.poses, self.ids, self.tag = list(frames), list(poses), (None if ids is None else [int(i) for i in ids]), tag
        assert len(self.frames) == len(self.poses) and len({len(f) for f in self.frames}) == 1
        assert self.ids is None or len(self.ids) == len(self.frames)

    @property
    def n_points(self):
        return len(self.frames[0])

    def oracle_order(self):
        """The frames as a sequential capture takes them: by frame id (the smallest id that touched a cell is its viewpoint)."""
        return range(len(self.frames)) if self.ids is None else np.argsort(self.ids, kind="stable")


CLEAN = "clean"


def single(rec, pose, tag="", fid=None):
    return Launch([rec], [pose], None if fid is None else [fid], tag)


def base_ops(seed=0xBA5E):
    """The two-epoch base surface: two frames on the first epoch's layers, clean, one on the second's, clean."""
    a, b = sheet(LAYERS_A), sheet(LAYERS_B)
    ops = [single(*points(a, seed + k, spread=0.3), tag="base") for k in range(2)] + [CLEAN]
    ops += [single(*points(b, seed + 2, spread=0.3), tag="base"), CLEAN]
    return ops


class Case:
    """ops: Launch | CLEAN; `measured`: index of the launch whose counters the case is about (None: a clean pass is); the figures of
    the launch are taken from the oracle's state just ahead of it."""

    def __init__(self, name, ops, measured, config=None, caps=None, cells=None, figures_at=None, snaps=()):
        self.name, self.ops, self.measured = name, ops, measured
        self.figures_at = measured if figures_at is None else figures_at   # the launch figures() is taken ahead of
        self.snaps = tuple(snaps)   # indices of ops behind which the occupied list is compared as well
        self.config, self.caps = dict(config or {}), dict(caps or {})
        self.cells = cells   # the crafted cells a CPU test looks at


def drive_oracle(og, ops, colour):
    for op in ops:
        if op is CLEAN:
            og.clean()
        else:
            for f in op.oracle_order():
                og.capture(op.frames[f], op.poses[f], **(dict(off_rgb=12) if colour else {}))


def oracle_grid(oracle_mod, case, colour=False):
    return oracle_mod.OracleGrid(resolution=RES, bbox=BBOX, exact_moments=True, **case.config, **(dict(fuse_color=True) if colour else {}))


# ---- figures, from the oracle alone --------------------------------------------------------------------------------------------------

def cells_of(og, rec, pose):
    """The cell of every record as the oracle indexes it (n, 3), and which lie in the box."""
    import oracle
    xyz = oracle.probe_transform(pose, np.ascontiguousarray(rec[:, :3]))
    return og.probe_index(xyz)


def rows_now(og):
    og.extract()
    return og.extract_exact()


def state(og, launch):
    """Per distinct cell the launch's points fall into: (cells, points, has a normal, number of dependants), before the launch."""
    all_cells = []
    for rec, pose in zip(launch.frames, launch.poses):
        idx, valid = cells_of(og, rec, pose)
        assert valid.all(), "a crafted point lies outside the box"
        all_cells.append(idx)
    cells, n = np.unique(np.vstack(all_cells), axis=0, return_counts=True)
    rows = rows_now(og)
    with_normal = {(int(r["ix"]), int(r["iy"]), int(r["iz"])) for r in rows}
    has_n = np.array([tuple(int(v) for v in c) in with_normal for c in cells], bool)
    deps = np.array([len(og.dependants(int(c[0]), int(c[1]), int(c[2]))) for c in cells], np.int64)
    return cells, n, has_n, deps


def figures(og, launch, form):
    """What the launch means to k_integrate and k_update_cells<form>, from the state of `og` just ahead of it:
    fill       brick -> points k_integrate parks (cell without a normal, or with dependants)
    rounds     sum over bricks of (fill - 1) // CAP: the growth of update_extra_rounds
    items      brick -> work items if the brick's fill is one round: sum over cells of deps * ceil(n / CHUNK)
    cells, n, has_n, deps: state()"""
    cap = ENGINE[form]["cap"]
    cells, n, has_n, deps = state(og, launch)
    parked = (~has_n) | (deps > 0)
    fill, items = {}, {}
    for c, k, p, d in zip(cells, n, parked, deps):
        if p:
            b = tuple(int(v) for v in brick_of(c))
            fill[b] = fill.get(b, 0) + int(k)
            items[b] = items.get(b, 0) + int(d) * ((int(k) + CHUNK - 1) // CHUNK)
    rounds = sum((f - 1) // cap for f in fill.values())
    return dict(fill=fill, rounds=rounds, items=items, cells=cells, n=n, has_n=has_n, deps=deps)


def records_with_members(og, launch, colour=False):
    """Feeds the launch to `og` and returns how many records gained a member through it (the count column of the rows)."""
    before = rows_now(og)
    drive_oracle(og, [launch], colour)
    after = rows_now(og)
    assert len(before) == len(after)
    return int((after["count"] > before["count"]).sum())


# ---- the cases -----------------------------------------------------------------------------------------------------------------------

ELIGIBLE_LAYERS = (40, 41, 43, 44, 46, 47)   # the sheet layers inside T: 384 cells with a normal and four or five dependants each


def eligible():
    return t_cells(ELIGIBLE_LAYERS)


def _twice(rec, pose, tag):
    """The demand launch and the measured launch: the identical frame twice (the plan of a launch is the demand of the one before)."""
    return [single(rec, pose, tag + ", demand"), single(rec, pose, tag + ", measured")]


def update_case(name, cells, counts, seed, spread=0.45):
    rec, pose = from_counts(cells, counts, seed, spread=spread)
    ops = base_ops() + _twice(rec, pose, name) + [CLEAN]
    return Case(name, ops, len(ops) - 2, cells=np.asarray(cells)[np.asarray(counts) > 0])


def one_cell_fills_a_round(form, where):
    """Case 1.  CAP + 1 points in one cell of T: local index 0, local index 511, or the all-odd cell (41, 33, 41) with a single point in
    cell 0 in front of it, so that a full cell's first position is not zero."""
    cap = ENGINE[form]["cap"]
    cell = {"first": T_LO, "last": T_LO + 7, "odd": T_LO + 1}[where]
    cells, counts = [cell], [cap + 1]
    if where == "odd":
        cells, counts = [T_LO, cell], [1, cap + 1]
    return update_case("one cell fills a round (%s, cap %d)" % (where, cap), np.array(cells), counts, 0xC100 + len(where))


def round_boundaries(form, k):
    """Case 2.  A fill of exactly CAP, CAP + 1, 2 CAP, 2 CAP + 1 (k = 0..3) spread unevenly over the eligible cells of T."""
    cap = ENGINE[form]["cap"]
    fill = (cap, cap + 1, 2 * cap, 2 * cap + 1)[k]
    el = eligible()
    counts = np.random.default_rng(0xC200 + k).multinomial(fill, np.full(len(el), 1.0 / len(el)))
    return update_case("round boundary %d (cap %d)" % (fill, cap), el, counts, 0xC210 + k)


def more_items_than_descriptors(form):
    """Case 3.  0 to 9 points in every eligible cell of T, uneven: one chunk and two, empty cells between occupied ones, at most CAP
    points in all (one round) and, with four or five dependants a cell, more work items than the round has descriptors."""
    cap = ENGINE[form]["cap"]
    hi = {2048: 8, 1536: 6, 1024: 2}[cap]
    rng = np.random.default_rng(0xC300)
    el = eligible()
    r = rng.uniform(size=len(el))
    counts = np.where(r < 0.12, 0, np.where(r < 0.22, 9, rng.integers(1, hi + 1, len(el))))
    return update_case("more items than descriptors (cap %d)" % cap, el, counts, 0xC310)


def full_table(form):
    """Case 4.  One point near the centre of every eligible cell of T: each is a member of the records of its own column, in T and in
    the bricks above and below whose lines enter T."""
    el = eligible()
    return update_case("full table", el, np.ones(len(el), np.int64), 0xC400, spread=0.1)


def largest_item_sums(form):
    """Case 5.  Full chunks of points at the far end of a record's segment -- the cell three layers above the record's, in its upper
    half -- and just inside the radius: 64 points in each of four cells of layer 43 of T, whose columns hold the records of layer 40
    (u near +3.5 cells for them), 0.9 to 0.99 mm from the line."""
    rng = np.random.default_rng(0xC500)
    cells = t_cells((43,))[[5, 18, 33, 60]]
    per_point = np.repeat(cells, 64, axis=0)
    rec, pose = points(per_point, 0xC501, spread=0.0)
    # towards the cell's corners: at 0.99 mm along an axis a point would leave the cell (half a cell is 0.977 mm)
    ang = np.pi / 4 + np.pi / 2 * rng.integers(0, 4, len(per_point)) + rng.uniform(-0.3, 0.3, len(per_point))
    rad = rng.uniform(0.90e-3, 0.99e-3, len(per_point))
    rec[:, 0] += (rad * np.cos(ang)).astype(np.float32)
    rec[:, 1] += (rad * np.sin(ang)).astype(np.float32)
    rec[:, 2] += rng.uniform(0.30, 0.49, len(per_point)).astype(np.float32) * np.float32(RES)
    ops = base_ops() + _twice(rec, pose, "largest item sums") + [CLEAN]
    return Case("largest item sums", ops, len(ops) - 2, cells=cells)


PRE_LAYERS = (42, 45)   # free layers of T between the sheets: every cell carries the one pre-dependant the base's passes left


def pre_dependant_lists(form):
    """Case 6.  In the epoch behind the base's second pass, without a clean in between: a frame occupies the free layers 42 and 45 of T
    (cells that carry a pre-dependant), then more than CAP points go into exactly those cells, twice."""
    cap = ENGINE[form]["cap"]
    fresh = t_cells(PRE_LAYERS)
    counts = np.random.default_rng(0xC600).multinomial(cap + 1, np.full(len(fresh), 1.0 / len(fresh)))
    rec, pose = from_counts(fresh, counts, 0xC610)
    ops = base_ops() + [single(*points(fresh, 0xC601, spread=0.3), tag="occupy")] + _twice(rec, pose, "pre-dependant lists") + [CLEAN]
    return Case("pre-dependant lists (cap %d)" % cap, ops, len(ops) - 2, cells=fresh)


# ---- replay and k_buffer -------------------------------------------------------------------------------------------------------------

REPLAY_FRAMES = 9        # more than the dry run's 8: a session's first call then has a plan and parks from its first point
REPLAY_M = 2
REPLAY_LAYERS = (38, 47)   # in bricks of their own: 64 cells x 9 frames stay below every CAP


def streamed_replay(form):
    """Case 7.  One first call of nine frames: each holds the sheets 38 and 47 once (one point per cell), and T receives REPLAY_M * CAP + 1
    points in all, its own sheet points included, evenly over the frames (the plan comes from the first eight: 8/9 of the demand
    x 9/8 x 1.5 + 64).  Everything is buffered, T's points as ONE run.  Clean.  The second epoch lays the sheet 48, in the bricks above:
    its records register in the cells of layer 47, which have lists by then, and T's run is streamed again with the lists cut."""
    cap = ENGINE[form]["cap"]
    base = sheet(REPLAY_LAYERS)
    in_t = (brick_of(base) == np.array(T_BRICK)).all(axis=1)
    heavy = t_cells((47,))
    total = REPLAY_M * cap + 1 - REPLAY_FRAMES * int(in_t.sum())
    share = [total // REPLAY_FRAMES + (1 if f < total % REPLAY_FRAMES else 0) for f in range(REPLAY_FRAMES)]
    frames, poses = [], []
    rng = np.random.default_rng(0xC700)
    for f in range(REPLAY_FRAMES):
        extra = heavy[rng.integers(0, len(heavy), share[f])]
        pad = base[~in_t][rng.integers(0, int((~in_t).sum()), max(share) - share[f])]   # frames of one call have one length
        rec, pose = points(np.vstack([base, extra, pad]), 0xC710 + f)
        frames.append(rec), poses.append(pose)
    ops = [Launch(frames, poses, tag="streamed replay, first epoch"), CLEAN, single(*points(sheet((48,)), 0xC720, spread=0.3), tag="second epoch"), CLEAN]
    return Case("streamed replay (cap %d)" % cap, ops, None, cells=heavy, figures_at=0)


BUF_BRICKS = ((4, 4, 4), (5, 4, 4), (6, 4, 4))   # below the base's layer 37, z 32..39
BUF_COUNTS = (BUF_LDS_MIN - 1, BUF_LDS_MIN, BUF_LDS_MIN + 1)
BUF_LAYER = 36


def buffer_runs(spread_over_brick):
    """Case 8.  Behind the base: three bricks receive exactly 255, 256 and 257 points in never occupied cells of layer 36 (one cell
    each, or the brick's 64 cells of the layer) in ONE call of three frames whose ids are out of order, the middle id's camera above
    the sheets and the others below.  The demand launch before it carries larger ids, so the measured call decides the latch; a
    later call adds 10 points to each brick through the other chaining path."""
    def cells_for(n, brick, rng):
        lo = np.array(brick) * BRICK
        if not spread_over_brick:
            return np.repeat([[lo[0] + 3, lo[1] + 4, BUF_LAYER]], n, axis=0)
        c = sheet((BUF_LAYER,), (lo[0], lo[0] + 8), (lo[1], lo[1] + 8))
        return c[rng.integers(0, len(c), n)]

    def batch(seed, ids, counts):
        rng = np.random.default_rng(seed)
        per_brick = [cells_for(n, b, rng) for n, b in zip(counts, BUF_BRICKS)]
        n_frames = len(ids)
        frames, poses = [], []
        # frame f takes every n_frames-th point of the three bricks, rotated so that the frames have one length
        allp = np.vstack(per_brick)
        assert len(allp) % n_frames == 0
        for f in range(n_frames):
            rec, pose = points(allp[f::n_frames], seed + 1 + f, flip=(f == 1))
            frames.append(rec), poses.append(pose)
        return Launch(frames, poses, ids, "k_buffer %r" % (ids,))

    demand = batch(0xC800, [22, 20, 21], BUF_COUNTS)
    measured = batch(0xC800, [12, 10, 11], BUF_COUNTS)
    later = batch(0xC850, [30], (10, 10, 10))
    ops = base_ops() + [demand, measured, later, CLEAN]
    return Case("k_buffer at kBufLdsMin (%s)" % ("spread" if spread_over_brick else "single cell"), ops, len(ops) - 3)


# ---- k_integrate ---------------------------------------------------------------------------------------------------------------------

NEAR_BRICKS = ((3, 2, 3), (7, 6, 7))


def wave_grouping():
    """Case 9.  Behind the base, three calls: (a) three identical frames of 1024 points, every run of 64 consecutive points in 64
    distinct bricks no point has touched; (b) 512 points in one cell; (c) 512 points alternating between two bricks of the sheets,
    cells with a normal and never occupied cells mixed."""
    nb = [d // BRICK for d in DIMS]
    bricks = np.stack(np.meshgrid(*[np.arange(n) for n in nb], indexing="ij"), -1).reshape(-1, 3)
    # the base lies in the bricks 4..6 x 3..5 x 4..6, and what its records register (seven cells along the normal, which lies in the
    # plane at the rim of a sheet) within the bricks beside them: a clean pass allocates those
    near = ((bricks >= np.array(NEAR_BRICKS[0])) & (bricks <= np.array(NEAR_BRICKS[1]))).all(axis=1)
    far = bricks[~near]
    assert len(far) >= 1024
    far = far[np.random.default_rng(0xC900).permutation(len(far))[:1024]]
    cells_a = far * BRICK + np.random.default_rng(0xC901).integers(0, BRICK, far.shape)
    rec_a, pose = points(cells_a, 0xC902)
    one = np.repeat([T_LO + np.array([3, 4, 2])], 512, axis=0)   # layer 42: never occupied, carries a pre-dependant
    left, right = t_cells((40, 42)), t_cells((40, 42)) + np.array([8, 0, 0])
    rng = np.random.default_rng(0xC903)
    alt = np.empty((512, 3), np.int64)
    alt[0::2] = left[rng.integers(0, len(left), 256)]
    alt[1::2] = right[rng.integers(0, len(right), 256)]
    ops = base_ops() + [Launch([rec_a] * 3, [pose] * 3, tag="all lanes lead"), single(*points(one, 0xC904), tag="one cell"),
                        single(*points(alt, 0xC905), tag="two bricks alternating"), CLEAN]
    n = len(ops)
    return Case("wave grouping extremes", ops, None, cells=cells_a, snaps=(n - 4, n - 3, n - 2))


OCC_RES = 0.001
OCC_BBOX = (-0.5, 0.5, -0.5, 0.5, 0.0, 1.0)
OCC_TILES = 5


def occupancy_staging():
    """Case 10.  One call of one frame in which every point is the first touch of its cell, OCC_TILES tiles of 256 points for each
    of INTEGRATE_GRID workgroups: a sheet three cells thick in the 1 m^3 box at 1 mm, seen by an unrotated camera 0.4 m below it.
    Consecutive points lie in consecutive cells along x, so a wave's 64 points are all new and the stage fills 64 at a time."""
    n = INTEGRATE_GRID * OCC_TILES * 256
    side = int(np.ceil(np.sqrt(n / 3.0)))
    assert side <= 1000
    i = np.arange(n, dtype=np.int64)
    cells = np.stack([i % side, (i // side) % side, 500 + i // (side * side)], axis=1).astype(np.float64)
    rng = np.random.default_rng(0xCA00)
    world = np.array([-0.5, -0.5, 0.0]) + (cells + 0.5 + rng.uniform(-0.3, 0.3, cells.shape)) * OCC_RES
    rec = np.zeros((n, 4), np.float32)
    rec[:, :3] = world - np.array([0.0, 0.0, 0.1])   # camera-frame z 0.4 .. 0.403
    pose = np.hstack([np.eye(3), np.array([[0.0], [0.0], [0.1]])])
    return rec, pose, n


def largest_frame_id():
    """Case 11.  max_frames = 2^23 and the ids 2^23 - 1, 0, 2^23 - 2 in one call, twice: the session's first call (direct: no plan yet) on
    the cells of sheet 41 with x + y even, the second (planned from the first's demand: the ids travel in the parked word) on those
    with x + y odd.  Id 2^23 - 2 looks from above at every cell, 2^23 - 1 from below at every cell, 0 from below at the cells with even
    x: the smallest id a cell has seen decides the sign of its normal."""
    sh = sheet((41,))
    ids = [MAX_FRAMES - 1, 0, MAX_FRAMES - 2]
    ops = []
    for k, parity in enumerate((0, 1)):
        mine = sh[(sh[:, 0] + sh[:, 1]) % 2 == parity]
        half = mine[mine[:, 0] % 2 == 0]
        assert 2 * len(half) == len(mine)
        f_hi, pose_hi = points(mine, 0xCB00 + 8 * k)                                   # id 2^23 - 1, from below
        f_0, pose_0 = points(np.vstack([half, half]), 0xCB01 + 8 * k)                  # id 0, from below, even x only
        f_top, pose_top = points(mine, 0xCB02 + 8 * k, flip=True)                      # id 2^23 - 2, from above
        ops.append(Launch([f_hi, f_0, f_top], [pose_hi, pose_0, pose_top], ids, "ids %r, %s" % (ids, ("direct", "planned")[k])))
    ops.append(CLEAN)
    return Case("largest frame id", ops, 1, caps=dict(max_frames=MAX_FRAMES), cells=sh)


# ---- one oracle run per case, shared by the CPU and the GPU tests (read-only) ----------------------------------------------------------

_runs = {}


def oracle_run(oracle_mod, case, form, colour=False):
    """The oracle through the case's schedule, once per (case, colour): dict of
    figures    figures() ahead of the launch case.figures_at (None without one)
    records    records that gained a member through that launch
    counters   the oracle's counters behind every op
    occupied   op index -> occupied list, for case.snaps
    rows, occ  exact rows and occupied list at the end."""
    key = (case.name, bool(colour))
    if key in _runs:
        return _runs[key]
    og = oracle_grid(oracle_mod, case, colour)
    out = dict(figures=None, records=None, counters=[], occupied={})
    for i, op in enumerate(case.ops):
        if i == case.figures_at:
            out["figures"] = figures(og, op, form)
            out["records"] = records_with_members(og, op, colour)
        else:
            drive_oracle(og, [op], colour)
        out["counters"].append(og.counters())
        if i in case.snaps:
            out["occupied"][i] = og.occupied()
    out["rows"], out["occ"] = rows_now(og), og.occupied()
    og.close()
    for a in (out["rows"], out["occ"]):
        a.setflags(write=False)
    _runs[key] = out
    return out


def occupied_keys(occ):
    """An occupied list as a sorted array of int64 keys: two lists hold the same set when their keys are equal."""
    occ = np.asarray(occ, np.int64).reshape(-1, 3)
    return np.sort((occ[:, 2] << 42) | (occ[:, 1] << 21) | occ[:, 0])
