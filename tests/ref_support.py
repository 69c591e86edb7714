"""The compiled reference grid (oracle/_ref/libhfpf_ref.so, built by `make -C oracle ref` from oracle/ref_driver.cpp and the reference
tree's own OccupancyGrid.hpp) and the cases it is compared on (imported by tests and by tests/golden/make_reference_golden.py only).

A CASE is a box, a resolution and a schedule of ops: ("add", records, pose) | ("clean",).  records are packed 16-byte sensor-frame
points (x, y, z, rgb as one f32 word) and pose is the 3 x 4 f64 camera -> fusion-frame transform, exactly what hfpf_integrate and
OracleGrid.capture take.  The reference's grid takes world-frame clouds and a viewpoint (its node did the rest), so world_cloud() does
the node's part for it and for OracleGrid.add_points alike: the strict z-clip in the camera frame (node.cpp:251-255), the f64
transform rounded once to f32 (oracle.probe_transform, a leaf pinned against the engine in test_gpu_leaves.py) and the viewpoint
(float)translation (node.cpp:290).  Points with a NaN coordinate are dropped there as well: in the reference they index out of
bounds (grid.hpp:633 -> 203), the oracle and the engine drop them.

Every box keeps to the reference's dense storage, 16 bytes a cell: at most 2^23 cells, and ydim < 2048 (the int shift of the
reference's key, grid.hpp:154, which order_mode=1 of the oracle reproduces only below that)."""
import ctypes as C
import os

import numpy as np

import crafted
import faces
import lattice
import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.path.join(ROOT, "oracle", "_ref", "libhfpf_ref.so")
REFERENCE_TREE = os.environ.get("HFPF_REFERENCE", "/root/reference")   # oracle/Makefile's default
MAX_CELLS = 1 << 23
Z_CLIP = (0.28, 0.6)   # node.cpp:92-93; the default of engine and oracle

_libs = {}


def available():
    return os.path.exists(LIB_PATH)


def lib(path=None):
    path = path or LIB_PATH
    if path not in _libs:
        import oracle
        L = C.CDLL(path)
        L.href_create.restype = C.c_void_p
        L.href_create.argtypes = [C.c_float, C.c_void_p]
        L.href_destroy.argtypes = [C.c_void_p]
        L.href_dims.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.href_add_points.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.href_add_points.restype = C.c_int32
        L.href_clean.argtypes = [C.c_void_p]
        L.href_is_dirty.argtypes = [C.c_void_p]
        L.href_is_dirty.restype = C.c_int32
        L.href_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.href_extract.restype = C.c_int64
        L.href_occupied.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.href_occupied.restype = C.c_uint64
        L.href_dependants.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_uint64]
        L.href_dependants.restype = C.c_uint64
        L.href_dependant_cells.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.href_dependant_cells.restype = C.c_uint64
        L.href_fresh_info_is_zero.restype = C.c_int32
        L.href_sizeof_row.restype = C.c_uint64
        assert L.href_sizeof_row() == oracle.ROW_DTYPE.itemsize
        assert L.href_fresh_info_is_zero() == 1, "the driver's zero-filling operator new is not in effect"
        _libs[path] = L
    return _libs[path]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class ReferenceGrid:
    """The reference's OccupancyGrid behind oracle/ref_driver.cpp, with the method names of oracle.OracleGrid."""

    def __init__(self, resolution, bbox, path=None):
        import oracle
        self._row_dtype = oracle.ROW_DTYPE
        self._L = lib(path)
        b = np.ascontiguousarray(bbox, np.float64)
        self._h = C.c_void_p(self._L.href_create(C.c_float(resolution), _p(b)))
        assert self._h, "href_create refused the box (ydim >= 2048)"
        d, _ = self.dims
        assert d[0] * d[1] * d[2] <= MAX_CELLS, "box too large for the reference's dense storage: %r" % (d,)

    def close(self):
        if self._h:
            self._L.href_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def dims(self):
        d = (C.c_int32 * 3)()
        r = C.c_double()
        self._L.href_dims(self._h, d, C.byref(r))
        return (d[0], d[1], d[2]), r.value

    def add_points(self, xyz, viewpoint=(0, 0, 0)):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        assert not np.isnan(xyz).any(), "a NaN coordinate is undefined behaviour in the reference (grid.hpp:633 -> 203)"
        vp = np.ascontiguousarray(viewpoint, dtype=np.float32)
        assert self._L.href_add_points(self._h, _p(xyz), xyz.shape[0], _p(vp)) == 1

    def clean(self):
        self._L.href_clean(self._h)

    def is_dirty(self):
        return bool(self._L.href_is_dirty(self._h))

    def extract(self):
        n = self._L.href_extract(self._h, None, 0)
        assert n >= 0, "the cloud the reference's downloadData emitted and its grid disagree"
        rows = np.zeros(n, dtype=self._row_dtype)
        if n:
            assert self._L.href_extract(self._h, _p(rows), n) == n
        return rows

    def occupied(self):
        n = self._L.href_occupied(self._h, None, 0)
        out = np.zeros((n, 3), dtype=np.int32)
        if n:
            self._L.href_occupied(self._h, _p(out), n)
        return out

    def dependants(self, x, y, z):
        n = self._L.href_dependants(self._h, x, y, z, None, 0)
        out = np.zeros((n, 3), dtype=np.int32)
        if n:
            self._L.href_dependants(self._h, x, y, z, _p(out), n)
        return out

    def dependant_cells(self):
        n = self._L.href_dependant_cells(self._h, None, 0)
        out = np.zeros((n, 3), dtype=np.int32)
        if n:
            self._L.href_dependant_cells(self._h, _p(out), n)
        return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------------

CLEAN = ("clean",)


class Case:
    """name, resolution, bbox, ops; contest: the rows depend on the order of a clean pass by design (compared under order_mode=1 only),
    with the reason."""

    def __init__(self, name, resolution, bbox, ops, contest=None):
        self.name, self.resolution, self.bbox, self.ops, self.contest = name, float(resolution), tuple(float(b) for b in bbox), list(ops), contest


def records(xyz):
    """Packed 16-byte records (x, y, z, rgb = 0) of (n, 3) sensor-frame points."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    rec = np.zeros((len(xyz), 4), np.float32)
    rec[:, :3] = xyz
    return rec


def world_cloud(rec, pose):
    """(world-frame f32 points, f32 viewpoint) of one op, as the node hands them to addPoints (see the module docstring)."""
    import oracle
    xyz = np.ascontiguousarray(np.asarray(rec, np.float32).reshape(-1, 4)[:, :3])
    z = xyz[:, 2].astype(np.float64)
    keep = (z < Z_CLIP[1]) & (z > Z_CLIP[0]) & ~np.isnan(xyz).any(axis=1)
    pose = np.asarray(pose, np.float64).reshape(3, 4)
    return oracle.probe_transform(pose, np.ascontiguousarray(xyz[keep])), pose[:, 3].astype(np.float32)


def drive(grid, case):
    """A ReferenceGrid or an OracleGrid through the case's schedule, by add_points and clean."""
    for op in case.ops:
        if op[0] == "add":
            grid.add_points(*world_cloud(op[1], op[2]))
        else:
            grid.clean()
    return grid


def state(grid):
    """What the parity tests compare: rows, occupied list, the cells that hold dependants and every list, in order."""
    cells = grid.dependant_cells()
    lists = [grid.dependants(int(c[0]), int(c[1]), int(c[2])) for c in cells]
    return dict(rows=grid.extract(), occupied=grid.occupied(), dep_cells=cells,
                dep_lengths=np.array([len(l) for l in lists], np.int64),
                dep_lists=np.vstack(lists) if lists else np.zeros((0, 3), np.int32))


def order_dependent_rows(rows, ref_state, canon_state):
    """Per row: whether the count of its record can depend on the order of a clean pass.  The order decides one thing: which record
    keeps an UNOCCUPIED cell that several records of one pass register on (grid.hpp:443-449); that shows in a row only when the cell
    is occupied later and its points reach the record that kept it.  So the rows in question are those of the records that are in
    the dependant list of an occupied cell under one order (ref_state: the reference's) and not under the other (canon_state: the
    oracle's, order_mode=0), multiplicities counted (duplicate line steps register twice)."""
    def key(c):
        c = np.asarray(c, np.int64).reshape(-1, 3)
        return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]

    def pairs(st):
        cell = key(st["dep_cells"])[np.repeat(np.arange(len(st["dep_cells"])), st["dep_lengths"])]
        p = np.stack([cell, key(st["dep_lists"])], axis=1)
        return p[np.isin(cell, key(st["occupied"]))]
    a, b = pairs(ref_state), pairs(canon_state)
    ua, ca = np.unique(a, axis=0, return_counts=True)
    both, n = np.unique(np.vstack([a, b]), axis=0, return_counts=True)
    mult_a = dict(zip(map(tuple, ua.tolist()), ca.tolist()))
    owners = sorted({pair[1] for pair, k in zip(map(tuple, both.tolist()), n.tolist()) if k != 2 * mult_a.get(pair, 0)})
    return np.isin(key(np.stack([rows["ix"], rows["iy"], rows["iz"]], axis=1)), np.array(owners, np.int64))


def from_scene(name, sc):
    """A scenes.Scene's frames, poses and clean schedule."""
    ops = []
    for ev in sc.schedule():
        if ev[0] == "integrate":
            rec = np.ascontiguousarray(sc.frame(ev[1])).view(np.float32).reshape(-1, 4).copy()
            rec[:, 3] = 0.0
            ops.append(("add", rec, np.asarray(sc.poses[ev[1]], np.float64)))
        else:
            ops.append(CLEAN)
    return Case(name, sc.resolution, sc.bbox, ops)


# the sphere of hfpf_synth (r = 0.10 at (0.05, 0, 0.45)) in a box of 200^3 cells at 1 mm; at 5 mm the plane z = 0.56 + 0.05 x behind it
# as well, under the scene's rotated poses (up to 30 degrees)
SPHERE_BBOX = (-0.05, 0.15, -0.10, 0.10, 0.35, 0.55)
PLANE_BBOX = (-0.30, 0.30, -0.30, 0.30, 0.30, 0.80)


def sphere_1mm():
    return from_scene("sphere capture, 1 mm", scenes.Scene(6, 80, 60, 0.001, bbox=SPHERE_BBOX, fx=615.0, clean_every=2))


def plane_5mm():
    return from_scene("plane capture, 5 mm, rotated poses", scenes.Scene(6, 96, 72, 0.005, bbox=PLANE_BBOX, clean_every=2))


def sphere_5mm():
    return from_scene("sphere capture, 5 mm", scenes.Scene(6, 96, 72, 0.005, bbox=SPHERE_BBOX, fx=615.0, clean_every=2))


def plane_1mm():
    """The plane at 1 mm: a box 2^23 cells large around the part of it a zoomed camera sees."""
    return from_scene("plane capture, 1 mm, rotated poses", scenes.Scene(6, 96, 72, 0.001, bbox=(-0.10, 0.10, -0.10, 0.10, 0.45, 0.65), fx=615.0,
                                                                       clean_every=2))


# ---- crafted clouds in a small box at any resolution --------------------------------------------------------------------------------
# The box has SMALL_CELLS + 0.4 cells an axis, so dim = SMALL_CELLS and the storage's cell index == dim exists and is 0.4 cells wide; its
# minimum corner is (-w/2, -w/2, 0.35): with an unrotated camera at the origin every point lies inside the z-clip.

SMALL_CELLS = 40


def small_bbox(res):
    w = (SMALL_CELLS + 0.4) * float(np.float32(res))
    return (-w / 2, w / 2, -w / 2, w / 2, 0.35, 0.35 + w)


def centres(res, cells, offset=(0.0, 0.0, 0.0)):
    """f64 world positions: the cells' centres plus `offset` cells."""
    r = float(np.float32(res))
    lo = np.asarray(small_bbox(res), np.float64)[0::2]
    return lo + (np.asarray(cells, np.float64).reshape(-1, 3) + 0.5 + np.asarray(offset, np.float64)) * r


def plate(xs, ys, zs):
    return np.stack(np.meshgrid(np.asarray(xs), np.asarray(ys), np.asarray(zs), indexing="ij"), -1).reshape(-1, 3)


IDENT = np.hstack([np.eye(3), np.zeros((3, 1))])


def add_world(world, pose=IDENT):
    """The op that lays the f64 world points `world` down through `pose`: sensor = R^T (world - t), rounded to f32."""
    pose = np.asarray(pose, np.float64)
    s = (np.asarray(world, np.float64) - pose[:, 3]) @ pose[:, :3]
    return ("add", records(s), pose)


def jittered(res, cells, seed, spread=0.3):
    rng = np.random.default_rng(seed)
    cells = np.asarray(cells).reshape(-1, 3)
    return centres(res, cells) + rng.uniform(-spread, spread, cells.shape) * float(np.float32(res))


def from_above(res):
    """A camera that looks down at the box from 0.3 m above its top (half a turn about x)."""
    b = small_bbox(res)
    return np.hstack([np.diag([1.0, -1.0, -1.0]), np.array([[0.0], [0.0], [b[5] + 0.3]])])


INNER = range(6, 31)   # a 25 x 25 plate: its interior passes the gate, its rim does not


def contest(res):
    """Two plates two cells apart: the cells between them are unoccupied and registered by both; the last writer of the pass keeps
    them (grid.hpp:443-449).  Then points occupy those cells (the surviving registration must survive occupation, grid.hpp:234-241),
    both plates are seen again and a second pass runs."""
    both = plate(INNER, INNER, (18, 20))
    mid = plate(INNER, INNER, (19,))
    ops = [add_world(jittered(res, both, 1)), CLEAN, add_world(jittered(res, mid, 2)), add_world(jittered(res, both, 3)), CLEAN,
           add_world(jittered(res, np.vstack([both, mid]), 4)), CLEAN]
    return Case("registration contest on an unoccupied cell", res, small_bbox(res), ops,
                contest="which of the two plates registers last on a cell between them is the order of the pass")


def several_normals(res):
    """A slab three cells thick: every cell of the middle layer lies on the lines of the records above and below it and on its own,
    so its list holds several records and a later point updates them all."""
    slab = plate(INNER, INNER, (18, 19, 20))
    ops = [add_world(jittered(res, slab, 5)), CLEAN, add_world(jittered(res, slab, 6)), add_world(jittered(res, slab, 7, spread=0.45)), CLEAN]
    return Case("a cell registered by several normals", res, small_bbox(res), ops)


def normal_leaves_grid(res):
    """Plates in the layers 1 and dim - 1 that cover the whole box in x and y, cell index == dim included: the +-K steps of their
    records leave the grid below and above (validPoints, grid.hpp:406; validCoord, grid.hpp:410), and the 5 x 5 x 5 stencils of the
    cells near the faces are clipped (grid.hpp:337).  A third plate in layer dim lies in storage the scans never visit."""
    n = SMALL_CELLS
    full = range(0, n + 1)
    low, high, beyond = plate(full, full, (1,)), plate(full, full, (n - 1,)), plate(full, full, (n,))
    # cell index == dim is 0.4 cells wide: keep its points in its lower part
    def lay(cells, seed):
        rng = np.random.default_rng(seed)
        off = rng.uniform(-0.3, 0.3, cells.shape)
        at_dim = cells == n
        off[at_dim] = rng.uniform(-0.45, -0.2, int(at_dim.sum()))
        return centres(res, cells) + off * float(np.float32(res))
    ops = [add_world(lay(low, 8)), add_world(lay(high, 9)), add_world(lay(beyond, 10)), CLEAN,
           add_world(lay(np.vstack([low, high, beyond]), 11)), CLEAN]
    return Case("normals whose steps leave the grid; stencils clipped by the grid", res, small_bbox(res), ops)


def count_zero(res):
    """Points 0.42 cells from their cell's centre line along x and along y: at 5 mm that is 2.97 mm from the line through the centre
    along z, outside the 1 mm cylinder, so records exist and have no members: rows of count 0 emit a zero centroid (grid.hpp:472-476).
    (At 1 mm every point of a cell is within 0.71 mm of that line: the same cloud gives members, and no cloud gives such a row
    under a normal along z.)"""
    cells = plate(INNER, INNER, (20,))
    ops = [add_world(centres(res, cells, (0.42, 0.42, 0.0))), CLEAN, add_world(centres(res, cells, (-0.42, 0.42, 0.1))), CLEAN]
    return Case("count-zero rows", res, small_bbox(res), ops)


def gate_20_21(res):
    """Two 5 x 5 plates far apart, one with five cells missing, one with four: the centre cell sees exactly 20 and exactly 21 occupied
    cells, itself included (total > 20, grid.hpp:352)."""
    def patch(cx, missing):
        c = plate(range(cx - 2, cx + 3), range(18, 23), (20,))
        drop = {(cx - 2, 18), (cx + 2, 18), (cx - 2, 22), (cx + 2, 22), (cx - 2, 20)}
        drop = set(list(sorted(drop))[:missing])
        return np.array([v for v in c if (int(v[0]), int(v[1])) not in drop])
    a, b = patch(8, 5), patch(28, 4)
    assert len(a) == 20 and len(b) == 21
    both = np.vstack([a, b])
    ops = [add_world(jittered(res, both, 12)), CLEAN, add_world(jittered(res, both, 13)), CLEAN]
    return Case("gates of exactly 20 and 21 neighbours", res, small_bbox(res), ops)


def boundary_points(res):
    """A plate, and on it points whose x is the f32 nearest to a cell boundary min + i res and its two f32 neighbours, and points whose
    x, y or z is the f32 nearest to a face of the box and its neighbours (strict compares, grid.hpp:644; floor in f64, grid.hpp:633)."""
    cells = plate(INNER, INNER, (20,))
    base = jittered(res, cells, 14)
    r = float(np.float32(res))
    b = np.asarray(small_bbox(res), np.float64)
    lo, hi = b[0::2], b[1::2]
    mid = centres(res, [[20, 20, 20]])[0]
    extra = []
    for i in (7, 8, 19, 30):
        v = np.float32(lo[0] + i * r)
        for x in (np.nextafter(v, np.float32(-1)), v, np.nextafter(v, np.float32(1))):
            for j in (10, 20):
                p = centres(res, [[i, j, 20]])[0]
                p[0] = float(x)
                extra.append(p)
    for axis in range(3):
        for face in (lo[axis], hi[axis]):
            v = np.float32(face)
            for x in (np.nextafter(v, np.float32(-9)), v, np.nextafter(v, np.float32(9))):
                p = mid.copy()
                p[axis] = float(x)
                extra.append(p)
    ops = [add_world(np.vstack([base, np.array(extra)])), CLEAN, add_world(np.vstack([np.array(extra), base])), CLEAN]
    return Case("points on cell boundaries and on the faces of the box", res, small_bbox(res), ops)


def viewpoint_latch(res):
    """A plate seen from above first and from below afterwards, and a second plate seen from below first: a cell's viewpoint is the
    first frame's that touched it (grid.hpp:229), so the normals of the first plate point up and those of the second down."""
    first, second = plate(INNER, INNER, (14,)), plate(INNER, INNER, (26,))
    up = from_above(res)
    ops = [add_world(jittered(res, first, 15), up), add_world(jittered(res, np.vstack([first, second]), 16)), add_world(jittered(res, second, 17), up),
           CLEAN, add_world(jittered(res, np.vstack([first, second]), 18), up), CLEAN]
    return Case("viewpoint latched at first occupancy", res, small_bbox(res), ops)


def erased_key(res):
    """A plate gets its normals; the next frame erases its cells' keys from unprocessed_data_ (grid.hpp:214-215), the frame after finds
    them erased already; then the plate grows by a ring, whose cells and the old rim are the only candidates of the second pass."""
    inner = plate(INNER, INNER, (20,))
    grown = plate(range(3, 34), range(3, 34), (20,))
    ops = [add_world(jittered(res, inner, 19)), CLEAN, add_world(jittered(res, inner, 20)), add_world(jittered(res, inner, 21)),
           add_world(jittered(res, grown, 22)), CLEAN, add_world(jittered(res, grown, 23)), CLEAN]
    return Case("addPoints on cells whose key was erased", res, small_bbox(res), ops)


RANDOM_POINTS, RANDOM_BATCHES = 4000, 10
RANDOM_SLAB = (30, 30, 6)   # cells the random points fall into, from cell (5, 5, 17): about four in ten of them occupied a batch


def random_cloud(res, schedule_seed):
    """RANDOM_POINTS uniform random points in a slab of 30 x 30 x 6 cells, in RANDOM_BATCHES batches, with a clean pass behind a batch
    where a seeded coin says so, and one at the end.  The stencils are random, so are the normals: lines cross, unoccupied cells are
    registered by several records in one pass, and cells are occupied after they were registered."""
    rng = np.random.default_rng(0xA11CE)
    r = float(np.float32(res))
    lo = np.asarray(small_bbox(res), np.float64)[0::2]
    pts = lo + (np.array([5, 5, 17]) + rng.uniform(0, 1, (RANDOM_POINTS, 3)) * np.array(RANDOM_SLAB)) * r
    coin = np.random.default_rng(schedule_seed).uniform(size=RANDOM_BATCHES) < 0.4
    ops = []
    for k, part in enumerate(np.array_split(pts, RANDOM_BATCHES)):
        ops.append(add_world(part))
        if coin[k]:
            ops.append(CLEAN)
    ops.append(CLEAN)
    return Case("random cloud, schedule %d" % schedule_seed, res, small_bbox(res), ops,
                contest="random lines cross: which record keeps an unoccupied cell is the order of the pass, and the cell is occupied later")


def settled_random_cloud(res):
    """The random cloud for the engine: every cell is occupied by the first batch and the later batches (the same cells, other points)
    follow the first clean pass, so no cell is occupied after a pass registered records on it and the order of a pass decides nothing."""
    rng = np.random.default_rng(0xB0B)
    r = float(np.float32(res))
    lo = np.asarray(small_bbox(res), np.float64)[0::2]
    cells = np.unique((np.array([5, 5, 17]) + rng.uniform(0, 1, (RANDOM_POINTS // 2, 3)) * np.array(RANDOM_SLAB)).astype(np.int64), axis=0)
    ops = []
    for k in range(4):
        p = lo + (cells + rng.uniform(0.05, 0.95, cells.shape)) * r
        ops += [add_world(p[rng.permutation(len(p))])] + ([CLEAN] if k in (0, 2) else [])
    ops.append(CLEAN)
    return Case("random cells, occupied before the first pass", res, small_bbox(res), ops)


# ---- the clouds of tests/lattice.py and tests/crafted.py that fit the cap: the dyadic box, 107 x 75 x 90 cells --------------------------

def from_lattice(model):
    ops = [("add", np.asarray(op[1], np.float32).reshape(-1, 4), np.asarray(op[2], np.float64)) if op[0] == "integrate" else CLEAN for op in model.ops]
    return Case("lattice: " + model.name, model.resolution, model.bbox, ops)


def from_crafted(case):
    ops = []
    for op in case.ops:
        if op is crafted.CLEAN:
            ops.append(CLEAN)
        else:
            for f in op.oracle_order():
                ops.append(("add", np.asarray(op.frames[f], np.float32).reshape(-1, 4), np.asarray(op.poses[f], np.float64)))
    return Case("crafted: " + case.name, crafted.RES, crafted.BBOX, ops)


def dyadic_boundary():
    """In the dyadic box every lattice plane is an f32 exactly: a plate, and points EXACTLY on cell boundaries, on the minimum faces and
    on the maximum faces of the box (strict compares: the former belong to the upper cell, the latter two are dropped)."""
    res, bbox = faces.DYADIC_RES, faces.DYADIC_BBOX
    lo, hi = faces.lo_hi(bbox)
    cells = plate(range(30, 60), range(20, 50), (40,))
    rng = np.random.default_rng(24)
    base = lo + (cells + 0.5 + rng.uniform(-0.3, 0.3, cells.shape)) * res
    on = lo + (cells[::7] + 0.5) * res
    on[:, 0] = lo[0] + cells[::7, 0] * res          # exactly on the boundary between cell x - 1 and cell x
    on2 = lo + (cells[3::11] + 0.5) * res
    on2[:, 1] = lo[1] + (cells[3::11, 1] + 1) * res  # exactly on the upper boundary in y
    facep = []
    for axis in range(3):
        for face in (lo[axis], hi[axis]):
            p = lo + (np.array([40.5, 30.5, 40.5])) * res
            p[axis] = face
            facep.append(p)
    pose = crafted.pose_of(False, bbox, lattice.DIMS, res)
    exact = np.vstack([on, on2, np.array(facep)])
    assert (exact.astype(np.float32).astype(np.float64) == exact).all(), "the dyadic points are f32s"
    world = np.vstack([base, exact])
    ops = [add_world(world, pose), CLEAN, add_world(world[::-1], pose), CLEAN]
    return Case("dyadic box: points exactly on cell boundaries and faces", res, bbox, ops)


RESOLUTIONS = (0.001, 0.005)
PER_RESOLUTION = dict(contest=contest, several_normals=several_normals, normal_leaves_grid=normal_leaves_grid, count_zero=count_zero,
                      gate_20_21=gate_20_21, boundary_points=boundary_points, viewpoint_latch=viewpoint_latch, erased_key=erased_key,
                      random_1=lambda r: random_cloud(r, 1), random_2=lambda r: random_cloud(r, 2), random_3=lambda r: random_cloud(r, 3),
                      settled_random=settled_random_cloud)
# the cases whose rows depend on the order of a clean pass BY DESIGN: compared under order_mode=1 only (Case.contest has the reason)
CONTESTS = ("contest", "random_1", "random_2", "random_3")

BUILDERS = {"sphere_1mm": sphere_1mm, "sphere_5mm": sphere_5mm, "plane_1mm": plane_1mm, "plane_5mm": plane_5mm}
for _k, _f in PER_RESOLUTION.items():
    for _r in RESOLUTIONS:
        BUILDERS["%s_%dmm" % (_k, round(_r * 1000))] = (lambda f, r: lambda: f(r))(_f, _r)
BUILDERS.update({
    "dyadic_boundary": dyadic_boundary,
    "lattice_flat": lambda: from_lattice(lattice.flat_model()),
    "lattice_flat_x2_further": lambda: from_lattice(lattice.flat_model(axis=0, layers=2, further=True)),
    "lattice_placement_0": lambda: from_lattice(lattice.placement_model(0, shift=(0.0, 0.0, 0.0))),
    "crafted_full_table": lambda: from_crafted(crafted.full_table("dense")),
    "crafted_pre_dependant_lists": lambda: from_crafted(crafted.pre_dependant_lists("dense")),
})
NAMES = tuple(BUILDERS)
# ... and the cases that turned out to hold the same thing without being built for it
FOUND_CONTESTS = {
    "sphere_1mm": "a real capture: lines of neighbouring records of one pass cross free cells that later frames occupy",
    "lattice_flat_x2_further": "the further layer is laid on cells that both layers of the patch registered on in one pass",
    "crafted_full_table": "the base surface's second epoch occupies layers that the sheets above and below registered on in one pass",
    "crafted_pre_dependant_lists": "as crafted_full_table, and the case then fills exactly those cells",
}
CONTEST_NAMES = tuple(n for n in NAMES if n.rsplit("_", 1)[0] in CONTESTS or n in FOUND_CONTESTS)
CANONICAL_NAMES = tuple(n for n in NAMES if n not in CONTEST_NAMES)

_cases = {}


def case(name):
    """The case of that name, built once."""
    if name not in _cases:
        c = BUILDERS[name]()
        c.contest = c.contest or FOUND_CONTESTS.get(name)
        assert (c.contest is not None) == (name in CONTEST_NAMES), name
        _cases[name] = c
    return _cases[name]
