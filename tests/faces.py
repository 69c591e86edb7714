"""Scenes whose model is cut by all six faces of the grid, and the boundary inputs of the read-outs (imported by tests only).

The synthetic surface (plane z = 0.56 + 0.05 x, sphere r = 0.10 at (0.05, 0, 0.45), a box) sits in the middle of scenes.BBOX_1M,
more than 100 voxels from every face.  The boxes here are cut out of it, so that rows lie in every face layer (index 0 and dim - 1),
occupied cells lie at index == dim (the storage has dim + 1 cells an axis; such a cell never has a row), every window of a read-out
is clipped somewhere, and a triangle or a ray near the model leaves the grid.  Four of the scenes fuse the same surface where a map
frame puts it, 137 m to 1024 m from the origin: an f32 step is 1/131 to 1/16 of a voxel there, so input points, centroids and lattice
points land exactly on cell boundaries and box faces and candidate rows tie for the nearest (boundary_counts, on_lattice_plane,
query_ref.nearest_ties count what each scene contains).  Four more (DEEP) keep the surface and CUT_BBOX's max corner and push the min
corner away until the cell and brick indices are the largest a handle takes; the model then fills a 10^-5 part of the box, so the
input generators below take the box they aim at from the caller, who passes FaceScene.model_box."""
import numpy as np

import scenes

CUT_BBOX = (-0.105, 0.1035, -0.0715, 0.0735, 0.38, 0.5575)
THIN_BBOX = (-0.105, 0.1035, -0.0715, 0.0735, 0.5530, 0.5595)
FAR_SHIFT = (3.2, -1.7, 2.0)
# A box of whole cells at a power-of-two resolution: every lattice plane min + i * res, and every one of them moved by a whole number
# of metres, is an f32 exactly, so transformed points land ON cell boundaries and box faces; (max - min) / res is an exact integer.
DYADIC_RES = 2.0 ** -9
DYADIC_BBOX = tuple(k * DYADIC_RES for k in (-54, 53, -37, 38, 195, 285))
SHIFT_137 = (137.0, -52.0, 23.0)
SHIFT_128 = (128.0, -64.0, 32.0)
SHIFT_1024 = (1024.0, -512.0, 256.0)
SHIFTED_COV = dict(pcl_shifted_cov=True)
# The largest indices: CUT_BBOX's max corner with the min corner pushed away until an axis has DEEP_CELLS cells (the most hfpf_create
# takes: index == dim = 0x1FFFFE then uses all 21 bits of a key field) or every axis DEEP3_CELLS (1579^3 = 3.94e9 directory entries, just
# under the 4.0e9 hfpf_create takes and well over 2^31).  The surface stays at 0.5 m, so coordinates keep full f32 precision: the
# opposite corner of the parameter space from the far* scenes.
DEEP_CELLS = 2097150
DEEP3_CELLS = 12630


def deep_bbox(cells, res=0.002):
    """CUT_BBOX with the min of every axis that has cells[a] > 0 moved to max - (cells[a] + 0.25) * (double)(float)res."""
    r = float(np.float32(res))
    b = list(CUT_BBOX)
    for a, n in enumerate(cells):
        if n:
            b[2 * a] = b[2 * a + 1] - (n + 0.25) * r
    return tuple(b)


# name -> (bbox, resolution, shift of the fusion frame, dims, config of engine and oracle)
DEFS = {"cut": (CUT_BBOX, 0.002, (0.0, 0.0, 0.0), (104, 72, 88), {}),
        "cut3": (CUT_BBOX, 0.003, (0.0, 0.0, 0.0), (69, 48, 59), {}),
        "thin": (THIN_BBOX, 0.001, (0.0, 0.0, 0.0), (208, 144, 6), {}),
        "far": (CUT_BBOX, 0.002, FAR_SHIFT, (104, 72, 88), {}),
        # 137 m out an f32 step is 1.5e-5 m, 1/131 of a voxel.  With the default (single-pass f32) covariance the normals of far137
        # are rounding noise, as the reference's would be: arbitrary but deterministic, so any change in operation order shows
        "far137": (CUT_BBOX, 0.002, SHIFT_137, (104, 72, 88), {}),
        "far137s": (CUT_BBOX, 0.002, SHIFT_137, (104, 72, 88), SHIFTED_COV),
        "dy128s": (DYADIC_BBOX, DYADIC_RES, SHIFT_128, (107, 75, 90), SHIFTED_COV),
        "dy1024s": (DYADIC_BBOX, DYADIC_RES, SHIFT_1024, (107, 75, 90), SHIFTED_COV),
        "deepx": (deep_bbox((DEEP_CELLS, 0, 0)), 0.002, (0.0, 0.0, 0.0), (DEEP_CELLS, 72, 88), {}),
        "deepy": (deep_bbox((0, DEEP_CELLS, 0)), 0.002, (0.0, 0.0, 0.0), (104, DEEP_CELLS, 88), {}),
        "deepz": (deep_bbox((0, 0, DEEP_CELLS)), 0.002, (0.0, 0.0, 0.0), (104, 72, DEEP_CELLS), {}),
        "deep3": (deep_bbox((DEEP3_CELLS,) * 3), 0.002, (0.0, 0.0, 0.0), (DEEP3_CELLS,) * 3, {})}
ALL = tuple(DEFS)
NAMES = ("cut", "cut3", "thin", "far", "far137s", "dy128s")   # every read-out
HOT_NAMES = ("far137", "dy1024s")                              # hot path, query and mesh only
SIX = ("cut", "cut3", "far", "far137", "far137s")   # the scenes every face of which cuts a surface, with cells at index == dim
DYADIC = ("dy128s", "dy1024s")                      # every face cuts a surface; a box of whole cells has no cell at index == dim
SHIFTED = ("far", "far137", "far137s", "dy128s", "dy1024s")
DEEP = ("deepx", "deepy", "deepz", "deep3")          # the model in the max corner of a grid with the largest indices
DEEP_AXES = {"deepx": (0,), "deepy": (1,), "deepz": (2,), "deep3": (0, 1, 2)}
# what the CPU oracle alone gives (asserted exactly in test_faces_ref.py only): rows, live rows, live rows in the layers
# x=0, x=dim-1, y=0, y=dim-1, z=0, z=dim-1, occupied cells at index == dim per axis
ORACLE_TABLE = {"cut": (10087, 9872, (140, 45, 132, 114, 291, 260), (42, 216, 1358)),
                "cut3": (5185, 4812, (66, 22, 76, 78, 174, 388), (36, 143, 582)),
                "thin": (5230, 5230, (0, 0, 33, 8, 0, 272), (0, 66, 97)),
                "far": (10087, 9897, (140, 45, 132, 112, 290, 255), (42, 216, 1358)),
                "far137": (10085, 10011, (140, 45, 128, 111, 275, 252), (42, 216, 1357)),
                "far137s": (10085, 9863, (140, 45, 132, 114, 291, 258), (42, 216, 1357)),
                "dy128s": (13871, 13583, (145, 43, 194, 170, 300, 681), (0, 0, 0)),
                "dy1024s": (13462, 13175, (145, 47, 186, 152, 297, 682), (0, 0, 0)),
                # rows at ix 2096923..2097149 / iy 2096998..2097149 / iz 2097045..2097149 / 12403..12629, 12472.., 12525..; largest
                # linear brick index of a row 3.1e7, 4.1e7, 3.4e7 and 3,936,827,528 (every row of deep3 lies above 2^31)
                "deepx": (19967, 19464, (0, 45, 240, 215, 291, 260), (42, 335, 1358)),
                "deepy": (14618, 14263, (196, 53, 0, 116, 351, 1291), (49, 158, 3582)),
                "deepz": (18171, 17912, (109, 150, 169, 153, 0, 820), (107, 209, 975)),
                "deep3": (45342, 44294, (0, 162, 0, 206, 0, 2972), (117, 211, 2409))}
# boundary_counts() of the dyadic scenes (asserted exactly in test_faces_ref.py only): in-box input points, those of them on an exact
# cell boundary, used points exactly on the plane of a box face
BOUNDARY_TABLE = {"dy128s": (58260, 729, 96), "dy1024s": (58121, 5838, 866)}
# half of the last two, as the floor check_conditions holds every session to
BOUNDARY_FLOOR = {"dy128s": (360, 48), "dy1024s": (2900, 430)}
Z_CLIP = (0.28, 0.6)   # the default z-clip of engine and oracle
# Per option set of test_gpu_faces.QUERY_OPTS, half of query_ref.nearest_ties(...).sum() over query_points() on the oracle's exact rows
# alone: far137 gives 0, 5, 10, 12, 12, 10, 7 and far137s 0, 949, 1367, 1524, 1615, 1366, 1187 (radius 0 has one candidate a point).
# Point and centroid are f32s of spacing 2^-16 (x), 2^-18 (y), 2^-19 m (z) there, so d2 is a sum of three small integer squares scaled
# by powers of two, and equal sums are common.
TIE_FLOOR = {"far137": (0, 2, 5, 6, 6, 5, 3), "far137s": (0, 474, 683, 762, 807, 683, 593)}


class FaceScene(scenes.Scene):
    """scenes.Scene(8, 320, 240, res, bbox, clean_every=4) with the default seeds.  Every frame is rendered from the scene's own
    pose; it is integrated with the same rotation and the translation moved by `shift`, into the box moved by the same amount: the
    same surface, fused elsewhere (the z-clip acts in the camera frame and does not notice)."""

    def __init__(self, name):
        bbox, res, shift, dims, config = DEFS[name]
        moved = tuple(float(b) + float(shift[i // 2]) for i, b in enumerate(bbox))
        super().__init__(8, 320, 240, res, bbox=moved, clean_every=4)
        self.name, self.dims, self.shift, self.config = name, dims, np.asarray(shift, np.float64), dict(config)
        # where the model is, for the input generators below to aim at: a deep scene's model fills a 10^-5 part of its box.  What the
        # box means (IN_BBOX, the faces, the lattice) is always taken from bbox
        self.model_box = CUT_BBOX if name in DEEP else moved
        self.render_poses = self.poses
        self.poses = [np.hstack([p[:, :3], p[:, 3:] + self.shift.reshape(3, 1)]) for p in self.render_poses]

    def frame(self, f):
        import hfpf_synth as S
        return S.frame(self.seed, f, self.W, self.H, self.render_poses[f], noise_sigma=self.noise, nan_permille=self.nan_permille,
                       fx=self.fx, layout=self.layout)


def face_counts(rows, occ, dims):
    """(rows, live rows, live rows in the six face layers, occupied cells at index == dim per axis)."""
    live = rows[rows["count"] > 0]
    layers = []
    for a, k in enumerate(("ix", "iy", "iz")):
        layers += [int((live[k] == 0).sum()), int((live[k] == dims[a] - 1).sum())]
    occ = np.asarray(occ).reshape(-1, 3)
    return len(rows), len(live), tuple(layers), tuple(int((occ[:, a] == dims[a]).sum()) for a in range(3))


def check_conditions(name, rows, occ, dims):
    """The conditions a session must meet before it is used: without them its tests would pass without touching a face."""
    assert tuple(dims) == DEFS[name][3], "%s: dims %r" % (name, dims)
    n, n_live, layers, at_dim = face_counts(rows, occ, dims)
    print("%s: %d rows / %d live; face layers %r; occupied at index == dim %r" % (name, n, n_live, layers, at_dim))
    for k in ("ix", "iy", "iz"):
        assert (rows[k] >= 0).all(), "a row with a negative index"
    for a, k in enumerate(("ix", "iy", "iz")):
        assert (rows[k] < dims[a]).all(), "a row at index >= dim was emitted"
    if name in SIX:
        assert min(layers) >= 20, "%s: a face layer holds fewer than 20 live rows: %r" % (name, layers)
        assert min(at_dim) >= 1, "%s: an axis without an occupied cell at index == dim: %r" % (name, at_dim)
    elif name in DYADIC:
        # max = min + dim * res exactly: a point of cell dim would have p >= max, and the strict box test drops it
        assert min(layers) >= 20, "%s: a face layer holds fewer than 20 live rows: %r" % (name, layers)
        assert at_dim == (0, 0, 0), "%s: a box of whole cells with an occupied cell at index == dim: %r" % (name, at_dim)
        n_in, on_cell, on_face = boundary_counts(FaceScene(name))
        print("%s: %d input points in the box, %d on an exact cell boundary, %d exactly on a face's plane" % (name, n_in, on_cell, on_face))
        assert on_cell >= BOUNDARY_FLOOR[name][0] and on_face >= BOUNDARY_FLOOR[name][1], "%s: %r" % (name, (n_in, on_cell, on_face))
    elif name in DEEP:
        # without these a later change of a constant turns the deep tests vacuous: the widths are hfpf_create's own (key_widths)
        widths = key_widths(dims)
        lin = brick_lin(rows, dims)
        print("%s: key widths %r, Morton width %d, largest linear brick index of a row %d (%d rows above 2^31)" % (
            name, widths, 3 * max(widths), lin.max(), (lin > 2 ** 31).sum()))
        for a in DEEP_AXES[name]:
            k = ("ix", "iy", "iz")[a]
            assert layers[2 * a + 1] >= 20, "%s: the max layer of axis %d holds fewer than 20 live rows: %r" % (name, a, layers)
            assert int(rows[k].max()) == dims[a] - 1, "%s: no row at index dim - 1 of axis %d" % (name, a)
            assert at_dim[a] >= 1, "%s: axis %d without an occupied cell at index == dim: %r" % (name, a, at_dim)
            assert layers[2 * a] == 0 and int(rows[k].min()) > 0, "%s: the min layer of axis %d is not empty" % (name, a)
        if name == "deep3":
            assert prod_bdims(dims) > 2 ** 31 and lin.max() > 2 ** 31 and (lin > 2 ** 31).sum() >= 1000, "%s: brick indices below 2^31" % name
        else:
            assert widths[DEEP_AXES[name][0]] == KEY_FIELD_BITS, "%s: the deep axis' key field has %r bits" % (name, widths)
            assert 3 * max(widths) == 63, "%s: Morton width %d" % (name, 3 * max(widths))
    else:
        assert dims[2] < 8 and layers[2] > 0 and layers[3] > 0 and layers[5] > 0, "%s: %r %r" % (name, dims, layers)
    return layers, at_dim


KEY_FIELD_BITS = 21   # bits of a key field at the largest grid (tables.hpp, query_ref.KEY_BITS)


def key_widths(dims):
    """Per axis, the bits that hold 0..dim (the storage has dim + 1 cells an axis): hfpf_create's bits_for, restated.  A handle's
    cell key is x << (wy + wz) | y << wz | z, and the candidates of a clean pass are sorted over 3 * max(widths) bits of Morton code."""
    return tuple(max(1, int(d).bit_length()) for d in dims)


def brick_dims(dims):
    return tuple((int(d) + 1 + 7) // 8 for d in dims)


def prod_bdims(dims):
    b = brick_dims(dims)
    return b[0] * b[1] * b[2]


def brick_lin(rows, dims):
    """Per row, the linear index of its 8 x 8 x 8 brick in the directory, (bx * bdim_y + by) * bdim_z + bz, as int64."""
    b = brick_dims(dims)
    return (rows["ix"].astype(np.int64) // 8 * b[1] + rows["iy"].astype(np.int64) // 8) * b[2] + rows["iz"].astype(np.int64) // 8


def boundary_counts(scene):
    """(input points in the box, those of them with a coordinate exactly on a cell boundary, used points with a coordinate exactly on
    the plane of a box face) over the scene's frames, with no engine or oracle: integrate's transform restated (f64 from the widened
    f32 input, left to right, one rounding to f32; query_ref.transform), its z-clip in the camera frame and its strict box test.  p -
    min is exact in f64, so for a power-of-two resolution "the quotient is a whole number" is decided exactly; the points on a face's
    plane fail the strict test and are not among the first figure."""
    import query_ref as Q
    lo, hi = lo_hi(scene.bbox)
    res = float(np.float32(scene.resolution))   # engine and oracle keep (double)(float)resolution
    lay = scene.layout
    n_in = on_cell = on_face = 0
    for f in range(scene.n_frames):
        rec = np.frombuffer(scene.frame(f), np.uint8).reshape(-1, lay["point_step"])
        xyz = np.stack([rec[:, lay[k]:lay[k] + 4].copy().view(np.float32)[:, 0] for k in ("off_x", "off_y", "off_z")], axis=1)
        xyz = xyz[Q.used(xyz, True, Z_CLIP)]
        p = Q.transform(scene.poses[f], xyz).astype(np.float64)
        inside = ((p > lo) & (p < hi)).all(axis=1)
        q = (p - lo) / res
        n_in += int(inside.sum())
        on_cell += int((inside & (q == np.floor(q)).any(axis=1)).sum())
        on_face += int(((p == lo) | (p == hi)).any(axis=1).sum())
    return n_in, on_cell, on_face


def on_lattice_plane(p, bbox, res):
    """Per (n, 3) f32 point: whether a coordinate lies exactly on a lattice plane min + i * res (decided exactly where p - min and the
    division by res are exact in f64: a power-of-two resolution), and the exact integer quotients floor((p - min) / res)."""
    lo, _ = lo_hi(bbox)
    q = (np.asarray(p, np.float32).astype(np.float64) - lo) / float(res)
    return (q == np.floor(q)).any(axis=1), np.floor(q).astype(np.int64)


def in_face_layer(vox, dims):
    """Per (n, 3) voxel: whether it lies in one of the six face layers."""
    v = np.asarray(vox, np.int64).reshape(-1, 3)
    d = np.asarray(dims, np.int64)
    return ((v == 0) | (v == d - 1)).any(axis=1)


def lo_hi(bbox):
    b = np.asarray(bbox, np.float64)
    return b[0::2], b[1::2]


def centroids(rows):
    return np.stack([rows["x"], rows["y"], rows["z"]], axis=1)


# ---- a. query points ----------------------------------------------------------------------------------------------------

def lattice_values(bbox, res, dims, axis):
    """(float)(min + i * res) for i in {0, 1, dim-1, dim, dim+1} and the f32 neighbours on both sides of each: 15 f32 values that
    land on cell boundaries and on the two faces of `axis`."""
    lo = float(bbox[2 * axis])
    d = int(dims[axis])
    c = np.array([lo + i * float(res) for i in (0, 1, d - 1, d, d + 1)], np.float64).astype(np.float32)
    return np.concatenate([np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))])


def query_points(rows, bbox, res, dims, seed=0xFACE, per_face=5000, per_value=400):
    """About 60,000 f32 points (identity pose): every live row's centroid jittered by N(0, one voxel); per face a sheet of random
    points within +-5 voxels of it, on both sides; the lattice values of every axis crossed with random positions on the others."""
    rng = np.random.default_rng(seed)
    lo, hi = lo_hi(bbox)
    res = float(res)
    live = rows[rows["count"] > 0]
    out = [(centroids(live).astype(np.float64) + rng.normal(0.0, res, (len(live), 3))).astype(np.float32)]
    for axis in range(3):
        for face in (lo[axis], hi[axis]):
            p = rng.uniform(lo - 5 * res, hi + 5 * res, (per_face, 3))
            p[:, axis] = face + rng.uniform(-5 * res, 5 * res, per_face)
            out.append(p.astype(np.float32))
    for axis in range(3):
        vals = lattice_values(bbox, res, dims, axis)
        p = rng.uniform(lo - 2 * res, hi + 2 * res, (len(vals) * per_value, 3)).astype(np.float32)
        p[:, axis] = np.repeat(vals, per_value)
        out.append(p)
    return np.ascontiguousarray(np.vstack(out))


# ---- c. rays ------------------------------------------------------------------------------------------------------------

def ray_t_max(bbox, res, step=0.5, max_samples=400):
    """A march long enough to cross the whole box from 0.05 m outside it, cut to ~max_samples samples."""
    lo, hi = lo_hi(bbox)
    return float(min(np.linalg.norm(hi - lo) + 0.06, max_samples * step * float(res)))


def ray_sets(bbox, res, seed=0xFACE + 1):
    """[(label, (n, 6) f32 rays {o, d})], about 3000 rays in all (identity pose): from 0.05 m outside each face at points inside;
    axis-parallel (two rates exactly 0) through random points; in each face's plane and one f32 step inside and outside it; from
    inside the box outwards; past the box altogether, some parallel to a face 1 mm outside it."""
    rng = np.random.default_rng(seed)
    lo, hi = lo_hi(bbox)
    span = hi - lo
    sets = []

    def inside(n):
        return rng.uniform(lo, hi, (n, 3))

    def add(label, parts):
        sets.append((label, np.ascontiguousarray(np.vstack(parts).astype(np.float32))))

    out = []
    for axis in range(3):                                  # 6 x 150 from outside a face, aimed at points inside
        for side, face in ((-1.0, lo[axis]), (1.0, hi[axis])):
            o = rng.uniform(lo - 0.02, hi + 0.02, (150, 3))
            o[:, axis] = face + side * 0.05
            out.append(np.hstack([o, inside(150) - o]))
    add("from outside a face", out)
    out = []
    for axis in range(3):                                  # 6 x 100 axis-parallel, entering through a face
        for sign in (1.0, -1.0):
            o = inside(100)
            o[:, axis] = (lo[axis] - 0.01) if sign > 0 else (hi[axis] + 0.01)
            d = np.zeros((100, 3))
            d[:, axis] = sign
            out.append(np.hstack([o, d]))
    add("axis-parallel", out)
    out = []
    for axis in range(3):                                  # 6 faces x 3 planes x 30 rays lying in the plane
        for face in (lo[axis], hi[axis]):
            f = np.float32(face)
            for plane in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
                o = rng.uniform(lo - 0.01, hi + 0.01, (30, 3))
                o[:, axis] = float(plane)
                d = inside(30) - o
                d[:, axis] = 0.0
                out.append(np.hstack([o, d]))
    add("in a face's plane", out)
    o = inside(500)                                        # from inside, leaving the box
    add("from inside", [np.hstack([o, rng.normal(size=(500, 3))])])
    c = (lo + hi) / 2                                      # 300 that miss the box: pointing away from outside it
    d = rng.normal(size=(300, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out = [np.hstack([c + d * (span * 0.6 + 0.02), d + rng.normal(0, 0.2, d.shape)])]
    for axis in range(3):                                  # 6 x 30 parallel to a face, 1 mm outside it
        for side, face in ((-1.0, lo[axis]), (1.0, hi[axis])):
            o = rng.uniform(lo - 0.01, hi + 0.01, (30, 3))
            o[:, axis] = face + side * 0.001
            d = inside(30) - o
            d[:, axis] = 0.0
            out.append(np.hstack([o, d]))
    add("past the box", out)
    return sets


def rays(bbox, res, seed=0xFACE + 1):
    return np.ascontiguousarray(np.vstack([r for _, r in ray_sets(bbox, res, seed)]))


def face_pairs(bbox, res, n=60, step=0.5, seed=0xFACE + 2, model_box=None):
    """Per face, n pairs of axis-parallel rays on one line, pointing inwards: [(outer rays, inner rays, m, offset in t)].  The inner
    ray starts on the face's plane (the f32 nearest to it), the outer one m march steps of `step` voxels before it, with the smallest
    m in 16..256 for which that origin is an f32 exactly: then sample k + m of the outer ray and sample k of the inner one are the same
    f64 sums, and the same f32 point.  A face without such an m is left out (the z faces of `thin`: a step of 0.5 mm has bits 2^10
    times finer than the f32 spacing at 0.55 m).  The faces are those of bbox (before a plane inside the grid the outer ray could meet a
    surface the inner one never sees); the lines run through random points of model_box (bbox by default)."""
    rng = np.random.default_rng(seed)
    lo, hi = lo_hi(bbox)
    mlo, mhi = lo_hi(bbox if model_box is None else model_box)
    dt = float(step) * float(res)
    out = []
    for axis in range(3):
        for sign, face in ((1.0, lo[axis]), (-1.0, hi[axis])):
            f = float(np.float32(face))
            m = next((m for m in range(16, 257) if float(np.float32(f - sign * (m * dt))) == f - sign * (m * dt)), None)
            if m is None:
                continue
            assert (f - sign * (m * dt)) + sign * (m * dt) == f
            o = rng.uniform(mlo, mhi, (n, 3)).astype(np.float32)
            d = np.zeros((n, 3), np.float32)
            d[:, axis] = sign
            o[:, axis] = np.float32(f)
            inner = np.hstack([o, d])
            o = o.copy()
            o[:, axis] = np.float32(f - sign * (m * dt))
            out.append((np.hstack([o, d]), inner, m, m * dt))
    return out


def outside_view(bbox, W=160, H=120, max_face=False):
    """(pose, K) of a camera 0.08 m outside the z-min face, looking along +z through it at the whole box; with max_face, outside the
    z-max face looking along -z (half a turn about x)."""
    lo, hi = lo_hi(bbox)
    c = (lo + hi) / 2
    if max_face:
        pose = np.hstack([np.diag([1.0, -1.0, -1.0]), np.array([[c[0]], [c[1]], [hi[2] + 0.08]])])
    else:
        pose = np.hstack([np.eye(3), np.array([[c[0]], [c[1]], [lo[2] - 0.08]])])
    f = 0.08 * W / (hi[0] - lo[0]) * 0.8   # the z-min face fills the image and a little of its surroundings
    return pose, (f, f, (W - 1) / 2.0, (H - 1) / 2.0)


# ---- e. meshes ----------------------------------------------------------------------------------------------------------

def huge_quad(bbox):
    """Two triangles under an oblique pose through the centre of the box, six times its longest side across (as the quad of
    test_gpu_deviation is to the 1 m box): they leave the grid on every side."""
    lo, hi = lo_hi(bbox)
    h = 3.0 * float((hi - lo).max())
    quad = np.array([[-h, -h, 0], [h, -h, 0], [h, h, 0], [-h, h, 0]], np.float32)
    a, b = 0.4, 0.3
    R = (np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]]) @
         np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]]))
    return quad, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.hstack([R, ((lo + hi) / 2).reshape(3, 1)])


def near_faces(p, bbox, res):
    """Per face (x-min, x-max, y-min, y-max, z-min, z-max) the number of points p (n, 3) within one voxel of it.  A lattice plane
    on a face is never IN_BBOX, so cubes touching it stay open (include/hfpf.h); lattice plane 0 is (float)bbox_min, which is on or
    outside the min face unless the rounding went inwards.  Where it did not, the outermost cube that can be meshed is cube 1, and the
    count is of the points within one voxel of lattice plane 1 instead."""
    lo, hi = lo_hi(bbox)
    p = np.asarray(p, np.float64)
    res = float(res)
    out = []
    for a in range(3):
        i0 = 0 if float(np.float32(lo[a])) > lo[a] else 1
        out += [int((p[:, a] <= lo[a] + (i0 + 1) * res).sum()), int((p[:, a] >= hi[a] - res).sum())]
    return out


def shift_pose(voxels, res):
    return np.hstack([np.eye(3), (np.asarray(voxels, np.float64) * float(res)).reshape(3, 1)])


def outside_own_cell(rows, bbox, res, dims):
    """Live rows in a face layer whose centroid does not lie in the cell of their own voxel index (the centroid of a voxel's members
    is a mean of projections onto a line, not of points of the cell)."""
    lo, _ = lo_hi(bbox)
    live = rows[rows["count"] > 0]
    cell = np.floor((centroids(live).astype(np.float64) - lo) / float(res)).astype(np.int64)
    vox = np.stack([live["ix"], live["iy"], live["iz"]], axis=1).astype(np.int64)
    return live[(cell != vox).any(axis=1) & in_face_layer(vox, dims)]
