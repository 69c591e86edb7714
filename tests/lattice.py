"""Models that lie exactly along the grid, and the stencils the plane fit degenerates on (imported by tests only).

Every other scene fuses a noisy synthetic surface; here the occupied cells are chosen one by one.  A cloud has one point per cell
and frame, at the cell centre plus a uniform jitter of +-0.3 voxels, seen by a camera without rotation that stands 0.3125 m below
the box's minimum corner (camera-frame z 0.3125 .. 0.49 in the dyadic box of tests/faces.py: inside the default z-clip).  In that box
every cell centre is an f32 exactly, so far from the origin the single-pass f32 covariance of a flat stencil cancels, the normals
become arbitrary and some come out as 0/0: NaN in all three components.  A stencil with fewer than three cells has no fit at all
and keeps a zero normal (gates below 2 let such cells through).  Either row has count == 0: nothing lies within a cylinder about a
NaN or zero-length line."""
import numpy as np

import faces

DIMS = (107, 75, 90)   # of faces.DYADIC_BBOX at faces.DYADIC_RES
OFFSETS = np.stack(np.meshgrid(np.arange(-2, 3), np.arange(-2, 3), np.arange(-2, 3), indexing="ij"), -1).reshape(125, 3)  # setK order
CAMERA_DEPTH = 0.3125
QUIET_NAN = 0x7FC00000
NORMAL_COLUMNS = ("nx", "ny", "nz")


def _families():
    x, y, z = OFFSETS[:, 0], OFFSETS[:, 1], OFFSETS[:, 2]
    cheb = np.abs(OFFSETS).max(axis=1)
    fam = {
        "single": cheb == 0,
        "pair": (y == 0) & (z == 0) & ((x == 0) | (x == 1)),
        "line_x": (y == 0) & (z == 0),
        "line_y": (x == 0) & (z == 0),
        "line_z": (x == 0) & (y == 0),
        "line_diag": (x == y) & (y == z),
        "plane_x0": x == 0,
        "plane_y0": y == 0,
        "plane_z0": z == 0,
        "plane_xy": x == y,
        "plane_xyz": x + y + z == 0,
        "slab2": (z == 0) | (z == 1),
        "slab3": np.abs(z) <= 1,
        "planes_z2": np.abs(z) == 2,
        "half": z <= 0,
        "octant": (x >= 0) & (y >= 0) & (z >= 0),
        "cross": (x == 0) | (y == 0),
        "corner": (x == 0) | (y == 0) | (z == 0),
        "shell": cheb == 2,
        "checker": (x + y + z) % 2 == 0,
        "cube": cheb >= 0,
    }
    return {k: np.ascontiguousarray(v.astype(np.uint8)) for k, v in fam.items()}


FAMILIES = _families()   # name -> 125-byte mask in setK order (x outermost, z innermost)
SYMMETRIC = ("plane_x0", "plane_y0", "plane_z0", "plane_xy", "plane_xyz", "slab2", "slab3", "planes_z2", "cross")
GATE20 = tuple(k for k, m in FAMILIES.items() if int(m.sum()) > 20)   # the centre of such a stencil passes the default gate


def moved(bbox, shift):
    return tuple(float(b) + float(shift[i // 2]) for i, b in enumerate(bbox))


def place(family, centre):
    """The cells of a family's stencil around `centre`, (n, 3) int64."""
    return np.asarray(centre, np.int64) + OFFSETS[FAMILIES[family] != 0]


def sites(pitch=10, first=5, dims=DIMS):
    """Stencil centres `pitch` cells apart: with 5-cell stencils at least 5 free cells lie between two of them, so that no cell of
    one is in the 5 x 5 x 5 window of a cell of another."""
    ax = [np.arange(first, d - 2, pitch) for d in dims]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def cloud(bbox, res, cells, jitter=0.3, frames=1, seed=0):
    """(frames, pose): `frames` arrays of packed 16-byte records (x, y, z, rgb), one point per cell each, in the frame of the camera
    described above, and the camera's pose (3 x 4, camera -> fusion frame).  Reproducible from the seed."""
    rng = np.random.default_rng(seed)
    cells = np.asarray(cells, np.float64).reshape(-1, 3)
    lo, _ = faces.lo_hi(bbox)
    out = []
    for _ in range(frames):
        rec = np.zeros((len(cells), 4), np.float32)
        local = (cells + 0.5 + rng.uniform(-jitter, jitter, cells.shape)) * float(res)
        local[:, 2] += CAMERA_DEPTH
        rec[:, :3] = local
        out.append(np.ascontiguousarray(rec))
    pose = np.hstack([np.eye(3), (lo - np.array([0.0, 0.0, CAMERA_DEPTH])).reshape(3, 1)])
    return out, pose


class Model:
    """A box, a configuration of engine and oracle, and a schedule [('integrate', records, pose) | ('clean',), ...]."""

    def __init__(self, name, shift, config, epochs, dims=DIMS):
        self.name, self.shift, self.config, self.dims = name, tuple(shift), dict(config), dims
        self.resolution = faces.DYADIC_RES
        self.bbox = moved(faces.DYADIC_BBOX, shift)
        self.ops = []
        self.cells = np.zeros((0, 3), np.int64)
        for n, (cells, frames) in enumerate(epochs):
            recs, pose = cloud(self.bbox, self.resolution, cells, frames=frames, seed=0x1A77 + n)
            self.ops += [("integrate", r, pose) for r in recs] + [("clean",)]
            self.cells = np.unique(np.vstack([self.cells, np.asarray(cells, np.int64)]), axis=0)
        self.pose = pose
        self.max_points = max(len(op[1]) for op in self.ops if op[0] == "integrate")

    def run(self, grid, capture_name, upto=None):
        """Drives an oracle grid ('capture') or an engine grid ('integrate') through the first `upto` steps (all by default)."""
        for op in self.ops[:upto]:
            if op[0] == "integrate":
                getattr(grid, capture_name)(op[1], op[2])
            else:
                grid.clean()


FURTHER_WIDTH = 8   # the further layer is a strip of the patch this wide: a model keeps to 5000 rows


def _patch(axis, layers, first=0, size=48, at=(33, 17, 41), width=None):
    """The cells of a size x size patch normal to `axis`, `layers` thick from layer `first`; with `width`, a strip of it that wide
    along the next axis."""
    span = [np.arange(size) + at[a] for a in range(3)]
    span[axis] = np.arange(first, first + layers) + at[axis]
    if width:
        span[(axis + 1) % 3] = span[(axis + 1) % 3][:width]
    return np.stack(np.meshgrid(*span, indexing="ij"), -1).reshape(-1, 3)


def flat_model(shift=(0.0, 0.0, 0.0), axis=2, layers=1, shifted_cov=False, further=False, name=None):
    """The flat patch: 3 frames, clean, 2 frames, clean; with `further`, one more frame that adds a further layer beside the patch (a strip
    FURTHER_WIDTH wide), and a third clean, so that cells which hold a NaN normal sit in the stencils of new candidates."""
    p = _patch(axis, layers)
    epochs = [(p, 3), (p, 2)] + ([(_patch(axis, 1, first=layers, width=FURTHER_WIDTH), 1)] if further else [])
    name = name or "flat %s%d at %r%s" % ("xyz"[axis], layers, tuple(shift), ", shifted cov" if shifted_cov else "")
    return Model(name, shift, dict(pcl_shifted_cov=True) if shifted_cov else {}, epochs)


LOW_GATE_SINGLES, LOW_GATE_PAIRS, LOW_GATE_LINES = 12, 8, 10   # lines: of each of the four directions


def low_gate_cells():
    """Isolated single cells, pairs and five-cell lines along x, y, z and the space diagonal, each on a site of its own."""
    kinds = ["single"] * LOW_GATE_SINGLES + ["pair"] * LOW_GATE_PAIRS
    for k in ("line_x", "line_y", "line_z", "line_diag"):
        kinds += [k] * LOW_GATE_LINES
    s = sites()
    pick = np.random.default_rng(0x10E).permutation(len(s))[:len(kinds)]
    return np.vstack([place(k, s[i]) for k, i in zip(kinds, pick)])


def low_gate_model(gate, further=False):
    c = low_gate_cells()
    epochs = [(c, 3), (c, 2)]
    if further:  # one more cell beside every cell, along y
        epochs.append((np.unique(c + np.array([0, 1, 0]), axis=0), 1))
    return Model("low gate %d" % gate, (0.0, 0.0, 0.0), dict(gate=gate), epochs)


PLACEMENT_PARTS = 4  # the families are dealt to this many models, each within 5000 rows


def placement_cells(part=None, dims=DIMS):
    """(cells, [(family, centre)]) of the families GATE20[part::PLACEMENT_PARTS] (all of them without a part).  Every family that
    passes gate 20 with its centre at local brick indices 0 and 7 on every axis (all eight corners), and once with the centre two
    cells from a grid face: neighbourhood() assembles known patterns across brick and box borders.  Sites are 16
    cells apart (centres 16 i + 8 or 16 i + 7); the last row of sites along y holds the face placements, centre at dim - 3 (the x
    sites at either end lie two cells from the x faces as well)."""
    nx, ny, nz = ((d - 11) // 16 + 1 for d in dims)   # centres 16 i + 8 <= dim - 3
    grid_sites = [(i, j, k) for j in range(ny - 1) for k in range(nz) for i in range(nx)]
    face_sites = [(i, ny - 1, k) for k in range(nz) for i in range(nx)]
    out, centres = [], []
    mine = GATE20 if part is None else GATE20[part::PLACEMENT_PARTS]
    for m, fam in enumerate(GATE20):
        for corner in range(8):
            if fam not in mine:
                continue
            i, j, k = grid_sites[8 * m + corner]
            c = np.array([16 * i + 8, 16 * j + 8, 16 * k + 8]) - np.array([(corner >> 2) & 1, (corner >> 1) & 1, corner & 1])
            assert all(int(v) % 8 in (0, 7) for v in c)
            out.append(place(fam, c))
            centres.append((fam, tuple(int(v) for v in c)))
    for m, fam in enumerate(GATE20):
        if fam not in mine:
            continue
        i, j, k = face_sites[m]
        c = np.array([2 if i == 0 else min(16 * i + 8, dims[0] - 3), dims[1] - 3, 2 if k == 0 else 16 * k + 8])
        out.append(place(fam, c))
        centres.append((fam, tuple(int(v) for v in c)))
    cells = np.vstack(out)
    assert (cells >= 0).all() and (cells < np.asarray(dims)).all() and len(np.unique(cells, axis=0)) == len(cells)
    return cells, centres


def placement_model(part, shift=faces.SHIFT_128, further=False):
    c, _ = placement_cells(part)
    epochs = [(c, 3), (c, 2)]
    if further:  # every stencil again, five cells up: a 5 x 5 x 10 block at each site
        epochs.append((np.unique(c + np.array([0, 0, 5]), axis=0), 1))
    return Model("placement %d at %r" % (part, tuple(shift)), shift, {}, epochs)


# ---- NaN and zero normals -------------------------------------------------------------------------------------------------------------

def nan_mask(rows):
    return np.isnan(rows["nx"]) | np.isnan(rows["ny"]) | np.isnan(rows["nz"])


def zero_mask(rows):
    return (rows["nx"] == 0) & (rows["ny"] == 0) & (rows["nz"] == 0)


def canonical_nans(rows):
    """A copy of the rows in which every NaN in nx, ny, nz has the bits 0x7FC00000: sign and payload of a NaN are unspecified."""
    out = np.array(rows, copy=True)
    for f in NORMAL_COLUMNS:
        col = np.ascontiguousarray(out[f])
        bits = col.view(np.uint32)
        bits[np.isnan(col)] = QUIET_NAN
        out[f] = col
    return out


def nan_patterns(rows):
    """The distinct bit patterns of the NaNs in nx, ny, nz, as sorted hex strings."""
    bits = np.concatenate([np.ascontiguousarray(rows[f]).view(np.uint32)[np.isnan(rows[f])] for f in NORMAL_COLUMNS])
    return ["0x%08X" % b for b in np.unique(bits)]


def normal_counts(rows):
    """(rows, NaN-normal rows, zero-normal rows, rows with a component above 0.99 per axis)."""
    big = tuple(int((np.abs(rows[f]) > 0.99).sum()) for f in NORMAL_COLUMNS)
    return len(rows), int(nan_mask(rows).sum()), int(zero_mask(rows).sum()), big


# ---- the leaf: stencils handed to the plane fit directly ------------------------------------------------------------------------------

# (resolution, bbox): the 1 mm and 5 mm boxes of the leaf tests, and the three boxes of tests/faces.py in a map frame
LEAF_BOXES = {"1mm": (0.001, (-0.5, 0.5, -0.5, 0.5, 0.0, 1.0)),
              "5mm": (0.005, (-0.80, 1.80, -1.5, 1.5, 0.0, 1.0)),
              "far137": (0.002, moved(faces.CUT_BBOX, faces.SHIFT_137)),
              "dy128": (faces.DYADIC_RES, moved(faces.DYADIC_BBOX, faces.SHIFT_128)),
              "dy1024": (faces.DYADIC_RES, moved(faces.DYADIC_BBOX, faces.SHIFT_1024))}
LEAF_PER_FAMILY = 400
LEAF_NEAR_FACE = 80      # of them within 2 cells of a grid face on one axis at least: validCoord clips the stencil
LEAF_EMPTY = 40          # further probes with an empty stencil
LEAF_VP_AT_CENTRE = 20   # of them with the viewpoint equal to the cell centre: a zero direction, no flip


def leaf_inputs(dims, bbox, centre_of, seed=0x1EAF):
    """(family per probe, cells (n, 3) int32, stencils (n, 125) uint8, viewpoints (n, 3) f32) for every family at LEAF_PER_FAMILY random
    cells, and LEAF_EMPTY empty stencils.  centre_of: cells -> their f32 centres (OracleGrid.probe_center)."""
    rng = np.random.default_rng(seed)
    d = np.asarray(dims, np.int64)
    lo, hi = faces.lo_hi(bbox)
    names, cells, occ = [], [], []
    for fam, mask in FAMILIES.items():
        c = np.stack([rng.integers(0, d[a], LEAF_PER_FAMILY) for a in range(3)], axis=1)
        k = np.arange(LEAF_NEAR_FACE)
        axis = rng.integers(0, 3, LEAF_NEAR_FACE)
        edge = rng.integers(0, 4, LEAF_NEAR_FACE)   # index 0, 1, dim - 2, dim - 1
        c[k, axis] = np.where(edge < 2, edge, d[axis] - 4 + edge)
        names += [fam] * LEAF_PER_FAMILY
        cells.append(c)
        occ.append(np.broadcast_to(mask, (LEAF_PER_FAMILY, 125)))
    names += ["empty"] * LEAF_EMPTY   # a total of 0: no stencil at all
    cells.append(np.stack([rng.integers(0, d[a], LEAF_EMPTY) for a in range(3)], axis=1))
    occ.append(np.zeros((LEAF_EMPTY, 125), np.uint8))
    cells = np.ascontiguousarray(np.vstack(cells), np.int32)
    occ = np.ascontiguousarray(np.vstack(occ), np.uint8)
    vps = rng.uniform(lo - 1.0, hi + 1.0, (len(cells), 3)).astype(np.float32)
    at_centre = (np.arange(len(cells)) % LEAF_PER_FAMILY) >= LEAF_PER_FAMILY - LEAF_VP_AT_CENTRE
    vps[at_centre] = centre_of(cells[at_centre])
    return np.array(names), cells, occ, np.ascontiguousarray(vps)


def leaf_reference(og, cells, occ, vps):
    """(totals, normals) of OracleGrid.probe_normal, one call per probe; a total below 3 leaves the zero normal."""
    totals = np.zeros(len(cells), np.int32)
    normals = np.zeros((len(cells), 3), np.float32)
    for i in range(len(cells)):
        totals[i], normals[i] = og.probe_normal(int(cells[i, 0]), int(cells[i, 1]), int(cells[i, 2]), occ[i], vps[i])
    return totals, normals
