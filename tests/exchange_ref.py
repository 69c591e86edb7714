"""The epoch exchange's 16-byte records and what export and import promise, in numpy (imported by tests only).

Written from include/hfpf.h ("Transport 2: bring your own") and the comment above struct EpochRec in csrc/kernels.hpp:

  a CELL record    key = x << sx | y << sy | z, with just enough bits an axis for 0..dim (storage is dim + 1 cells an axis, so a
                   coordinate EQUAL to dim is kept and dim + 1 is outside); first_frame = the smallest frame id that touched the
                   cell on the exporting rank; pad = 0.  A cell key is below 2^63.
  a FRAME record   key = 2^63 | half << 62 | frame id; the other eight bytes are two f32: half 0 carries the viewpoint's x and y,
                   half 1 its z and 0.  Two records per frame the rank has integrated since the last exchange.

An export lists the cells first, the frame records behind them.  An import is a fold over the records, in any order and any split
into launches: a cell joins the occupied set once, its latch becomes the minimum of what it was and every VALID first_frame
(< max_frames) offered for it; a frame half overwrites its two (one) floats; a cell key outside the storage extent, a latch or a
frame id at or above max_frames change nothing."""
import numpy as np

REC_DTYPE = np.dtype([("key", "<u8"), ("first_frame", "<u4"), ("pad", "<u4")])
assert REC_DTYPE.itemsize == 16
FRAME = np.uint64(1 << 63)
HALF = np.uint64(1 << 62)
NO_FRAME = 0xFFFFFFFF   # the latch of a cell nobody has offered a valid frame id for


def bits_for(dim):
    """Bits that hold 0..dim."""
    b = 1
    while (1 << b) <= int(dim):
        b += 1
    return b


def key_shifts(dims):
    """(sy, sx, bits): z takes the low sy bits, y the next sx - sy, x what lies above."""
    sy = bits_for(dims[2])
    sx = sy + bits_for(dims[1])
    return sy, sx, sx + bits_for(dims[0])


def make_key(dims, cells):
    sy, sx, _ = key_shifts(dims)
    c = np.asarray(cells, np.uint64).reshape(-1, 3)
    return (c[:, 0] << np.uint64(sx)) | (c[:, 1] << np.uint64(sy)) | c[:, 2]


def key_cells(dims, keys):
    """(n, 3) uint64: x is everything above the y field, however large."""
    sy, sx, _ = key_shifts(dims)
    k = np.asarray(keys, np.uint64).reshape(-1)
    return np.stack([k >> np.uint64(sx), (k >> np.uint64(sy)) & np.uint64((1 << (sx - sy)) - 1), k & np.uint64((1 << sy) - 1)], axis=1)


def is_frame(records):
    return (records["key"] & FRAME) != 0


def cell_records(dims, cells, first_frame):
    cells = np.asarray(cells).reshape(-1, 3)
    out = np.zeros(len(cells), REC_DTYPE)
    out["key"] = make_key(dims, cells)
    out["first_frame"] = np.broadcast_to(np.asarray(first_frame, np.uint32), (len(cells),))
    return out


def frame_records(frames, viewpoints):
    """Two records a frame, half 0 then half 1."""
    frames = np.asarray(frames, np.uint64).reshape(-1)
    vp = np.asarray(viewpoints, np.float32).reshape(-1, 3)
    assert len(vp) == len(frames)
    out = np.zeros(2 * len(frames), REC_DTYPE)
    floats = np.zeros((len(out), 2), np.float32)
    out["key"][0::2] = FRAME | frames
    out["key"][1::2] = FRAME | HALF | frames
    floats[0::2, 0], floats[0::2, 1] = vp[:, 0], vp[:, 1]
    floats[1::2, 0], floats[1::2, 1] = vp[:, 2], 0.0
    words = floats.view(np.uint32)
    out["first_frame"], out["pad"] = words[:, 0], words[:, 1]
    return out


def export_records(cells, first_frame, frames, viewpoints, dims):
    """What a rank exports that has newly occupied `cells` (n, 3) with the latches first_frame (n) and integrated `frames` (ids) from
    `viewpoints` (f32 x, y, z each) since the last exchange: the cell records, then two records per frame."""
    return np.concatenate([cell_records(dims, cells, first_frame), frame_records(frames, viewpoints)])


def record_floats(records):
    """The eight bytes behind the key as two f32, (n, 2)."""
    r = np.ascontiguousarray(records)
    return r.view(np.uint8).reshape(-1, 16)[:, 8:].copy().view(np.float32).reshape(-1, 2)


class State:
    """The part of a handle the exchange acts on: occupied cells, cell -> latch, frame -> viewpoint (three f32, zero until written)."""

    def __init__(self):
        self.occupied, self.latch, self.viewpoint = set(), {}, {}

    def copy(self):
        s = State()
        s.occupied, s.latch = set(self.occupied), dict(self.latch)
        s.viewpoint = {f: v.copy() for f, v in self.viewpoint.items()}
        return s

    def same(self, other):
        return (self.occupied == other.occupied and self.latch == other.latch and sorted(self.viewpoint) == sorted(other.viewpoint) and
                all(self.viewpoint[f].tobytes() == other.viewpoint[f].tobytes() for f in self.viewpoint))

    def cell_records(self, dims):
        """Every occupied cell as a record, sorted by key."""
        cells = np.array(sorted(self.occupied), np.int64).reshape(-1, 3)
        out = cell_records(dims, cells, [self.latch[tuple(c)] for c in cells.tolist()])
        return out[np.argsort(out["key"], kind="stable")]


def import_records(state, records, dims, max_frames):
    """Folds `records` into `state`; returns the cells newly added, in the order they first appear."""
    records = np.ascontiguousarray(records).view(REC_DTYPE).reshape(-1)
    frame = is_frame(records)
    cells = key_cells(dims, records["key"])
    floats = record_floats(records)
    new = []
    for i in range(len(records)):
        if frame[i]:
            fid = int(records["key"][i]) & 0xFFFFFFFF
            if fid >= max_frames:
                continue
            vp = state.viewpoint.setdefault(fid, np.zeros(3, np.float32))
            if int(records["key"][i]) & int(HALF):
                vp[2] = floats[i, 0]
            else:
                vp[0], vp[1] = floats[i, 0], floats[i, 1]
            continue
        c = tuple(int(v) for v in cells[i])
        if c[0] > dims[0] or c[1] > dims[1] or c[2] > dims[2]:
            continue
        if c not in state.occupied:
            state.occupied.add(c)
            state.latch[c] = NO_FRAME
            new.append(c)
        ff = int(records["first_frame"][i])
        if ff < max_frames:
            state.latch[c] = min(state.latch[c], ff)
    return new
