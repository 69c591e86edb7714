"""A crafted schedule (tests/crafted.py: Launch | CLEAN) driven over several handles that stand in for ranks (imported by tests only).

Every frame of every launch has a global id: the launch's own ids, else a running count over the launches without ids, as a single
handle numbers them.  deal(launch_index, frame_index, fid) names the rank that owns a frame; a rank's share of a launch goes down as
ONE hfpf_integrate_device call with its frame ids, and a rank without a share makes no call.  At a CLEAN every rank exports, the
records move in one of three ways, and every rank cleans:

  "lists"     one hfpf_epoch_import per foreign rank               (hfpf_dist.LocalVirtualRanks)
  "gathered"  one padded buffer, hfpf_epoch_import_gathered        (LocalVirtualRanks(gathered=True); with `poison` the driver's own
              buffer: a stride 2048 records and more beyond the largest count, all padding and the importer's own slice filled with
              the poison records)
  "concat"    the foreign ranks' records joined on the host and imported in ONE launch, as hfpf_dist.HostStagedTransport.exchange

The handles are wrapped so that every export is downloaded into the run's log (exchange -> rank -> record array) before anything is
imported: a test checks the log against exchange_ref and asserts its own preconditions on it."""
import numpy as np

import crafted as X
import exchange_ref as E
import hfpf_dist

CAPS = dict(max_bricks=4096, max_log_points=1 << 20, max_normals=1 << 15, max_frames=64)   # the crafted cases' (test_gpu_crafted.py)
MODES = ("lists", "gathered", "concat")
POISON_MARGIN = 2048   # records the poisoned buffer's stride exceeds the largest count by, at least


class _Logged:
    """A handle whose epoch_export also files the exported records (downloaded) in `sink`."""

    def __init__(self, g, sink):
        self._g, self._sink = g, sink

    def __getattr__(self, name):
        return getattr(self._g, name)

    def epoch_export(self):
        ptr, n = self._g.epoch_export()
        rec = self._g.device_download(ptr, n * E.REC_DTYPE.itemsize).view(E.REC_DTYPE) if n else np.zeros(0, E.REC_DTYPE)
        self._sink.append(rec.copy())
        return ptr, n


def frame_ids(ops):
    """op index -> the global ids of its frames (None for a CLEAN)."""
    out, running = [], 0
    for op in ops:
        if op is X.CLEAN:
            out.append(None)
        elif op.ids is not None:
            out.append(list(op.ids))
        else:
            out.append(list(range(running, running + len(op.frames))))
            running += len(op.frames)
    return out


def integrate(g, frames, poses, ids, n_points):
    """One hfpf_integrate_device call, waited for."""
    buf = np.concatenate([np.ascontiguousarray(f).view(np.uint8).reshape(-1) for f in frames])
    dev = g.device_alloc(max(buf.nbytes, 16))
    try:
        g.device_upload(dev, buf)
        g.integrate_device(dev, len(frames), n_points * 16, n_points, np.stack([np.asarray(p, np.float64).reshape(12) for p in poses]),
                           frame_ids=None if ids is None else np.array(ids, np.uint32))
        g.sync()
    finally:
        g.device_free(dev)


def _import_array(g, rec):
    if not len(rec):
        return
    dev = g.device_alloc(rec.nbytes)
    try:
        g.device_upload(dev, rec)
        g.epoch_import(dev, len(rec))
        g.sync()
    finally:
        g.device_free(dev)


def _exchange_concat(grids, sink):
    for g in grids:
        g.epoch_export()
    for i, g in enumerate(grids):
        foreign = [r for j, r in enumerate(sink) if j != i and len(r)]
        if foreign:
            _import_array(g, np.concatenate(foreign))


def poisoned_buffer(exports, importer, poison):
    """(buffer, stride in bytes, counts): slice r = the records rank r exported, then poison to the end of the slice; the importer's
    own slice is poison from its first record."""
    assert len(poison) > 0
    counts = np.array([len(r) for r in exports], np.uint64)
    stride = int(counts.max()) + POISON_MARGIN + 17
    buf = np.resize(poison, len(exports) * stride)   # the poison records, over and over
    for r, rec in enumerate(exports):
        if r != importer:
            buf[r * stride:r * stride + len(rec)] = rec
    return buf, stride * E.REC_DTYPE.itemsize, counts


def _exchange_poisoned(grids, sink, poison):
    for g in grids:
        g.epoch_export()
    for i, g in enumerate(grids):
        buf, stride, counts = poisoned_buffer(sink, i, poison)
        dev = g.device_alloc(buf.nbytes)
        try:
            g.device_upload(dev, buf)
            g.epoch_import_gathered(dev, stride, len(grids), i, counts)
            g.sync()
        finally:
            g.device_free(dev)


def run_sharded(hfpf_mod, ops, deal, world, mode, colour=False, config=None, caps=None, bbox=X.BBOX, res=X.RES, extract_on=(0,), poison=None):
    """-> dict: rows (rank -> merged rows taken on that rank, for the ranks of extract_on), occ (every rank's occupied list), counters
    (every rank's at the end), per_op (op index -> every rank's counters behind it), log (exchange -> rank -> exported records),
    points (all points of the schedule)."""
    assert mode in MODES and (poison is None or mode == "gathered")
    ids = frame_ids(ops)
    grids = [hfpf_mod.OccupancyGrid(resolution=res, bbox=bbox, fuse_color=colour, **(config or {}), **dict(CAPS, **(caps or {}))) for _ in range(world)]
    log, per_op, points = [], [], 0
    try:
        for i, op in enumerate(ops):
            if op is X.CLEAN:
                sink = []
                ranks = [_Logged(g, sink) for g in grids]
                if mode == "concat":
                    _exchange_concat(ranks, sink)
                elif poison is not None:
                    _exchange_poisoned(ranks, sink, poison)
                if mode == "concat" or poison is not None:
                    for g in grids:
                        g.clean()
                else:
                    hfpf_dist.LocalVirtualRanks(ranks, gathered=mode == "gathered").clean_all()
                assert len(sink) == world, "%d exports of %d ranks" % (len(sink), world)
                log.append(sink)
            else:
                owner = [int(deal(i, f, fid)) for f, fid in enumerate(ids[i])]
                assert all(0 <= r < world for r in owner), owner
                points += len(op.frames) * op.n_points
                for r, g in enumerate(grids):
                    mine = [f for f in range(len(op.frames)) if owner[f] == r]
                    if mine:
                        integrate(g, [op.frames[f] for f in mine], [op.poses[f] for f in mine], [ids[i][f] for f in mine], op.n_points)
            per_op.append([g.counters() for g in grids])
        vr = hfpf_dist.LocalVirtualRanks(grids)
        rows = {r: vr.extract(on=r).copy() for r in extract_on}
        return dict(rows=rows, occ=[g.occupied().copy() for g in grids], counters=[g.counters() for g in grids], per_op=per_op, log=log, points=points)
    finally:
        for g in grids:
            g.close()


def run_single(hfpf_mod, ops, colour=False, config=None, caps=None, bbox=X.BBOX, res=X.RES):
    """One handle through the same schedule: dict rows, occ, counters, per_op."""
    per_op = []
    with hfpf_mod.OccupancyGrid(resolution=res, bbox=bbox, fuse_color=colour, **(config or {}), **dict(CAPS, **(caps or {}))) as g:
        for op in ops:
            if op is X.CLEAN:
                g.clean()
            else:
                integrate(g, op.frames, op.poses, op.ids, op.n_points)
            per_op.append(g.counters())
        return dict(rows=g.extract().copy(), occ=g.occupied().copy(), counters=g.counters(), per_op=per_op)


def run_oracle(oracle_mod, ops, colour=False, config=None, each=None, bbox=X.BBOX, res=X.RES):
    """The oracle (exact moments) through the schedule: dict exact (extract_exact), rows (extract), occ.  each(og, i) is called ahead
    of op i, for what a precondition needs of the state there."""
    if (bbox, res) == (X.BBOX, X.RES):
        og = X.oracle_grid(oracle_mod, X.Case("sharded", ops, None, config=config), colour)
    else:   # crafted.oracle_grid is the dyadic box's
        og = oracle_mod.OracleGrid(resolution=res, bbox=bbox, exact_moments=True, **(config or {}), **(dict(fuse_color=True) if colour else {}))
    try:
        for i, op in enumerate(ops):
            if each:
                each(og, i)
            X.drive_oracle(og, [op], colour)
        rows = og.extract()
        return dict(exact=og.extract_exact(), rows=rows, occ=og.occupied())
    finally:
        og.close()


# ---- what the log says ----------------------------------------------------------------------------------------------------------

def log_cells(rec, dims=X.DIMS):
    """The cell records of one exported array as (cells (n, 3) int64, first_frame)."""
    c = rec[~E.is_frame(rec)]
    return E.key_cells(dims, c["key"]).astype(np.int64), c["first_frame"]


def check_export_shape(rec, what):
    """An export is its cell records (pad 0, keys distinct), then two records a frame: half 0, half 1, the same id."""
    fr = E.is_frame(rec)
    n_cells = int((~fr).sum())
    assert not fr[:n_cells].any() and fr[n_cells:].all(), "%s: cell records behind frame records" % what
    assert (rec["pad"][:n_cells] == 0).all() and len(np.unique(rec["key"][:n_cells])) == n_cells, "%s: pad or duplicate keys" % what
    fk = rec["key"][n_cells:]
    assert len(fk) % 2 == 0, "%s: an odd number of frame records" % what
    assert ((fk[0::2] & E.HALF) == 0).all() and ((fk[1::2] & E.HALF) != 0).all() and ((fk[0::2] | E.HALF) == fk[1::2]).all(), "%s: frame halves" % what
    return n_cells, len(fk) // 2


def replay_log(log, world, dims=X.DIMS, max_frames=CAPS["max_frames"]):
    """exchange_ref over the whole log: every rank's model state after importing, at every exchange, all foreign ranks' records on top
    of its own.  Returns the states (all ranks must agree on cells and latches) -- the occupied set any rank must end with."""
    states = [E.State() for _ in range(world)]
    for sink in log:
        for i in range(world):
            for j in range(world):
                E.import_records(states[i], sink[j], dims, max_frames)   # its own records: the cells it occupied itself
    for s in states[1:]:
        assert s.same(states[0]), "the model ranks disagree"
    return states
