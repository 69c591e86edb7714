"""GPU: rows that depth frames see through (hfpf_depth_consistency, hfpf_depth_consistency_device).  The call is defined on the rows
hfpf_extract_filtered returns, so rows, records and summary are compared byte for byte with tests/consistency_ref.py run on those.
The shared session is three frames of the synthetic depth stream plus a ghost: a 32 mm square of points integrated once, 30 cm in
front of the first camera, which every scene frame then looks through.  The frames looked at are the three scene frames, the
held-out frame and a copy of frame 0 with three rectangles moved behind the model, in front of it, and zeroed."""
import os

import numpy as np
import pytest

import consistency_ref as CR
from gpu_support import RES, Session, counters, download, grid, held_out, perturb, run, same_records, same_summary, uploaded
from scenes import DepthScene

pytestmark = pytest.mark.gpu
W, H = 160, 120
GHOST_KW = dict(window=1, tolerance=0.004, min_cos=0.3, min_through=1, through_ratio=1.0)  # the settings the ghost test pins


def _fuse(hfpf_mod, sc, ghost=True, **kw):
    """(grid, rows before the ghost) of the session's model on a fresh handle."""
    g = grid(hfpf_mod, **kw)
    try:
        run(g, sc)
        pre = g.extract().copy()
        if ghost:
            g.integrate(CR.ghost_cloud(RES), sc.poses[0])
            g.clean()
    except BaseException:
        g.close()
        raise
    return g, pre


class _Scene:
    pass


@pytest.fixture(scope="module")
def session(hfpf_mod, synth_mod):
    s = _Scene()
    s.sc = DepthScene(3, W, H, clean_every=2)
    s.g, s.pre = _fuse(hfpf_mod, s.sc)
    s.K = s.sc.K
    s.rows = s.g.extract().copy()
    s.ghost = ~np.isin(CR.voxel_keys(s.rows), CR.voxel_keys(s.pre))
    held, held_K, held_pose = held_out(synth_mod, W, H)
    assert held_K == s.K
    s.frames = np.stack([s.sc.frames[f][0] for f in range(3)] + [held, CR.tampered(s.sc.frames[0][0])])
    s.poses = np.stack(list(s.sc.poses) + [held_pose, s.sc.poses[0]])
    s.desc = hfpf_mod.depth_desc(W, H, hfpf_mod.DEPTH_U16, 2 * W, s.K)
    # the scene as the reference sees it, so that a failure of the scene is not mistaken for one of the engine
    cls = CR.classify(s.rows, s.frames[4], s.poses[4], s.K, window=0, tolerance=0.004)
    pop = {k: int((cls == v).sum()) for k, v in (("support", CR.SUPPORT), ("through", CR.THROUGH), ("occluded", CR.OCCLUDED), ("no_depth", CR.NO_DEPTH))}
    print("session: %d rows, %d ghost rows; the tampered frame alone: %r" % (len(s.rows), s.ghost.sum(), pop))
    assert len(s.rows) > 10000 and s.ghost.sum() > 100 and s.rows[~s.ghost].tobytes() == s.pre.tobytes()
    assert all(v > 100 for v in pop.values()), pop
    s.refs = {}
    yield s
    s.g.close()


def _ref(s, window, frames=None, poses=None, **kw):
    """The reference on the session's rows, computed once per option set."""
    key = (window, id(frames), tuple(sorted(kw.items())))
    if key not in s.refs:
        s.refs[key] = CR.consistency(s.rows, s.frames if frames is None else frames, s.poses if poses is None else poses, s.K, window=window, **kw)
        for a in s.refs[key][:2]:
            a.setflags(write=False)
    return s.refs[key]


def _device(g, H_, desc, frames, stride, n, poses, rows=True, **kw):
    """hfpf_depth_consistency_device on a fresh upload of `frames` (any contiguous array), downloaded: (rows, cons, summary)."""
    with uploaded(g, frames) as (d,):
        r, c, nr, s = g.depth_consistency_device(desc, d, stride, n, poses, rows=rows, **kw)
    out_rows, cons = download(g, (r if rows else 0, nr, H_.ROW_DTYPE), (c, nr, H_.ROW_CONSISTENCY_DTYPE), free=(r,))
    return (out_rows if rows else None), cons, s


def _same(got, ref, what):
    same_records(got[:2], ref[:2], what, ("rows", "records"))
    same_summary(got[2], ref[2], CR.SUMMARY_KEYS, what)


def _sums(cons, s, n_set):
    """The summary is the sum of the records of the whole row set (cons: the records without HFPF_CONSISTENCY_DROP)."""
    assert s["n_rows"] == n_set == len(cons), "n_rows"
    assert s["pairs_tested"] == int(cons["n_tested"].sum()) and s["pairs_support"] == int(cons["n_support"].sum()), "pairs"
    assert s["pairs_through"] == int(cons["n_through"].sum()), "pairs_through"
    assert s["n_seen"] == int((cons["flags"] & CR.SEEN != 0).sum()) and s["n_supported"] == int((cons["flags"] & CR.SUPPORTED != 0).sum()), "flags"
    assert s["n_contradicted"] == int((cons["flags"] & CR.CONTRADICTED != 0).sum()) and s["n_kept"] == s["n_rows"] - s["n_contradicted"], "kept"
    assert not cons["reserved"].any(), "reserved"


# ---- 1. byte-exact against the numpy contract, both forms, both formats -----------------------------------------------------------

@pytest.mark.parametrize("fmt", ["u16", "f32"])
@pytest.mark.parametrize("drop", [False, True], ids=["all", "drop"])
@pytest.mark.parametrize("window", [0, 1, 2])
def test_byte_exact_against_consistency_ref(hfpf_mod, session, window, drop, fmt):
    s = session
    kw = dict(window=window, tolerance=0.004, min_cos=0.3, drop=drop)
    ref = _ref(s, window, tolerance=0.004, min_cos=0.3, drop=drop)
    full = _ref(s, window, tolerance=0.004, min_cos=0.3, drop=False)
    for k in ("n_support", "n_through", "n_occluded"):
        assert int(full[1][k].sum()) > 100, "the reference's own result exercises %s" % k
    if fmt == "u16":
        frames, desc = s.frames, s.desc
    else:
        frames = np.stack([CR.as_f32(f, 0.001) for f in s.frames])
        desc = hfpf_mod.depth_desc(W, H, hfpf_mod.DEPTH_F32, 4 * W, s.K)
    host = s.g.depth_consistency(frames, s.poses, s.K, **kw)
    dev = _device(s.g, hfpf_mod, desc, frames, frames.strides[0], len(frames), s.poses, **kw)
    what = "window %d, drop %s, %s" % (window, drop, fmt)
    print("%s: %r" % (what, host[2]))
    _same(host, ref, what + ", host form")
    _same(dev, ref, what + ", device form")
    _sums(full[1], host[2], len(s.rows))
    assert (len(host[0]) == host[2]["n_kept"]) if drop else (len(host[0]) == len(s.rows)), "output rows"
    no_rows = s.g.depth_consistency(frames, s.poses, s.K, rows=False, **kw)
    assert no_rows[0] is None and no_rows[1].tobytes() == ref[1].tobytes(), "rows = NULL"
    assert _device(s.g, hfpf_mod, desc, frames, frames.strides[0], len(frames), s.poses, rows=False, **kw)[1].tobytes() == ref[1].tobytes()


# ---- 2. the split into chunks, launches and uploads does not change a byte ----------------------------------------------------------

def _many(s, n):
    """n frames: the five repeated, every repeat at a slightly perturbed pose."""
    frames = np.stack([s.frames[i % 5] for i in range(n)])
    poses = []
    for i in range(n):
        r = i // 5
        poses.append(s.poses[i % 5] if r == 0 else perturb(s.poses[i % 5], 0.05 * r, (0.0004 * r, -0.0003 * r, 0.0002 * r)))
    return frames, np.stack(poses)


def test_split_invariance(hfpf_mod, session):
    s = session
    frames, poses = _many(s, 130)
    ref = CR.consistency(s.rows, frames, poses, s.K, **GHOST_KW)
    assert ref[1]["first_through"][ref[1]["n_through"] > 0].max() >= 64, "a first THROUGH frame behind the first chunk of 64"
    assert ref[2]["n_contradicted"] > 100 and ref[2]["pairs_through"] > 1000
    # the session's own handle: plan_consistency decides
    _same(_device(s.g, hfpf_mod, s.desc, frames, frames.strides[0], 130, poses, **GHOST_KW), ref, "130 frames, planned")
    old = os.environ.get("HFPF_CONSISTENCY_CHUNK")
    try:
        for chunk in ("1", "64"):  # 130 chunks of one frame; 64 + 64 + a tail of 2
            os.environ["HFPF_CONSISTENCY_CHUNK"] = chunk
            g, _ = _fuse(hfpf_mod, s.sc)
            with g:
                assert g.extract().tobytes() == s.rows.tobytes(), "a fresh handle fuses the same rows"
                _same(_device(g, hfpf_mod, s.desc, frames, frames.strides[0], 130, poses, **GHOST_KW), ref, "130 frames, chunk " + chunk)
                _same(g.depth_consistency(frames, poses, s.K, **GHOST_KW), ref, "130 frames, chunk %s, host form" % chunk)
                # five frames in one chunk: plain stores
                _same(g.depth_consistency(s.frames, s.poses, s.K, **GHOST_KW), _ref(s, 1, **{k: v for k, v in GHOST_KW.items() if k != "window"}),
                      "5 frames, chunk " + chunk)
    finally:
        if old is None:
            os.environ.pop("HFPF_CONSISTENCY_CHUNK", None)
        else:
            os.environ["HFPF_CONSISTENCY_CHUNK"] = old


def test_host_form_in_two_uploads(hfpf_mod, session):
    """Nine frames 4 MB apart: the pinned staging takes 16 MB at a time, so they go up as 4 + 4 + 1."""
    s = session
    frames, poses = _many(s, 9)
    stride = 4 << 20
    buf = np.full(8 * stride + 2 * W * H, 0xFF, np.uint8)
    for f in range(9):
        buf[f * stride:f * stride + 2 * W * H] = frames[f].view(np.uint8).reshape(-1)
    ref = CR.consistency(s.rows, frames, poses, s.K, **GHOST_KW)
    got = s.g.depth_consistency(buf, poses, s.K, desc=s.desc, depth_frame_stride=stride, n_frames=9, **GHOST_KW)
    _same(got, ref, "9 frames, 4 MB apart")
    assert got[1]["first_through"][got[1]["n_through"] > 0].max() >= 4, "a first THROUGH frame in the second upload"


# ---- 3. the ghost ------------------------------------------------------------------------------------------------------------------

def test_drop_removes_exactly_the_ghost(hfpf_mod, session):
    s = session
    frames, poses = s.frames[:3], s.poses[:3]
    ref = CR.consistency(s.rows, frames, poses, s.K, **GHOST_KW)
    contra = (ref[1]["flags"] & CR.CONTRADICTED) != 0
    print("ghost: %d rows, contradicted %d of them and %d others" % (s.ghost.sum(), (contra & s.ghost).sum(), (contra & ~s.ghost).sum()))
    assert (contra == s.ghost).all(), "the reference contradicts the ghost rows and no others"
    out, cons, summary = s.g.depth_consistency(frames, poses, s.K, drop=True, **GHOST_KW)
    assert out.tobytes() == s.rows[~s.ghost].tobytes() == s.pre.tobytes(), "DROP leaves the rows from before the ghost"
    assert out.tobytes() == s.g.extract_filtered(0.0)[~s.ghost].tobytes()
    assert summary["n_contradicted"] == s.ghost.sum() and summary["n_kept"] == len(s.pre) and not (cons["flags"] & CR.CONTRADICTED).any()
    # min_count: the row set is hfpf_extract_filtered's
    gated = s.g.extract_filtered(3.0)
    assert 0 < len(gated) < len(s.rows)
    _same(s.g.depth_consistency(frames, poses, s.K, min_count=3.0, **GHOST_KW), CR.consistency(gated, frames, poses, s.K, **GHOST_KW), "min_count 3")


# ---- 4. render round trip, far from the origin ----------------------------------------------------------------------------------------

def test_render_round_trip(hfpf_mod):
    """The model's own depth plane as a frame at the same pose: nothing is seen through, and every row that won a pixel is supported."""
    s = Session(hfpf_mod, "far")
    try:
        K, Wr, Hr, z_range = (300.0, 300.0, 159.5, 119.5), 320, 240, (0.05, 3.0)
        pose = s.sc.poses[0]
        desc = hfpf_mod.depth_desc(Wr, Hr, hfpf_mod.DEPTH_F32, 4 * Wr, K)
        kw = dict(window=0, min_cos=-1.0, min_count=1.0, z_range=z_range, tolerance=0.004)
        plane = s.g.device_alloc(4 * Wr * Hr)
        try:
            s.g.render_device([pose], K, Wr, Hr, {"depth": plane}, z_range=z_range, min_count=1, splat_radius=0)
            r, c, nr, summary = s.g.depth_consistency_device(desc, plane, 4 * Wr * Hr, 1, [pose], **kw)
            rows, cons = download(s.g, (r, nr, hfpf_mod.ROW_DTYPE), (c, nr, hfpf_mod.ROW_CONSISTENCY_DTYPE))
            depth = s.g.device_download(plane, 4 * Wr * Hr, np.float32).reshape(1, Hr, Wr).copy()
        finally:
            s.g.device_free(plane)
        voxel = s.g.render(pose, K, Wr, Hr, planes=("voxel",), z_range=z_range, min_count=1, splat_radius=0)["voxel"].reshape(-1, 3)
        won = np.zeros(len(rows), bool)
        hit = voxel[voxel[:, 0] >= 0].astype(np.int64)
        won[np.searchsorted(CR.voxel_keys(rows), (hit[:, 0] << 42) | (hit[:, 1] << 21) | hit[:, 2])] = True
        print("round trip: %d rows, %d won a pixel, summary %r" % (len(rows), won.sum(), summary))
        assert won.sum() > 1000 and rows.tobytes() == s.g.extract_filtered(1.0).tobytes()
        assert not cons["n_through"].any(), "no row is seen through by the model's own depth"
        assert (cons["n_support"][won] >= 1).all(), "a row that won a pixel is supported by it"
        _same((rows, cons, summary), CR.consistency(s.rows, depth, [pose], K, **kw), "render round trip")
    finally:
        s.close()


# ---- 5. layout -----------------------------------------------------------------------------------------------------------------------

def test_padded_layout_gives_the_same_bytes(hfpf_mod, session):
    """depth_step and depth_frame_stride larger than needed, the padding 0xFFFF; the last frame ends where its allocation ends."""
    s = session
    step, n = 2 * W + 64, len(s.frames)
    stride = H * step + 128
    tight = (H - 1) * step + 2 * W
    buf = np.full((n - 1) * stride + tight, 0xFF, np.uint8)
    for f in range(n):
        img = buf[f * stride:f * stride + tight]
        for v in range(H):
            img[v * step:v * step + 2 * W] = s.frames[f][v].view(np.uint8)
    desc = hfpf_mod.depth_desc(W, H, hfpf_mod.DEPTH_U16, step, s.K)
    for window in (0, 2):
        ref = _ref(s, window, tolerance=0.004, min_cos=0.3)
        kw = dict(window=window, tolerance=0.004, min_cos=0.3)
        _same(_device(s.g, hfpf_mod, desc, buf, stride, n, s.poses, **kw), ref, "padded, device form, window %d" % window)
        _same(s.g.depth_consistency(buf, s.poses, s.K, desc=desc, depth_frame_stride=stride, n_frames=n, **kw), ref, "padded, host form")
    # a strided numpy view gives the same through the binding's own descriptor
    wide = np.full((n, H, W + 32), 0xFFFF, np.uint16)
    wide[:, :, :W] = s.frames
    _same(s.g.depth_consistency(wide[:, :, :W], s.poses, s.K, **kw), ref, "a view of a wider array")


# ---- 6. edges ------------------------------------------------------------------------------------------------------------------------

def test_edges(hfpf_mod, session):
    s = session
    kw = dict(window=1, tolerance=0.004)
    # fewer than one wave of rows
    counts = np.unique(s.rows["count"])
    top = float(min(c for c in counts if (s.rows["count"] >= c).sum() < 64))  # the lowest count gate that leaves fewer than 64 rows
    few = s.g.extract_filtered(top)
    assert 0 < len(few) < 64
    for drop in (False, True):
        _same(s.g.depth_consistency(s.frames, s.poses, s.K, min_count=top, drop=drop, **kw),
              CR.consistency(few, s.frames, s.poses, s.K, drop=drop, **kw), "%d rows, drop %s" % (len(few), drop))
    # no frames: the row set, all-zero records
    for rows, cons, summary in (s.g.depth_consistency(np.zeros((0, H, W), np.uint16), np.zeros((0, 12)), s.K, **kw),
                                _device(s.g, hfpf_mod, s.desc, np.zeros(16, np.uint8), 2 * W * H, 0, np.zeros((0, 12)), **kw)):
        assert rows.tobytes() == s.rows.tobytes() and len(cons) == len(rows)
        assert (cons["first_through"] == CR.NONE).all() and not any(cons[k].any() for k in cons.dtype.names if k != "first_through")
        assert summary == dict(n_rows=len(rows), n_seen=0, n_supported=0, n_contradicted=0, n_kept=len(rows), pairs_tested=0, pairs_support=0,
                               pairs_through=0)
    # a camera looking away from the model
    away = np.hstack([s.poses[0][:, :3] @ np.diag([1.0, -1.0, -1.0]), s.poses[0][:, 3:]])
    rows, cons, summary = s.g.depth_consistency(s.frames[:1], [away], s.K, **kw)
    assert len(cons) == len(s.rows) and not cons["n_in_view"].any() and summary["n_seen"] == 0
    _same((rows, cons, summary), CR.consistency(s.rows, s.frames[:1], [away], s.K, **kw), "looking away")


def test_empty_handle_and_before_the_first_clean(hfpf_mod, session):
    s = session
    with grid(hfpf_mod) as g:
        for stage in ("empty", "before the first clean"):
            rows, cons, summary = g.depth_consistency(s.frames, s.poses, s.K)
            assert len(rows) == 0 and len(cons) == 0 and summary["n_rows"] == 0 and summary["n_kept"] == 0, stage
            with uploaded(g, s.frames) as (d,):
                assert g.depth_consistency_device(s.desc, d, 2 * W * H, 5, s.poses)[:3] == (0, 0, 0), stage
            s.sc.integrate(g, 0)
        g.clean()
        assert len(g.depth_consistency(s.frames, s.poses, s.K)[1]) == len(g.extract()) > 0


def test_restored_handle_gives_the_same_bytes(hfpf_mod, session):
    """A read-only call on a restored handle returns what the source handle returns (include/hfpf.h, snapshots)."""
    s = session
    ref = _ref(s, 1, tolerance=0.004, min_cos=0.3, drop=True)
    blob = s.g.snapshot()
    with grid(hfpf_mod) as b:
        b.restore(blob)
        _same(b.depth_consistency(s.frames, s.poses, s.K, window=1, tolerance=0.004, min_cos=0.3, drop=True), ref, "restored handle")
        _same(_device(b, hfpf_mod, s.desc, s.frames, 2 * W * H, 5, s.poses, window=1, tolerance=0.004, min_cos=0.3, drop=True), ref,
              "restored handle, device form")


# ---- 7. rejected arguments ---------------------------------------------------------------------------------------------------------------

def test_rejected_arguments_change_nothing(hfpf_mod, session):
    import ctypes as C
    s = session
    g, L = s.g, hfpf_mod.lib()
    before, want = counters(g), g.extract().tobytes()
    ok_o = hfpf_mod.consistency_opts()
    poses = np.ascontiguousarray(s.poses, np.float64).reshape(-1)
    frames = np.ascontiguousarray(s.frames)
    bad_pose = poses.copy()
    bad_pose[17] = np.inf

    def desc(**kw):
        d = hfpf_mod.depth_desc(W, H, hfpf_mod.DEPTH_U16, 2 * W, s.K)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def opts(**kw):
        o = hfpf_mod.consistency_opts()
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    with uploaded(g, frames) as (dev,):
        for device in (False, True):
            fn = L.hfpf_depth_consistency_device if device else L.hfpf_depth_consistency
            base = dev if device else frames.ctypes.data

            def call(o=ok_o, d=None, depth=base, stride=2 * W * H, n=5, p=poses, cons=True, n_rows=True, summary=True):
                r, c, nr, sm = C.c_void_p(0x1), C.c_void_p(0x1), C.c_uint64(77), hfpf_mod.ConsistencySummary()
                sm.n_rows = 77
                rc = fn(g._h, C.byref(o) if o is not None else None, C.byref(d if d is not None else desc()), C.c_void_p(depth), stride, n,
                        p.ctypes.data_as(C.c_void_p) if p is not None else None, C.byref(r), C.byref(c) if cons else None,
                        C.byref(nr) if n_rows else None, C.byref(sm) if summary else None)
                assert (r.value, c.value, nr.value, sm.n_rows) == (0x1, 0x1, 77, 77), "a rejected call wrote an output"
                return rc

            cases = [("NULL opts", dict(o=None)), ("NULL depth", dict(depth=None)), ("NULL poses", dict(p=None)), ("non-finite pose", dict(p=bad_pose)),
                     ("stride below one image", dict(stride=2 * W * H - 2)), ("stride not a multiple of the sample", dict(stride=2 * W * H + 1)),
                     ("too many frames", dict(n=(1 << 20) + 1)), ("NULL cons", dict(cons=False)), ("NULL n_rows", dict(n_rows=False)),
                     ("NULL summary", dict(summary=False)),
                     ("desc struct_size", dict(d=desc(struct_size=8))), ("desc reserved", dict(d=desc(reserved=1))), ("desc width 0", dict(d=desc(width=0))),
                     ("desc format", dict(d=desc(depth_format=9))), ("desc step", dict(d=desc(depth_step=2 * W - 2))),
                     ("desc odd step", dict(d=desc(depth_step=2 * W + 1))), ("desc fx", dict(d=desc(fx=0.0))), ("desc cy", dict(d=desc(cy=float("nan")))),
                     ("desc scale", dict(d=desc(depth_scale=0.0))), ("desc colour format", dict(d=desc(color_format=9))),
                     ("desc colour step", dict(d=desc(color_format=hfpf_mod.COLOR_RGB8, color_step=3 * W - 1)))]
            cases += [("opts %s = %r" % (k, v), dict(o=opts(**{k: v}))) for k, v in (
                ("struct_size", 64), ("flags", 2), ("reserved", 1), ("window", 3), ("window", -1), ("min_count", float("nan")), ("z_near", 0.0),
                ("z_far", float("inf")), ("z_far", 0.001), ("tolerance", 0.0), ("tolerance", 2.0), ("slope", -0.5), ("slope", 2.0), ("min_cos", 1.5),
                ("min_cos", float("nan")), ("through_ratio", -1.0), ("through_ratio", float("inf")))]
            if device:
                cases.append(("misaligned image", dict(depth=dev + 1)))
            for what, kw in cases:
                assert call(**kw) == -2, "%s (%s form)" % (what, "device" if device else "host")
    assert counters(g) == before and g.extract().tobytes() == want, "a rejected call changed the handle"
    # a valid colour descriptor passes (no colour image is read), and the handle still answers
    d = desc(color_format=hfpf_mod.COLOR_RGB8, color_step=3 * W)
    ref = _ref(s, 0, tolerance=0.004, min_cos=0.3)
    _same(s.g.depth_consistency(frames, s.poses, s.K, desc=d, depth_frame_stride=2 * W * H, n_frames=5, window=0, tolerance=0.004, min_cos=0.3), ref,
          "after the rejected calls")
    assert counters(g) == before and g.extract().tobytes() == want, "a call changed the handle"
