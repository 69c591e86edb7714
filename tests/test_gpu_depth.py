"""GPU: registered depth + colour images integrated on the device (hfpf_integrate_depth*).  A depth frame is defined as the
packed cloud tests/depth_ref.py makes of it, so every session here is compared byte for byte -- rows and counters -- with the
same session fed those clouds through the cloud path, and once with the oracle."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import depth_ref as R
import scenes
from gpu_support import BBOX, DEPTH_CAPS, counters, grid, run, same_records
from scenes import DepthScene

pytestmark = pytest.mark.gpu


def _result(g):
    return g.extract(), counters(g)


def _cloud_session(hfpf_mod, sc, clouds=None, **kw):
    clouds = clouds or [sc.cloud(f) for f in range(sc.n_frames)]
    with hfpf_mod.OccupancyGrid(resolution=kw.pop("resolution", 0.002), bbox=BBOX, fuse_color=kw.pop("fuse_color", True), **DEPTH_CAPS, **kw) as g:
        run(g, sc, integrate=lambda g, f: g.integrate(clouds[f], sc.poses[f]))
        return _result(g)


def _depth_session(hfpf_mod, sc, **kw):
    with hfpf_mod.OccupancyGrid(resolution=kw.pop("resolution", 0.002), bbox=BBOX, fuse_color=kw.pop("fuse_color", True), **DEPTH_CAPS, **kw) as g:
        run(g, sc)
        return _result(g)


def _same(a, b):
    assert a[1] == b[1], "counters differ: %s vs %s" % (a[1], b[1])
    same_records(a[0], b[0], "rows", "rows")


# ---- leaf -----------------------------------------------------------------------------------------------------------

def _probe_equal(g, depth, K, color=None, color_format=None, depth_scale=0.001):
    xyz, rgb = g.probe_depth(depth, K, color=color, color_format=color_format, depth_scale=depth_scale)
    ref = R.backproject(np.ascontiguousarray(depth), K, depth_scale)
    bad = np.flatnonzero((xyz.view(np.uint32) != ref.view(np.uint32)).any(axis=1))
    assert bad.size == 0, "%d pixels differ, first %d: %r vs %r" % (bad.size, bad[0], xyz[bad[0]], ref[bad[0]])
    want = R.colors(color, color_format if color_format is not None else (R.COLOR_RGB8 if color is not None and color.shape[-1] == 3 else R.COLOR_RGBA8))
    assert np.array_equal(rgb, want if want is not None else np.zeros_like(rgb))


def test_probe_depth_bit_exact(hfpf_mod):
    rng = np.random.default_rng(7)
    with hfpf_mod.OccupancyGrid(**DEPTH_CAPS) as g:
        all_counts = np.arange(65536, dtype=np.uint32).astype(np.uint16).reshape(256, 256)  # every count; corners included
        for scale, K in ((0.001, (615.0, 615.0, 319.5, 239.5)), (0.00025, (612.31, 608.93, 121.37, 144.81)),
                         (0.0001, (1000.1, 999.7, 300.3, -17.9)), (0.0010000000474974513, (201.0, 203.5, 0.0, 255.0))):
            _probe_equal(g, all_counts, K, depth_scale=scale)
            _probe_equal(g, all_counts[::-1, ::-1].copy(), K, depth_scale=scale)
        specials = np.array([np.nan, np.inf, -np.inf, -1.5, -0.0, 0.0, 1e-40, 1.4e-45, -3e-39, 1e30, 0.3, 0.45, 65535.0], np.float32)
        f32 = rng.choice(specials, size=(48, 64)).astype(np.float32)
        f32 = np.where(rng.random((48, 64)) < 0.4, rng.uniform(-1, 1, (48, 64)).astype(np.float32), f32).astype(np.float32)
        for K in ((615.0, 615.0, 31.5, 23.5), (400.7, 421.3, 33.21, 20.07)):
            _probe_equal(g, f32, K)
        depth = rng.integers(0, 1200, size=(48, 64)).astype(np.uint16)
        c3 = rng.integers(0, 256, size=(48, 64, 3)).astype(np.uint8)
        c4 = rng.integers(0, 256, size=(48, 64, 4)).astype(np.uint8)
        K = (300.0, 301.0, 31.7, 24.1)
        _probe_equal(g, depth, K, c3, R.COLOR_RGB8)
        _probe_equal(g, depth, K, c3, R.COLOR_BGR8)
        _probe_equal(g, depth, K, c4, R.COLOR_RGBA8)
        _probe_equal(g, depth, K, c4, R.COLOR_BGRA8)
        _probe_equal(g, depth, K)
        # padded rows of both images, and an odd width: the last RGB8 pixel ends the image exactly
        wide_d = rng.integers(0, 1200, size=(37, 61)).astype(np.uint16)
        wide_c = rng.integers(0, 256, size=(37, 67, 3)).astype(np.uint8)
        xyz, rgb = g.probe_depth(wide_d[:, :53], K, color=wide_c[:, :53], color_format=R.COLOR_RGB8)
        ref = R.backproject(np.ascontiguousarray(wide_d[:, :53]), K)
        assert np.array_equal(xyz.view(np.uint32), ref.view(np.uint32))
        assert np.array_equal(rgb, R.colors(np.ascontiguousarray(wide_c[:, :53]), R.COLOR_RGB8))


# ---- whole sessions -------------------------------------------------------------------------------------------------

def test_scene_parity_with_the_cloud_path_and_the_oracle(hfpf_mod, oracle_mod, synth_mod):
    sc = DepthScene(12, 640, 480, clean_every=4)
    clouds = [sc.cloud(f) for f in range(sc.n_frames)]
    got = _depth_session(hfpf_mod, sc)
    ref = _cloud_session(hfpf_mod, sc, clouds)
    _same(got, ref)
    assert got[1]["points_presented"] == 12 * 640 * 480 and got[1]["points_in_bbox"] > 0
    og = oracle_mod.OracleGrid(resolution=0.002, bbox=BBOX, fuse_color=True)
    for ev in sc.schedule():
        if ev[0] == "integrate":
            og.capture(clouds[ev[1]], sc.poses[ev[1]], off_rgb=12)
        else:
            og.clean()
    oref = og.extract()
    assert (oref["rgb"][oref["count"] > 0] != 0).any()
    scenes.compare_rows(oref, got[0])


def test_pinned_and_device_batches_equal_pageable(hfpf_mod, synth_mod):
    sc = DepthScene(8, 320, 240, clean_every=4)
    ref = _depth_session(hfpf_mod, sc)
    # pinned: views of page-locked buffers, untouched until the session syncs
    with grid(hfpf_mod) as g:
        bufs = []

        def pinned(g, f):
            depth, rgb, K = sc.frames[f]
            bd, bc = g.host_alloc(depth.nbytes), g.host_alloc(rgb.nbytes)
            d = bd.view(np.uint16).reshape(depth.shape)
            c = bc.reshape(rgb.shape)
            d[...] = depth
            c[...] = rgb
            bufs.extend((bd, bc))
            g.integrate_depth_pinned(d, sc.poses[f], K, color=c)
        run(g, sc, integrate=pinned)
        got = _result(g)
        for b in bufs:
            g.host_free(b)
    _same(got, ref)
    # device: one launch per clean interval, explicit frame ids in shuffled order
    rng = np.random.default_rng(3)
    depth0, rgb0, K = sc.frames[0]
    dstride, cstride = (depth0.nbytes + 255) & ~255, (rgb0.nbytes + 255) & ~255
    with grid(hfpf_mod) as g:
        dd, dc = g.device_alloc(dstride * sc.n_frames), g.device_alloc(cstride * sc.n_frames)
        desc = hfpf_mod.depth_desc(sc.W, sc.H, hfpf_mod.DEPTH_U16, sc.W * 2, K, hfpf_mod.COLOR_RGB8, sc.W * 3)
        for start in range(0, sc.n_frames, 4):
            ids = rng.permutation(np.arange(start, start + 4)).astype(np.uint32)
            for k, f in enumerate(ids):
                g.device_upload(dd + k * dstride, sc.frames[f][0])
                g.device_upload(dc + k * cstride, sc.frames[f][1])
            g.integrate_depth_device(desc, dd, dstride, 4, np.stack([sc.poses[f].reshape(12) for f in ids]), dev_color=dc,
                                     color_frame_stride=cstride, frame_ids=ids)
            g.clean()
        got = _result(g)
        g.device_free(dd)
        g.device_free(dc)
    _same(got, ref)


_CHILD = textwrap.dedent("""
    import sys
    sys.path[:0] = sys.argv[1].split(":")
    import numpy as np
    import gpu_support as T
    import hfpf
    from scenes import DepthScene
    sc = DepthScene(10, 160, 128, clean_every=5)
    clouds = [sc.cloud(f) for f in range(sc.n_frames)]
    def session(integrate):
        with T.grid(hfpf) as g:
            T.run(g, sc, integrate=integrate)
            return g.extract(), T.counters(g)
    ref = session(lambda g, f: g.integrate(clouds[f], sc.poses[f]))
    def mixed(g, f):
        depth, rgb, K = sc.frames[f]
        if f % 3 == 1:
            g.integrate(clouds[f], sc.poses[f])
        else:
            g.integrate_depth(depth, sc.poses[f], K, color=rgb)
    got = session(mixed)
    assert got[1] == ref[1], "counters differ: %s vs %s" % (got[1], ref[1])
    T.same_records(got[0], ref[0], "rows", "rows")
    print("mixed ok", len(got[0]))
""")


@pytest.mark.parametrize("host_batch", ["1", "4"])
def test_interleaved_cloud_and_depth_frames_equal_all_cloud(hfpf_mod, synth_mod, host_batch):
    here = os.path.dirname(os.path.abspath(__file__))
    path = ":".join(sys.path + [here])
    env = dict(os.environ, HFPF_HOST_BATCH=host_batch)
    r = subprocess.run([sys.executable, "-c", _CHILD, path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "mixed ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _variant(hfpf_mod, sc, make, fuse_color=True):
    """make(f) -> (depth, K, color, color_format, depth_scale, cloud): the depth path against the cloud path."""
    items = [make(f) for f in range(sc.n_frames)]
    with hfpf_mod.OccupancyGrid(resolution=0.002, bbox=BBOX, fuse_color=fuse_color, **DEPTH_CAPS) as g:
        run(g, sc, integrate=lambda g, f: g.integrate_depth(items[f][0], sc.poses[f], items[f][1], color=items[f][2],
                                                            color_format=items[f][3], depth_scale=items[f][4]))
        got = _result(g)
    ref = _cloud_session(hfpf_mod, sc, [it[5] for it in items], fuse_color=fuse_color)
    _same(got, ref)
    assert got[1]["points_in_bbox"] > 0
    return got


def test_formats_and_geometry_equal_the_cloud_path(hfpf_mod, synth_mod):
    # U16 at a quarter millimetre per count, RGB8
    sc = DepthScene(4, 320, 240, clean_every=2, depth_scale=0.00025)
    _variant(hfpf_mod, sc, lambda f: (sc.frames[f][0], sc.frames[f][2], sc.frames[f][1], R.COLOR_RGB8, 0.00025, sc.cloud(f)))
    sc = DepthScene(4, 320, 240, clean_every=2)

    def f32(f):  # metres as f32, with NaN / inf holes and negative depths
        depth, rgb, K = sc.frames[f]
        d = (depth.astype(np.float64) * 0.001).astype(np.float32)
        d[depth == 0] = np.nan
        d[::37, ::11] = np.inf
        d[5::41, 3::13] = -0.4
        bgr = np.ascontiguousarray(rgb[..., ::-1])
        return d, K, bgr, R.COLOR_BGR8, 0.001, R.packed_cloud(d, K, bgr, R.COLOR_BGR8)
    _variant(hfpf_mod, sc, f32)

    def four(fmt):
        def make(f):
            depth, rgb, K = sc.frames[f]
            c4 = np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 0xA5, np.uint8)], axis=-1)
            return depth, K, c4, fmt, 0.001, R.packed_cloud(depth, K, c4, fmt)
        return make
    _variant(hfpf_mod, sc, four(R.COLOR_BGRA8))
    _variant(hfpf_mod, sc, four(R.COLOR_RGBA8))
    got = _variant(hfpf_mod, sc, lambda f: (sc.frames[f][0], sc.frames[f][2], None, None, 0.001, R.packed_cloud(sc.frames[f][0], sc.frames[f][2])))
    assert (got[0]["rgb"] == 0).all()
    _variant(hfpf_mod, sc, lambda f: (sc.frames[f][0], sc.frames[f][2], None, None, 0.001, R.packed_cloud(sc.frames[f][0], sc.frames[f][2])),
             fuse_color=False)

    def padded(f):  # row steps wider than the image (views of wider arrays)
        depth, rgb, K = sc.frames[f]
        wd = np.zeros((sc.H, sc.W + 9), np.uint16)
        wd[:, :sc.W] = depth
        wc = np.zeros((sc.H, sc.W + 5, 3), np.uint8)
        wc[:, :sc.W] = rgb
        return wd[:, :sc.W], K, wc[:, :sc.W], R.COLOR_RGB8, 0.001, sc.cloud(f)
    _variant(hfpf_mod, sc, padded)
    # 424 x 240 does not tile by 16: the linear walk
    sc = DepthScene(4, 424, 240, clean_every=2)
    _variant(hfpf_mod, sc, lambda f: (sc.frames[f][0], sc.frames[f][2], sc.frames[f][1], R.COLOR_RGB8, 0.001, sc.cloud(f)))


def test_bad_arguments_are_refused_and_the_handle_stays_usable(hfpf_mod, synth_mod):
    L = hfpf_mod.lib()
    sc = DepthScene(2, 64, 48, clean_every=0)
    depth, rgb, K = sc.frames[0]
    pose = np.ascontiguousarray(sc.poses[0], np.float64).reshape(12)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def desc(**kw):
        d = hfpf_mod.depth_desc(64, 48, hfpf_mod.DEPTH_U16, 128, K, hfpf_mod.COLOR_RGB8, 192)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    bad = [
        (desc(width=0), p(depth), p(rgb)), (desc(height=0), p(depth), p(rgb)),
        (desc(depth_step=126), p(depth), p(rgb)), (desc(depth_step=129), p(depth), p(rgb)),
        (desc(depth_format=hfpf_mod.DEPTH_F32), p(depth), p(rgb)),  # step 128 < 64 * 4
        (desc(depth_format=7), p(depth), p(rgb)), (desc(color_format=9), p(depth), p(rgb)),
        (desc(color_step=191), p(depth), p(rgb)), (desc(color_format=hfpf_mod.COLOR_RGBA8), p(depth), p(rgb)),
        (desc(fx=0.0), p(depth), p(rgb)), (desc(fy=-1.0), p(depth), p(rgb)), (desc(fx=float("nan")), p(depth), p(rgb)),
        (desc(fy=float("inf")), p(depth), p(rgb)), (desc(cx=float("nan")), p(depth), p(rgb)),
        (desc(depth_scale=0.0), p(depth), p(rgb)), (desc(depth_scale=-0.001), p(depth), p(rgb)),
        (desc(struct_size=64), p(depth), p(rgb)), (desc(reserved=1), p(depth), p(rgb)),
        (desc(), None, p(rgb)), (desc(), p(depth), None), (desc(color_format=hfpf_mod.COLOR_NONE), p(depth), p(rgb)),
    ]
    with grid(hfpf_mod) as g:
        for d, dp, cp in bad:
            assert L.hfpf_integrate_depth(g._h, C.byref(d), dp, cp, p(pose)) == -2, (d.width, d.depth_step, d.color_format)
            assert L.hfpf_probe_depth(g._h, C.byref(d), dp, cp, p(np.zeros(3 * 64 * 48, np.float32)), p(np.zeros(64 * 48, np.uint32))) == -2
        dev = g.device_alloc(1 << 16)
        d = desc()
        assert L.hfpf_integrate_depth_device(g._h, C.byref(d), C.c_void_p(dev + 1), 1 << 14, C.c_void_p(dev + 8192), 0, 1, p(pose), None) == -2
        assert L.hfpf_integrate_depth_device(g._h, C.byref(d), C.c_void_p(dev), 100, C.c_void_p(dev + 8192), 100, 2, p(pose.repeat(2)), None) == -2
        # not page-locked
        assert L.hfpf_integrate_depth_pinned(g._h, C.byref(d), p(depth), p(rgb), p(pose)) == -2
        g.device_free(dev)
        # ... and the same handle integrates a good frame exactly as a fresh one fed the cloud
        g.integrate_depth(depth, sc.poses[0], K, color=rgb)
        g.integrate_depth(sc.frames[1][0], sc.poses[1], K, color=sc.frames[1][1])
        g.clean()
        got = _result(g)
    _same(got, _cloud_session(hfpf_mod, sc))


def test_node_depth_callback_writes_the_same_files(tmp_path, hfpf_mod, synth_mod):
    import hfpf_node
    sc = DepthScene(5, 160, 120, clean_every=0)
    poses = {("base_link", "camera_%d" % f): sc.poses[f] for f in range(sc.n_frames)}
    out = {}
    for kind in ("cloud", "depth"):
        d = tmp_path / kind
        d.mkdir()
        with hfpf_node.FusionNode(bounding_box=list(BBOX), directory_name=str(d), fusion_frame="base_link",
                                  tf_lookup=lambda t, s: poses[(t, s)], clean_period_s=0.0, resolution=0.002, **DEPTH_CAPS) as node:
            depth, rgb, K = sc.frames[0]
            assert (node.publish_depth(depth, K, color=rgb, frame_id="camera_0") if kind == "depth" else
                    node.publish(sc.cloud(0), 1, sc.W * sc.H, frame_id="camera_0")) == 0  # not started
            node.start()
            for f in range(sc.n_frames):
                depth, rgb, K = sc.frames[f]
                rc = (node.publish_depth(depth, K, color=rgb, frame_id="camera_%d" % f) if kind == "depth" else
                      node.publish(sc.cloud(f), 1, sc.W * sc.H, frame_id="camera_%d" % f))
                assert rc == 1
                if f == 2:
                    assert node.clean_now() == 1
            stats = node.stats()
            rc, ok, msg = node.process()
            assert rc == 0 and ok
        out[kind] = ((d / "test_cloud.pcd").read_bytes(), (d / "meta.csv").read_bytes(), stats)
    assert out["depth"][0] == out["cloud"][0] and out["depth"][1] == out["cloud"][1]
    assert out["depth"][2] == out["cloud"][2]
    assert out["depth"][0].count(b"\n") > 20


def test_two_virtual_ranks_equal_one_handle(hfpf_mod, synth_mod):
    import hfpf_dist
    sc = DepthScene(6, 160, 128, clean_every=3)
    ref = _depth_session(hfpf_mod, sc)
    grids = [grid(hfpf_mod) for _ in range(2)]
    vr = hfpf_dist.LocalVirtualRanks(grids)
    depth0, rgb0, K = sc.frames[0]
    desc = hfpf_mod.depth_desc(sc.W, sc.H, hfpf_mod.DEPTH_U16, sc.W * 2, K, hfpf_mod.COLOR_RGB8, sc.W * 3)
    try:
        for ev in sc.schedule():
            if ev[0] == "integrate":
                f = ev[1]
                g = grids[f % 2]
                dd, dc = g.device_alloc(depth0.nbytes), g.device_alloc(rgb0.nbytes)
                g.device_upload(dd, sc.frames[f][0])
                g.device_upload(dc, sc.frames[f][1])
                g.integrate_depth_device(desc, dd, depth0.nbytes, 1, sc.poses[f].reshape(1, 12), dev_color=dc,
                                         color_frame_stride=rgb0.nbytes, frame_ids=np.array([f], np.uint32))
                g.sync()
                g.device_free(dd)
                g.device_free(dc)
            else:
                vr.clean_all()
        rows = vr.extract(on=1)
        presented = sum(g.counters()["points_presented"] for g in grids)
    finally:
        for g in grids:
            g.close()
    assert rows.tobytes() == ref[0].tobytes()
    assert presented == ref[1]["points_presented"]
