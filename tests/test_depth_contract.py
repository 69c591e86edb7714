"""CPU: the depth-frame contract (tests/depth_ref.py) on hand-computed pixels, and the synthetic sensor's depth rendering
(hfpf_synth_depth_frame): deterministic, and the same scene as its float cloud."""
import numpy as np

import depth_ref as R


def test_u16_hand_computed_values_and_invalid_pixels():
    # fx = fy = 2, depth_scale = 0.25: sx = sy = 0.125 and every product below is exact
    depth = np.array([[0, 4, 8], [4, 0, 2]], np.uint16)
    xyz = R.backproject(depth, (2.0, 2.0, 1.0, 0.5), depth_scale=0.25)
    bits = xyz.view(np.uint32)
    assert (bits[0] == R.NAN_BITS).all() and (bits[4] == R.NAN_BITS).all()
    # (u, v) = (1, 0), d = 4: x = ((1 - 1) * 4) * 0.125 = 0, y = ((0 - 0.5) * 4) * 0.125 = -0.25, z = 4 * 0.25 = 1
    assert xyz[1].tolist() == [0.0, -0.25, 1.0]
    # (2, 0), d = 8: x = ((2 - 1) * 8) * 0.125 = 1, y = -0.5, z = 2
    assert xyz[2].tolist() == [1.0, -0.5, 2.0]
    # (0, 1), d = 4: x = -0.5, y = 0.25, z = 1;  (2, 1), d = 2: x = 0.25, y = 0.125, z = 0.5
    assert xyz[3].tolist() == [-0.5, 0.25, 1.0]
    assert xyz[5].tolist() == [0.25, 0.125, 0.5]


def test_u16_rounding_follows_the_contract():
    # a non-trivial scale: sx = (float)((double)(float)0.001 / fx), products rounded one at a time
    depth = np.array([[523]], np.uint16)
    K = (615.3, 611.7, -0.37, 0.0)
    xyz = R.backproject(depth, K, depth_scale=0.001)
    unit = np.float32(0.001)
    sx = np.float32(float(unit) / 615.3)
    x = np.float32(np.float32(np.float32(0.0) - np.float32(-0.37)) * np.float32(523.0)) * sx
    assert xyz[0, 0].view(np.uint32) == np.float32(x).view(np.uint32)
    assert xyz[0, 2].view(np.uint32) == np.float32(np.float32(523.0) * unit).view(np.uint32)
    assert xyz[0, 1] == 0.0


def test_f32_hand_computed_values_and_invalid_pixels():
    depth = np.array([[np.nan, np.inf, -np.inf, 2.0, -2.0, 0.0]], np.float32)
    xyz = R.backproject(depth, (4.0, 4.0, 1.0, 0.0))  # sx = 0.25
    bits = xyz.view(np.uint32)
    assert (bits[:3] == R.NAN_BITS).all()
    assert xyz[3].tolist() == [1.0, 0.0, 2.0]       # ((3 - 1) * 2) * 0.25
    assert xyz[4].tolist() == [-1.5, -0.0, -2.0]    # negative depths are valid (they fail the z-clip later)
    assert xyz[5].tolist() == [0.0, 0.0, 0.0]


def test_colour_formats():
    px = np.array([[[0x11, 0x22, 0x33, 0x44]]], np.uint8)
    assert R.colors(px[..., :3], R.COLOR_RGB8)[0] == 0x112233
    assert R.colors(px[..., :3], R.COLOR_BGR8)[0] == 0x332211
    assert R.colors(px, R.COLOR_RGBA8)[0] == 0x112233
    assert R.colors(px, R.COLOR_BGRA8)[0] == 0x332211
    cloud = R.packed_cloud(np.array([[7]], np.uint16), (1.0, 1.0, 0.0, 0.0), color=px, color_format=R.COLOR_BGRA8)
    assert cloud.view(np.uint32)[3] == 0x332211
    assert R.packed_cloud(np.array([[7]], np.uint16), (1.0, 1.0, 0.0, 0.0)).view(np.uint32)[3] == 0


def test_synth_depth_frame_is_deterministic(synth_mod):
    S = synth_mod
    pose = S.pose(0x5E3, 2)
    a = S.depth_frame(0xF051, 2, 160, 120, pose)
    b = S.depth_frame(0xF051, 2, 160, 120, pose)
    c = S.depth_frame(0xF051, 3, 160, 120, pose)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert not np.array_equal(a[0], c[0])
    assert a[2] == (615.0 * 160 / 640, 615.0 * 160 / 640, 79.5, 59.5)


def test_synth_depth_frame_describes_the_same_scene_as_its_cloud(synth_mod):
    S = synth_mod
    W, H = 320, 240
    for f, scale in ((0, 0.001), (5, 0.00025)):
        pose = S.pose(0x5E3, f)
        depth, rgb, K = S.depth_frame(0xF051, f, W, H, pose, depth_scale=scale)
        cloud = S.frame(0xF051, f, W, H, pose).view(np.float32).reshape(-1, 4)
        valid_cloud = np.isfinite(cloud[:, 2])
        valid = depth.reshape(-1) != 0
        assert np.array_equal(valid, valid_cloud)  # 0 exactly where the synth emits NaN (every depth here is in range)
        assert valid.mean() > 0.9
        xyz = R.backproject(depth, K, depth_scale=scale)
        d = np.abs(xyz[valid].astype(np.float64) - cloud[valid, :3].astype(np.float64))
        assert d.max() <= scale, "back-projected depth frame %d is %.3g m from the synth's cloud" % (f, d.max())
        # the colour image carries the cloud's rgb field
        assert np.array_equal(R.colors(rgb, R.COLOR_RGB8), cloud[:, 3].view(np.uint32))


def test_python_descriptor_follows_numpy_strides(hfpf_mod):
    depth = np.zeros((48, 80), np.uint16)[:, :64]  # padded rows: step = 160 bytes
    color = np.zeros((48, 70, 4), np.uint8)[:, :64]
    d = hfpf_mod._image_desc(depth, (500.0, 501.0, 31.5, 23.5), color, None, 0.001)
    assert (d.width, d.height, d.depth_format, d.depth_step) == (64, 48, hfpf_mod.DEPTH_U16, 160)
    assert (d.color_format, d.color_step) == (hfpf_mod.COLOR_RGBA8, 280)
    assert d.struct_size == 72
    d = hfpf_mod._image_desc(np.zeros((4, 4), np.float32), (1, 1, 0, 0), None, None, 0.001)
    assert (d.depth_format, d.depth_step, d.color_format) == (hfpf_mod.DEPTH_F32, 16, hfpf_mod.COLOR_NONE)
