"""The depth-frame contract of include/hfpf.h restated in numpy (imported by tests only): registered depth + colour images and
intrinsics -> the organised cloud the engine defines a depth frame to be, as packed 16-byte records (x, y, z f32, rgb u32).
Every operation f32, left to right, one rounding each, as the engine evaluates it."""
import numpy as np

U16, F32 = 1, 2
COLOR_NONE, COLOR_RGB8, COLOR_BGR8, COLOR_RGBA8, COLOR_BGRA8 = 0, 1, 2, 3, 4
NAN_BITS = np.uint32(0x7FC00000)


def constants(depth_format, K, depth_scale=0.001):
    """(cxf, cyf, sx, sy, unit) rounded from their doubles as the host rounds them."""
    fx, fy, cx, cy = (float(k) for k in K)
    cxf, cyf = np.float32(cx), np.float32(cy)
    if depth_format == U16:
        unit = np.float32(depth_scale)
        return cxf, cyf, np.float32(float(unit) / fx), np.float32(float(unit) / fy), unit
    return cxf, cyf, np.float32(1.0 / fx), np.float32(1.0 / fy), np.float32(1.0)


def backproject(depth, K, depth_scale=0.001):
    """depth: HxW uint16 (counts) or float32 (metres).  Returns (H*W, 3) float32, NaN (0x7FC00000) for invalid pixels."""
    H, W = depth.shape
    fmt = U16 if depth.dtype == np.uint16 else F32
    cxf, cyf, sx, sy, unit = constants(fmt, K, depth_scale)
    u = np.broadcast_to(np.arange(W, dtype=np.float32)[None, :], (H, W))
    v = np.broadcast_to(np.arange(H, dtype=np.float32)[:, None], (H, W))
    with np.errstate(invalid="ignore", over="ignore"):
        if fmt == U16:
            valid = depth != 0
            d = depth.astype(np.float32)
            z = (d * unit).astype(np.float32)
        else:
            d = depth.astype(np.float32)
            valid = np.isfinite(d)
            z = d
        x = (((u - cxf).astype(np.float32) * d).astype(np.float32) * sx).astype(np.float32)
        y = (((v - cyf).astype(np.float32) * d).astype(np.float32) * sy).astype(np.float32)
    xyz = np.stack([x, y, z], axis=-1).reshape(-1, 3).copy()
    xyz.view(np.uint32)[~valid.reshape(-1)] = NAN_BITS
    return xyz


def colors(color, color_format):
    """HxWxC uint8 image -> H*W uint32 0x00RRGGBB (alpha dropped); None / COLOR_NONE -> zeros."""
    if color is None or color_format == COLOR_NONE:
        return None
    c = color.reshape(-1, color.shape[-1]).astype(np.uint32)
    if color_format in (COLOR_BGR8, COLOR_BGRA8):
        r, g, b = c[:, 2], c[:, 1], c[:, 0]
    else:
        r, g, b = c[:, 0], c[:, 1], c[:, 2]
    return (r << 16) | (g << 8) | b


def packed_cloud(depth, K, color=None, color_format=None, depth_scale=0.001):
    """The equivalent packed cloud: H*W records of 16 bytes as a flat uint8 array (hfpf_integrate's default layout)."""
    if color is not None and color_format is None:
        color_format = COLOR_RGB8 if color.shape[-1] == 3 else COLOR_RGBA8
    xyz = backproject(depth, K, depth_scale)
    rec = np.zeros((xyz.shape[0], 4), np.uint32)
    rec[:, :3] = xyz.view(np.uint32)
    rgb = colors(color, color_format)
    if rgb is not None:
        rec[:, 3] = rgb
    return rec.view(np.uint8).reshape(-1)
