"""The render contract of include/hfpf.h restated in numpy (imported by tests only): extracted rows + a camera -> the depth, normal,
rgb, count and voxel planes hfpf_render draws.  Every operation f64, left to right, one rounding each, as the engine evaluates
it; the winner of a pixel is the minimum of the uint64 words bits(depth32) << 32 | row, reduced with np.minimum.at."""
import numpy as np

CULL_BACKFACES, WORLD_NORMALS = 1, 2
NAN_BITS = np.uint32(0x7FC00000)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def drawn_rows(rows, min_count=0.0):
    """The row set of a render: count >= max(1, min_count), compared as hfpf_extract_opts compares ((double)(int)count)."""
    c = rows["count"].astype(np.int64).astype(np.int32).astype(np.float64)
    return rows[~(c < max(1.0, float(min_count)))]


def auto_radius(res, fx, fy, zc, max_radius):
    """min(max_splat_radius, floor(((0.5 * res) * max(fx, fy)) / zc))."""
    r = np.floor(((0.5 * float(res)) * max(float(fx), float(fy))) / np.asarray(zc, dtype=np.float64))
    return np.minimum(r, float(max_radius)).astype(np.int64)


def project(rows, pose, K, z_range, cull=False):
    """Per row: (mask of rows drawn before the image bounds, zc, pu, pv) -- the arithmetic of the splat."""
    T = np.asarray(pose, dtype=np.float64).reshape(12)
    fx, fy, cx, cy = (float(k) for k in K)
    x, y, z = (rows[k].astype(np.float64) for k in ("x", "y", "z"))
    dx, dy, dz = x - T[3], y - T[7], z - T[11]
    xc = (T[0] * dx + T[4] * dy) + T[8] * dz
    yc = (T[1] * dx + T[5] * dy) + T[9] * dz
    zc = (T[2] * dx + T[6] * dy) + T[10] * dz
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = (float(z_range[0]) < zc) & (zc < float(z_range[1]))
        if cull:
            nx, ny, nz = (rows[k].astype(np.float64) for k in ("nx", "ny", "nz"))
            ok &= ((nx * dx + ny * dy) + nz * dz) < 0.0
        u = (xc / zc) * fx + cx
        v = (yc / zc) * fy + cy
        ok &= (np.abs(u) < 2.0 ** 30) & (np.abs(v) < 2.0 ** 30)
        pu = np.where(ok, np.floor(u + 0.5), 0.0).astype(np.int64)
        pv = np.where(ok, np.floor(v + 0.5), 0.0).astype(np.int64)
    return ok, zc, pu, pv


def zbuffer(rows, pose, K, width, height, res, z_range=(0.01, 100.0), min_count=0.0, splat_radius=0, max_splat_radius=4, flags=0):
    """(drawn rows, uint64 z-buffer of width * height words; all ones = empty)."""
    rows = drawn_rows(rows, min_count)
    zb = np.full(width * height, EMPTY, dtype=np.uint64)
    ok, zc, pu, pv = project(rows, pose, K, z_range, cull=bool(flags & CULL_BACKFACES))
    idx = np.flatnonzero(ok)
    if idx.size == 0:
        return rows, zb
    zc, pu, pv = zc[idx], pu[idx], pv[idx]
    fx, fy = float(K[0]), float(K[1])
    r = np.full(idx.size, int(splat_radius), np.int64) if splat_radius >= 0 else auto_radius(res, fx, fy, zc, max_splat_radius)
    words = (zc.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    for rad in np.unique(r):
        sel = np.flatnonzero(r == rad)
        off = np.arange(-rad, rad + 1, dtype=np.int64)
        px = (pu[sel][:, None, None] + off[None, None, :]).repeat(off.size, axis=1)
        py = (pv[sel][:, None, None] + off[None, :, None]).repeat(off.size, axis=2)
        w = np.broadcast_to(words[sel][:, None, None], px.shape)
        inside = (px >= 0) & (px < width) & (py >= 0) & (py < height)
        np.minimum.at(zb, (py * width + px)[inside], w[inside])
    return rows, zb


def render(rows, pose, K, width, height, res, z_range=(0.01, 100.0), min_count=0.0, splat_radius=0, max_splat_radius=4, flags=0):
    """{depth, normal, rgb, count, voxel} planes of one view, shaped as OccupancyGrid.render returns them."""
    rows, zb = zbuffer(rows, pose, K, width, height, res, z_range, min_count, splat_radius, max_splat_radius, flags)
    full = zb != EMPTY
    row = (zb[full] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    win = rows[row]
    n = width * height
    depth = np.full(n, NAN_BITS, np.uint32)
    depth[full] = (zb[full] >> np.uint64(32)).astype(np.uint32)
    normal = np.full((n, 3), NAN_BITS, np.uint32)
    nrm = np.stack([win["nx"], win["ny"], win["nz"]], axis=-1).astype(np.float32)
    if not flags & WORLD_NORMALS:
        T = np.asarray(pose, dtype=np.float64).reshape(12)
        nx, ny, nz = (win[k].astype(np.float64) for k in ("nx", "ny", "nz"))
        nrm = np.stack([(T[0] * nx + T[4] * ny) + T[8] * nz, (T[1] * nx + T[5] * ny) + T[9] * nz,
                        (T[2] * nx + T[6] * ny) + T[10] * nz], axis=-1).astype(np.float32)
    normal[full] = nrm.view(np.uint32)
    rgb = np.zeros(n, np.uint32)
    rgb[full] = win["rgb"]
    count = np.zeros(n, np.uint32)
    count[full] = win["count"]
    voxel = np.full((n, 3), -1, np.int32)
    voxel[full] = np.stack([win["ix"], win["iy"], win["iz"]], axis=-1)
    return {"depth": depth.view(np.float32).reshape(height, width), "normal": normal.view(np.float32).reshape(height, width, 3),
            "rgb": rgb.reshape(height, width), "count": count.reshape(height, width), "voxel": voxel.reshape(height, width, 3)}
