"""Plain numpy restatement of the engine's statistics contract (csrc/stats.hpp, csrc/kernels.hpp record_centroid / record_row,
csrc/hfpf.hip setup_params): fixed-point scales from the config, one member's contribution, and "words -> row".  Independent of
the C++ oracle: sums are np.int64 (or Python ints), the row expression is f64 in the engine's operation order (numpy never fuses),
narrowed to f32 once at the end.  Imported by tests only."""
import math

import numpy as np

ROW_DTYPE = np.dtype(
    [
        ("ix", "<i4"), ("iy", "<i4"), ("iz", "<i4"), ("count", "<u4"),
        ("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
        ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
        ("sdx", "<f4"), ("sdy", "<f4"), ("sdz", "<f4"),
        ("mean_dist", "<f4"), ("sd_dist", "<f4"), ("rgb", "<u4"),
    ]
)
FLOAT_COLUMNS = ("x", "y", "z", "sdx", "sdy", "sdz", "mean_dist", "sd_dist")
SW_COUNT, SW_S, SW_SS, SW_D, SW_DD, SW_R, SW_G, SW_B = range(8)
ONE_CONTRIBUTION = 1 << 27  # every single contribution is below this in magnitude (stats.hpp)


def bounds(K, resolution, ball_radius, cylinder_radius):
    """(Bm, Bm^2, r, r^2): the magnitude bounds of u = s - 0.5, u^2, dist and dist^2 that the scales are chosen from.
    resolution passes through f32 as in hfpf_config / setResolution(float)."""
    res = float(np.float32(resolution))
    Bs = 0.5 + (float(K) + 2.0) * res / (2.0 * float(ball_radius))
    Bm = Bs - 0.5
    r = float(cylinder_radius)
    return Bm, Bm * Bm, r, r * r


def scale_for(bound):
    """2^(26 - floor(log2 bound)): a value below `bound` scaled by it stays below 2^27."""
    return np.float32(math.ldexp(1.0, 26 - int(math.floor(math.log2(bound)))))


def scales(K=3, resolution=0.005, ball_radius=0.015, cylinder_radius=0.001):
    """(fs, fss, fd, fdd) as f32 powers of two."""
    return np.array([scale_for(b) for b in bounds(K, resolution, ball_radius, cylinder_radius)], dtype=np.float32)


def contribution(s, d, sc):
    """The four integers one member adds to words 1-4 (pair_delta): s = projection parameter, d = distance, both f32; f32
    arithmetic, rint = round to nearest even, widened to int64."""
    s = np.asarray(s, dtype=np.float32)
    d = np.asarray(d, dtype=np.float32)
    fs, fss, fd, fdd = (np.float32(v) for v in sc)
    u = s - np.float32(0.5)
    return (np.rint(u * fs).astype(np.int64), np.rint((u * u) * fss).astype(np.int64),
            np.rint(d * fd).astype(np.int64), np.rint((d * d) * fdd).astype(np.int64))


def voxel_centers(idx, bbox_min, resolution):
    """f64 `min + res*i + res/2`, narrowed to f32 (OccupancyGrid.hpp:131-135)."""
    res = float(np.float32(resolution))
    idx = np.asarray(idx, dtype=np.float64).reshape(-1, 3)
    mn = np.asarray(bbox_min, dtype=np.float64).reshape(1, 3)
    return ((mn + res * idx) + res / 2.0).astype(np.float32)


def lines(centres, normals, ball_radius):
    """The f32 segment of a voxel (OccupancyGrid.hpp:40-49): a = centre - r*n, ab = a - (centre + r*n)."""
    c = np.asarray(centres, dtype=np.float32).reshape(-1, 3)
    n = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    d = np.float32(ball_radius) * n
    a = c - d
    b = c + d
    return a, a - b


def row_floats(m, a, ab, sc):
    """Words -> the eight float columns.  m: (n, >=5) int64 words (Python ints allowed: object arrays are converted); a, ab: (n, 3)
    f32 line; sc: the four scales.  Returns a dict of f32 arrays named as FLOAT_COLUMNS."""
    m = np.asarray(m)
    if m.dtype == object:
        m = m.astype(np.int64)
    m = m.reshape(-1, m.shape[-1])
    a = np.asarray(a, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    ab = np.asarray(ab, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    fs, fss, fd, fdd = (float(np.float32(v)) for v in sc)
    cnt = m[:, SW_COUNT]
    live = cnt > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / cnt.astype(np.float64)
        em = (m[:, SW_S].astype(np.float64) / fs) * inv
        es = 0.5 + em
        xyz = a - es[:, None] * ab
        vs = (m[:, SW_SS].astype(np.float64) / fss) * inv - em * em
        md = (m[:, SW_D].astype(np.float64) / fd) * inv
        vd = (m[:, SW_DD].astype(np.float64) / fdd) * inv - md * md
        one = cnt == 1
        vs = np.where(one, 0.0, vs)
        vd = np.where(one, 0.0, vd)
        vs = np.maximum(vs, 0.0)
        vd = np.maximum(vd, 0.0)
        sd = ab * ab * vs[:, None]
    out = {}
    z32 = np.float32(0.0)
    for i, f in enumerate(("x", "y", "z")):
        out[f] = np.where(live, xyz[:, i].astype(np.float32), z32)
    for i, f in enumerate(("sdx", "sdy", "sdz")):
        out[f] = np.where(live, sd[:, i].astype(np.float32), z32)
    out["mean_dist"] = np.where(live, md.astype(np.float32), z32)
    out["sd_dist"] = np.where(live, vd.astype(np.float32), z32)
    return out


def row_rgb(m, color):
    """Mean colour per channel, round half up: floor(sum / cnt + 1/2) in integers, 0x00RRGGBB; 0 without colour or members."""
    m = np.asarray(m, dtype=np.int64)
    cnt = m[:, SW_COUNT]
    if not color:
        return np.zeros(len(m), np.uint32)
    safe = np.maximum(cnt, 1)
    ch = [np.minimum((2 * m[:, w] + cnt) // (2 * safe), 255).astype(np.uint32) for w in (SW_R, SW_G, SW_B)]
    return np.where(cnt > 0, (ch[0] << 16) | (ch[1] << 8) | ch[2], 0).astype(np.uint32)


def rows_from_moments(mom, normals, bbox_min, resolution=0.005, K=3, ball_radius=0.015, cylinder_radius=0.001, color=False):
    """Whole rows from moment records (fields ix, iy, iz, m) and the rows' normals (n, 3) f32."""
    idx = np.stack([mom["ix"], mom["iy"], mom["iz"]], axis=1)
    normals = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    a, ab = lines(voxel_centers(idx, bbox_min, resolution), normals, ball_radius)
    fl = row_floats(mom["m"], a, ab, scales(K, resolution, ball_radius, cylinder_radius))
    rows = np.zeros(len(mom), ROW_DTYPE)
    rows["ix"], rows["iy"], rows["iz"] = mom["ix"], mom["iy"], mom["iz"]
    rows["count"] = mom["m"][:, SW_COUNT].astype(np.uint32)
    rows["nx"], rows["ny"], rows["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
    for f in FLOAT_COLUMNS:
        rows[f] = fl[f]
    rows["rgb"] = row_rgb(mom["m"], color)
    return rows


# ---- configurations with a bound on either side of a power of two (what the scale tests run) ----

def floor_log2(b):
    m, e = math.frexp(b)  # b = m * 2^e, 0.5 <= m < 1: exact, no logarithm
    return e - 1


def straddles():
    """(K, resolution, ball_radius below, ball_radius above, which bound) with Bm (or Bm^2) on either side of a power of two, found
    by stepping ball_radius through neighbouring doubles around (K + 2) res / (2 target)."""
    found = []
    for K in (1, 3, 5):
        for res in (0.001, 0.005):
            res32 = float(np.float32(res))
            for which, target in ((0, 0.25), (0, 1.0), (0, 4.0), (1, math.sqrt(0.5)), (1, math.sqrt(2.0)), (1, math.sqrt(8.0))):
                ball = (K + 2.0) * res32 / (2.0 * target)
                want = floor_log2(target * target * 1.0000001) if which else floor_log2(target)
                lo = hi = ball
                for _ in range(64):  # walk to a pair of neighbouring doubles with the bound's exponent on either side
                    if floor_log2(bounds(K, res, lo, 0.001)[which]) >= want:
                        lo = math.nextafter(lo, math.inf)  # larger radius, smaller bound
                    if floor_log2(bounds(K, res, hi, 0.001)[which]) < want:
                        hi = math.nextafter(hi, 0.0)
                e_lo, e_hi = (floor_log2(bounds(K, res, b, 0.001)[which]) for b in (lo, hi))
                if e_lo == want - 1 and e_hi == want and abs(lo - hi) <= 4 * math.ulp(ball):
                    found.append((K, res, lo, hi, which))
    return found


STRADDLES = straddles()
# the combination the scene tests (CPU and GPU) run: K = 3 at 1 mm, Bm across 2^-2, i.e. ball_radius across 10 mm
STRADDLE_SCENE = next(s for s in STRADDLES if s[0] == 3 and s[1] == 0.001 and s[4] == 0 and 0.009 < s[2] < 0.011)
