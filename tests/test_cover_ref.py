"""CPU: the coverage contract (tests/cover_ref.py) on hand-built cases with known answers and against an independent brute force, and
hfpf_check_cover_opts through the built library (host code, no GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cover_ref as V
import hfpf
import query_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.002
BBOX = (0.0, 0.1, 0.0, 0.1, 0.0, 0.1)  # 50 cells per axis
NO_ROWS = np.zeros(0, hfpf.ROW_DTYPE)


def cover(rows, verts, tris, pose=V.IDENT, occ=None, **kw):
    occ = np.stack([rows["ix"], rows["iy"], rows["iz"]], axis=1) if occ is None else occ
    return V.cover(rows, occ, np.asarray(verts, np.float32), 12, np.asarray(tris, np.uint32), pose, BBOX, RES, **kw)


# ---- (a) the sample pattern ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 7, 64])
def test_sample_pattern(n):
    i, j, kind = V.sub_triangles(n)
    assert len(set(zip(i.tolist(), j.tolist(), kind.tolist()))) == n * n == len(i)
    assert ((kind == 0) | (kind == 1)).all() and (i >= 0).all() and (j >= 0).all() and (i + j + kind <= n - 1).all()
    v, w = V.barycentric(n)
    assert len(set(zip(v.tolist(), w.tolist()))) == n * n, "the samples are distinct"
    assert (v > 0).all() and (w > 0).all() and (v + w < 1).all(), "strictly inside the simplex"
    assert abs(v.mean() - 1 / 3) < 1e-12 and abs(w.mean() - 1 / 3) < 1e-12
    # every sample against the centroid of its sub-triangle, from the sub-triangle's own corners
    rng = np.random.default_rng(n)
    A, B, Cc = rng.uniform(-1, 1, (3, 3))
    ab, ac = B - A, Cc - A
    tri, S = V.sample_points(A[None], ab[None], ac[None], np.array([n], np.uint32))
    assert (tri == 0).all() and S.shape == (n * n, 3)

    def corner(a, b):
        return A + (a / n)[:, None] * ab + (b / n)[:, None] * ac

    up = kind == 0
    cen = np.where(up[:, None], (corner(i, j) + corner(i + 1, j) + corner(i, j + 1)) / 3, (corner(i + 1, j) + corner(i, j + 1) + corner(i + 1, j + 1)) / 3)
    scale = max(np.linalg.norm(ab), np.linalg.norm(ac), np.linalg.norm(A))
    assert np.abs(S - cen).max() <= 1e-12 * scale


# ---- (b) the subdivision thresholds --------------------------------------------------------------------------------------

def _isosceles(L):
    """Longest edge exactly L (f32): A -> B along x, C above its middle at height L / 2."""
    L = np.float32(L)
    return np.array([[0, 0, 0], [L, 0, 0], [L / 2, L / 2, 0]], np.float32) + np.float32(0.25), np.array([[0, 1, 2]], np.uint32)


@pytest.mark.parametrize("L, n, capped", [(0.25, 1, False), (0.25 * (1 + 2.0 ** -20), 2, False), (2.0, 8, False), (2.0 * (1 + 2.0 ** -20), 8, True),
                                          (0.5, 2, False), (0.5 * (1 + 2.0 ** -20), 3, False), (0.01, 1, False)])
def test_subdivision_thresholds(L, n, capped):
    cov, s = cover(NO_ROWS, *_isosceles(L), spacing=0.25, max_subdivision=8)
    assert cov["n_samples"][0] == n * n and cov["flags"][0] == V.VALID | (V.CAPPED if capped else 0)
    assert s["n_samples"] == n * n and s["n_tris_valid"] == 1 and s["n_covered"] == 0


# ---- (c) a flat patch of rows against an independent brute force ---------------------------------------------------------

def patch_rows(x0=10, y0=10, z=20, n=24):
    r = np.zeros(n * n, hfpf.ROW_DTYPE)
    ix, iy = np.meshgrid(np.arange(x0, x0 + n), np.arange(y0, y0 + n), indexing="ij")  # lexicographic (ix, iy, iz)
    r["ix"], r["iy"], r["iz"] = ix.ravel(), iy.ravel(), z
    for k, c in (("x", r["ix"]), ("y", r["iy"]), ("z", r["iz"])):
        r[k] = ((c + 0.5) * RES).astype(np.float32)
    r["nz"], r["count"] = 1.0, 5
    return r


def quad(x=(22, 46), y=(12, 29), z=20.8, reverse=False):
    v = np.array([[x[0], y[0], z], [x[1], y[0], z], [x[1], y[1], z], [x[0], y[1], z]], np.float64) * RES
    t = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    return v.astype(np.float32), (t[:, ::-1].copy() if reverse else t)


def brute_force(rows, verts, tris, spacing, max_distance, max_subdivision=64):
    """Records by a double loop over every sample and every row: no window, no query_ref."""
    out = np.zeros(len(tris), V.TRI_COVERAGE_DTYPE)
    P = np.stack([rows[k].astype(np.float64) for k in ("x", "y", "z")], axis=1)
    lo, hi = np.asarray(BBOX)[0::2], np.asarray(BBOX)[1::2]
    for k, t in enumerate(tris):
        A, B, Cc = (verts[i].astype(np.float64) for i in t)
        L = max(np.sqrt(((B - A) ** 2).sum()), np.sqrt(((Cc - A) ** 2).sum()), np.sqrt(((Cc - B) ** 2).sum()))
        n = int(min(max(np.ceil(L / spacing), 1), max_subdivision))
        dist = []
        for i in range(n):
            for j in range(n - i):
                for kind in (0, 1):
                    if kind and i + j > n - 2:
                        continue
                    v, w = (3 * i + 1 + kind) / (3.0 * n), (3 * j + 1 + kind) / (3.0 * n)
                    p = ((A + v * (B - A)) + w * (Cc - A)).astype(np.float32).astype(np.float64)
                    out["n_samples"][k] += 1
                    if not ((p > lo) & (p < hi)).all():
                        continue
                    out["n_in_bbox"][k] += 1
                    d = p - P
                    d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).min()
                    if d2 <= max_distance * max_distance:
                        dist.append(np.float32(np.sqrt(d2)))
        out["n_covered"][k] = len(dist)
        out["flags"][k] = V.VALID
        out["area"][k] = np.float32(0.5 * np.linalg.norm(np.cross(B - A, Cc - A)))
        out["max_distance"][k] = max(dist) if dist else 0.0
        out["sum_dist_q30"][k] = sum(int(np.rint(float(d) * 2.0 ** 30)) for d in dist)
    return out


def test_flat_patch_against_brute_force():
    rows = patch_rows()
    radius, md = 2, 2 * RES
    # the precondition that makes the windowed search and the plain double loop agree
    assert md <= radius * RES
    own = Q.voxel(np.stack([rows["x"], rows["y"], rows["z"]], axis=1), BBOX, RES)
    assert (own == np.stack([rows["ix"], rows["iy"], rows["iz"]], axis=1)).all(), "every centroid lies in its own voxel"
    verts, tris = quad()
    cov, s = cover(rows, verts, tris, radius=radius, max_distance=md, spacing=RES)
    ref = brute_force(rows, verts, tris, RES, md)
    for k in ("n_samples", "n_in_bbox", "n_covered", "flags", "max_distance", "sum_dist_q30"):
        assert (cov[k] == ref[k]).all(), (k, cov[k], ref[k])
    assert np.abs(cov["area"] - ref["area"]).max() <= 1e-6 * ref["area"].max()  # the brute force's area goes through a norm, not NN
    assert (cov["n_samples"] == 30 * 30).all()
    assert 0 < s["n_covered"] < s["n_samples"] and (cov["n_covered"] > 0).all() and (cov["n_covered"] < cov["n_samples"]).all()
    assert s["n_in_bbox"] == s["n_samples"]
    for k in ("n_samples", "n_in_bbox", "n_covered", "sum_dist_q30"):
        assert s[k] == sum(int(x) for x in cov[k])
    assert s["max_distance"] == float(cov["max_distance"].max()) and s["pad"] == 0
    area = ((s["area_q40_hi"] << 32) + s["area_q40_lo"]) / 2.0 ** 40
    covered = ((s["covered_q40_hi"] << 32) + s["covered_q40_lo"]) / 2.0 ** 40
    assert abs(area - 24 * 17 * RES * RES) < 1e-9 and abs(covered / area - s["n_covered"] / s["n_samples"]) < 1e-9
    # the normal gate: the rows look to +z, as the quad does
    gated = cover(rows, verts, tris, radius=radius, max_distance=md, spacing=RES, min_normal_dot=0.5)
    assert gated[0].tobytes() == cov.tobytes() and gated[1] == s
    rv, rt = quad(reverse=True)
    back = cover(rows, rv, rt, radius=radius, max_distance=md, spacing=RES, min_normal_dot=0.5)
    assert back[1]["n_covered"] == 0 and back[1]["n_in_bbox"] == s["n_in_bbox"] and back[1]["sum_dist_q30"] == 0 and back[1]["max_distance"] == 0.0
    both = cover(rows, rv, rt, radius=radius, max_distance=md, spacing=RES, min_normal_dot=0.5, abs_normal=True)
    off = cover(rows, rv, rt, radius=radius, max_distance=md, spacing=RES)
    assert both[0].tobytes() == off[0].tobytes() and both[1] == off[1]
    assert both[1]["n_covered"] == s["n_covered"] and both[1]["sum_dist_q30"] == s["sum_dist_q30"]
    # min_count above the rows' count leaves nothing to cover
    assert cover(rows, verts, tris, radius=radius, max_distance=md, spacing=RES, min_count=6.0)[1]["n_covered"] == 0


# ---- (d), (e) invalid and huge triangles -----------------------------------------------------------------------------------

def test_invalid_triangles_have_zero_records_and_are_counted():
    rows = patch_rows()
    verts, tris = quad()
    verts = np.vstack([verts, [[np.nan, 0.05, 0.05]], [[0.01, 0.01, 0.01]], [[0.02, 0.02, 0.02]], [[0.03, 0.03, 0.03]]]).astype(np.float32)
    tris = np.vstack([tris, [[0, 1, 9]], [[0, 1, 4]], [[5, 6, 7]], [[0, 0, 1]], [[0xFFFFFFFF, 1, 2]]]).astype(np.uint32)  # range, NaN, collinear, repeated, range
    cov, s = cover(rows, verts, tris, max_distance=2 * RES, spacing=RES)
    good = cover(rows, *quad(), max_distance=2 * RES, spacing=RES)
    assert cov[:2].tobytes() == good[0].tobytes()
    assert cov[2:].tobytes() == bytes(5 * 32)
    assert s["n_tris_valid"] == 2 and s["n_tris_invalid"] == 5
    assert {k: v for k, v in s.items() if not k.startswith("n_tris")} == {k: v for k, v in good[1].items() if not k.startswith("n_tris")}


def test_a_huge_triangle_leaves_the_area_words_alone():
    verts, tris = quad()
    small = cover(NO_ROWS, verts, tris, spacing=RES)
    verts = np.vstack([verts, [[-5e4, -5e4, 0.05]], [[5e4, -5e4, 0.05]], [[0, 5e4, 0.05]]]).astype(np.float32)
    tris = np.vstack([tris, [[4, 5, 6]]]).astype(np.uint32)
    cov, s = cover(NO_ROWS, verts, tris, spacing=RES)
    assert cov["flags"][2] == V.VALID | V.CAPPED | V.HUGE and cov["n_samples"][2] == 4096 and cov["area"][2] == np.float32(5e9)
    assert cov["n_in_bbox"][2] < 4096 and cov["n_covered"][2] == 0
    assert s["n_tris_huge"] == 1 and s["n_tris_valid"] == 3 and s["n_samples"] == small[1]["n_samples"] + 4096
    for k in ("area_q40_lo", "area_q40_hi", "covered_q40_lo", "covered_q40_hi"):
        assert s[k] == small[1][k]
    alone = cover(NO_ROWS, verts, tris[2:], spacing=RES)[1]
    assert (alone["area_q40_lo"], alone["area_q40_hi"], alone["covered_q40_lo"], alone["covered_q40_hi"]) == (0, 0, 0, 0)


# ---- (f) the options check and the binding ---------------------------------------------------------------------------------

def test_check_cover_opts():
    H = hfpf
    assert H.check_cover_opts(H.cover_opts()) == 0
    assert H.check_cover_opts(None) == -2
    good = dict(radius=[1, 4], max_subdivision=[1, 64], min_count=[0.0, -1.0, 1e9], max_distance=[1.0, 1e-9], spacing=[1e-9, 1e9],
                min_normal_dot=[-2.0, 1.0, 0.0], flags=[0, H.COVER_ABS_NORMAL])
    bad = dict(struct_size=[0, 48, 64], flags=[2, 3, 1 << 31], reserved=[1], radius=[0, -1, 5], max_subdivision=[0, 65, 1 << 31],
               min_count=[float("nan")], max_distance=[0.0, -1.0, 1.0 + 2.0 ** -52, float("inf"), float("nan")],
               spacing=[0.0, -1.0, float("inf"), float("nan")], min_normal_dot=[-2.0 - 2.0 ** -51, 1.0 + 2.0 ** -52, float("inf"), float("nan")])
    for table, want in ((good, 0), (bad, -2)):
        for field, values in table.items():
            for val in values:
                o = H.cover_opts()
                setattr(o, field, val)
                assert H.check_cover_opts(o) == want, (field, val)


def test_binding_mirrors_the_header():
    txt = open(os.path.join(ROOT, "include", "hfpf.h")).read()
    for name in ("hfpf_check_cover_opts", "hfpf_cover_mesh", "hfpf_cover_mesh_device", "hfpf_free_coverage"):
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", txt, flags=re.S)), name
        assert name in hfpf.EXPORTS and hasattr(hfpf.lib(), name)
    for macro, val in (("HFPF_COV_VALID", hfpf.COV_VALID), ("HFPF_COV_CAPPED", hfpf.COV_CAPPED), ("HFPF_COV_HUGE", hfpf.COV_HUGE),
                       ("HFPF_COVER_ABS_NORMAL", hfpf.COVER_ABS_NORMAL)):
        assert int(re.search(r"#define\s+%s\s+(\d+)u" % macro, txt).group(1)) == val
    for struct, size in (("hfpf_cover_opts", C.sizeof(hfpf.CoverOpts)), ("hfpf_tri_coverage", hfpf.TRI_COVERAGE_DTYPE.itemsize),
                         ("hfpf_coverage_summary", C.sizeof(hfpf.CoverageSummary))):
        assert int(re.search(r"static_assert\(sizeof\(%s\) == (\d+)" % struct, txt).group(1)) == size
    assert hfpf.TRI_COVERAGE_DTYPE == V.TRI_COVERAGE_DTYPE
    assert tuple(k for k, _ in hfpf.CoverageSummary._fields_) == V.SUMMARY_KEYS
    d = hfpf.CoverageSummary(area_q40_lo=1 << 39, area_q40_hi=3, covered_q40_lo=0, covered_q40_hi=1).as_dict()
    assert d["area"] == 3 * 2.0 ** -8 + 0.5 and d["covered_area"] == 2.0 ** -8
