"""What the view-planning GPU tests share (imported by tests only): the reference meshes, the candidate poses, the device form's helper
and the byte-for-byte comparator.  No test and no fixture is defined here, and every assertion carries its message."""
import numpy as np

import cover_ref as V
import plan_ref as P
from gpu_support import RES, download, same_records, same_summary

SPHERE = ((0.05, 0.0, 0.45), 0.10)                           # the synthetic scene's sphere: centre, radius
BOX = ((-0.20, -0.08), (-0.10, 0.10), (0.40, 0.60))          # and its box
LOOK_AT = (0.0, 0.0, 0.47)
VIEW = dict(K=(200.0, 200.0, 80.0, 60.0), width=160, height=120)
SMALL_VIEW = dict(K=(40.0, 40.0, 16.0, 12.0), width=32, height=24)
# two-voxel samples; a one-pixel splat closes the gaps between them at 160 x 120; 1.5 voxels of depth tolerance
MAIN = dict(radius=2, max_distance=2 * RES, spacing=2 * RES, z_range=(0.05, 2.0), splat_radius=1, min_cos=0.2, tolerance=1.5 * RES, slope=0.0,
            max_views=8)


def sphere_and_box(stacks=24, slices=48):
    """The closed shapes of the synthetic scene as one mesh, wound outwards: a lat-long sphere whose polar triangles have zero area
    (2 * slices of them, invalid) and the box's 12 triangles."""
    (cx, cy, cz), r = SPHERE
    th = np.pi * np.arange(stacks + 1) / stacks
    ph = 2 * np.pi * np.arange(slices) / slices
    v = np.stack([cx + r * np.outer(np.sin(th), np.cos(ph)), cy + r * np.outer(np.cos(th), np.ones(slices)), cz + r * np.outer(np.sin(th), np.sin(ph))],
                 axis=-1)
    v[0], v[-1] = v[0, 0], v[-1, 0]  # one point per pole, repeated: the polar triangles are degenerate
    i, j = np.meshgrid(np.arange(stacks), np.arange(slices), indexing="ij")
    a, b, c, d = i * slices + j, i * slices + (j + 1) % slices, (i + 1) * slices + j, (i + 1) * slices + (j + 1) % slices
    st = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([b, d, c], -1).reshape(-1, 3)])
    sv = v.reshape(-1, 3)
    corners = np.array([[BOX[0][x], BOX[1][y], BOX[2][z]] for x in (0, 1) for y in (0, 1) for z in (0, 1)])  # index = 4x + 2y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]  # -x, +x, -y, +y, -z, +z seen from outside
    bt = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]) + len(sv)
    verts = np.concatenate([sv, corners]).astype(np.float32)
    tris = np.concatenate([st, bt]).astype(np.uint32)
    # outwards: flip whatever does not point away from its shape's centre
    P0, P1, P2 = (verts[tris[:, k]].astype(np.float64) for k in range(3))
    n = np.cross(P1 - P0, P2 - P0)
    centre = np.where((np.arange(len(tris)) < len(st))[:, None], np.array(SPHERE[0]), np.array([np.mean(b) for b in BOX]))
    flip = np.einsum("ij,ij->i", n, (P0 + P1 + P2) / 3 - centre) < 0
    tris[flip] = tris[flip][:, ::-1]
    return verts, tris


def look_at(eye, target=LOOK_AT, up=(0.0, -1.0, 0.0)):
    """The 3x4 camera -> fusion pose of a camera at `eye` whose +z looks at `target` (image y along -up)."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(-np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.hstack([np.stack([x, y, z], axis=1), eye.reshape(3, 1)])


def ring(n=12, radius=0.42, target=LOOK_AT, lift=0.0):
    """n poses on a circle around `target` in the plane y = target.y + lift, all looking at it; the first stands where the scanner did."""
    a = 2 * np.pi * np.arange(n) / n
    return np.stack([look_at((target[0] + radius * np.sin(t), target[1] + lift, target[2] - radius * np.cos(t)), target) for t in a])


def main_poses():
    """12 poses on the ring and, as view 12, view 3 again."""
    r = ring()
    return np.concatenate([r, r[3:4]])


def chips(n, z=0.15, seed=0xC41):
    """n small triangles of one sample each (with max_subdivision = 1) in the empty space in front of the scene, facing the scanner:
    nothing covers them, so a plan has exactly n targets."""
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(-0.1, 0.1, n), rng.uniform(-0.08, 0.08, n), rng.uniform(z, z + 0.05, n)], axis=1)
    tri = np.array([[-0.003, -0.003, 0.0], [0.0, 0.006, 0.0], [0.003, -0.003, 0.0]])
    return (c[:, None, :] + tri[None]).reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def soup(rows, pose, n=777, seed=0x50FA):
    """The mixed soup of the cover tests: triangles of 0.2 to 40 voxels near the rows, 78 of them invalid in three ways."""
    rng = np.random.default_rng(seed)
    Pt = np.stack([rows[k] for k in ("x", "y", "z")], axis=1).astype(np.float64)
    c = Pt[rng.integers(0, len(Pt), n)] + rng.uniform(-0.004, 0.004, (n, 3))
    c = (c - pose[:, 3]) @ pose[:, :3]
    edge = RES * np.exp(rng.uniform(np.log(0.2), np.log(40.0), (n, 1, 1)))
    verts = (c[:, None, :] + rng.uniform(-0.5, 0.5, (n, 3, 3)) * edge).reshape(-1, 3).astype(np.float32)
    tris = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    kinds = rng.permutation(n)[:78].reshape(3, 26)
    tris[kinds[0][:13], 2] = 3 * n + rng.integers(0, 1000, 13)
    tris[kinds[0][13:], 0] = 0xFFFFFFFF
    verts[tris[kinds[1], 1], 2] = np.nan
    tris[kinds[2], 1] = tris[kinds[2], 0]
    return verts, tris


def reference(g, rows, occ, verts, stride, tris, pose, poses, K, width, height, **kw):
    return P.plan(rows, occ, verts, stride, tris, pose, poses, tuple(g.cfg.bbox), g.dims[1], K, width, height, **kw)


def plan_device(g, H, d_verts, n_verts, stride, d_tris, n_tris, poses, pose, **kw):
    """hfpf_plan_views_device on a mesh in HBM, the records downloaded: (scores, records, summary)."""
    scores, ptr, s = g.plan_views(d_verts, d_tris, poses, pose, device=True, n_verts=n_verts, vertex_stride=stride, n_tris=n_tris, **kw)
    return scores, download(g, (ptr, n_tris, H.TRI_PLAN_DTYPE))[0], s


def same_plan(got, ref, what):
    """(scores, records, summary) of hfpf_plan_views, byte for byte."""
    same_records(got[0], ref[0], what, "views")
    same_records(got[1], ref[1], what, "triangles")
    same_summary(got[2], ref[2], P.SUMMARY_KEYS, what)
    same_summary(got[2]["coverage"], ref[2]["coverage"], V.SUMMARY_KEYS, what + ": coverage")


def plan_sums(scores, rec, s):
    """The summary of a plan is the sum of its records, and the gains add up to what is planned."""
    for k in ("n_targets", "n_reachable", "n_planned"):
        assert s[k] == sum(int(x) for x in rec[k]), k
    sel = scores["rank"] >= 0
    assert s["n_selected"] == int(sel.sum()) and sorted(scores["rank"][sel].tolist()) == list(range(s["n_selected"])), "ranks 0 .. n_selected - 1"
    assert s["planned_q40"] == sum(int(x) for x in scores["gain_q40"]) and s["n_planned"] == sum(int(x) for x in scores["gain_samples"]), "the gains"
    assert not scores["gain_q40"][~sel].any() and not scores["gain_samples"][~sel].any(), "an unselected view has no gain"
    order = np.argsort(scores["rank"][sel])
    gains = [int(x) for x in scores["gain_q40"][sel][order]]
    assert gains == sorted(gains, reverse=True), "marginal gains never grow"
    assert s["planned_q40"] <= s["reachable_q40"] <= s["target_q40"] and s["n_views"] == len(scores), "planned, reachable, targets"
    assert (scores["n_visible"] <= scores["n_facing"]).all() and (scores["n_facing"] <= scores["n_in_view"]).all(), "visible, facing, in view"
