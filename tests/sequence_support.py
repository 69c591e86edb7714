"""What the sequence tests share (imported by tests only): a model of the handle built from the oracle and tests/hide_ref.py, the table
of read-outs with their restatements, the fixed inputs those take, the engine-side driver of a script, the states of the matrix and the
script generator.  No test and no fixture is defined here, and every assertion carries its message.

include/hfpf.h says of every read-out that it sees "exactly the rows hfpf_extract would return at that point of the call sequence".
The tests of one read-out call it on a settled handle; here a read-out is the FIRST call to meet whatever the sequence left behind --
host frames waiting for their launch, a batch whose update kernel still runs, a clean pass that did not wait, a restore, another
read-out's row set.  The order of a check is therefore: the read-out, then hfpf_extract and hfpf_get_occupied, which are compared with
the model (scenes.compare_rows, as the random-schedule tests do), then the restatement on the ENGINE's rows and occupied list, byte for
byte, as the tests of that read-out compare it.  No tolerance is introduced here."""
import collections
import time

import numpy as np

import align_ref as A
import components_ref as CR
import consistency_ref as CS
import cover_ref as V
import deviation_ref as D
import gpu_support as G
import hide_ref as HR
import mesh_ref as M
import plan_ref as P
import plan_support as PS
import query_ref as Q
import raycast_ref as RC
import render_ref as R
import scenes
import track_ref as TR
from gpu_support import IDENT

W, H, N_FRAMES = 160, 120, 10    # the smallest frames at which the scene still has rows after one pass; they tile by 16 in width only
VW, VH = 80, 60                  # every view of a read-out ...
RW, RH = 40, 30                  # ... but the rays': the march of raycast_ref.py is the slowest of the restatements
RES, BBOX = G.RES, G.BBOX
MIN_COUNT = 2.0                  # the count gate of every checked read-out; the read-out that runs first in state 7 takes 0 (more rows)
CONFIG_KEYS = ("K", "gate", "pcl_shifted_cov")
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


# ---- the inputs: one scene, one mesh, one looking frame -- none depends on the state of a handle --------------------------------------

def icosphere(centre, radius, level=2):
    """(vertices (n, 3) f32, triangles (m, 3) u32) of an icosahedron subdivided `level` times, wound outwards: 320 triangles at level 2."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, out = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    verts = (np.asarray(centre, np.float64) + radius * np.asarray(v)).astype(np.float32)
    tris = np.asarray(f, np.uint32)
    n = np.cross(verts[tris[:, 1]] - verts[tris[:, 0]], verts[tris[:, 2]] - verts[tris[:, 0]])
    assert (np.einsum("ij,ij->i", n, verts[tris[:, 0]] - np.asarray(centre, np.float32)) > 0).all(), "the icosphere is wound outwards"
    return verts, tris


class Inputs:
    """The scene (frames as depth + colour images and as the equivalent packed clouds) and what the read-outs are asked with."""

    def __init__(self):
        sc = scenes.DepthScene(N_FRAMES, W, H, clean_every=0)
        self.sc, self.poses, self.K = sc, sc.poses, tuple(float(k) for k in sc.K)
        self.clouds = [np.ascontiguousarray(sc.cloud(f)) for f in range(N_FRAMES)]
        self.depths = [np.ascontiguousarray(sc.frames[f][0]) for f in range(N_FRAMES)]
        self.colors = [np.ascontiguousarray(sc.frames[f][1]) for f in range(N_FRAMES)]
        # the mesh: the icosphere around the sensor's sphere, one triangle with an index out of range, one with a NaN vertex
        v, t = icosphere(PS.SPHERE[0], PS.SPHERE[1])
        self.verts = np.ascontiguousarray(np.vstack([v, [[np.nan, 0.0, 0.4]]]).astype(np.float32))
        self.tris = np.ascontiguousarray(np.vstack([t, [[0, 1, len(v) + 7]], [[2, 3, len(v)]]]).astype(np.uint32))
        # the looking frame: every second pixel of frame 8, with the intrinsics of that image
        self.f_look = 8
        self.depth_q = np.ascontiguousarray(self.depths[self.f_look][::2, ::2])
        self.K_q = tuple(k / 2.0 for k in self.K)
        self.K_r = tuple(k / 4.0 for k in self.K)   # of the 40 x 30 view of the rays
        self.pose_q = self.poses[self.f_look]
        self.points = np.ascontiguousarray(Q.depth_points(self.depth_q, self.K_q)[::9])       # 534 query points, camera frame
        self.guess = G.perturb(self.pose_q, 1.0, (0.004, -0.003, 0.004))
        self.start = A.rigid(0.3, (0.5, 1.0, -0.4), tuple(np.array([0.6, -0.64, 0.48]) * 1.5 * RES), A.centre(BBOX))
        self.ring = PS.ring(6)
        self.plan_view = dict(K=(100.0, 100.0, 40.0, 30.0), width=VW, height=VH)
        # depth consistency: two frames of the stream and frame 0 again with its left half 50 mm farther (the rows in front are seen THROUGH)
        far = self.depths[0].copy()
        left = far[:, :W // 2]
        left[left != 0] += 50
        self.cons_frames = np.ascontiguousarray(np.stack([self.depths[0], self.depths[6], far]))
        self.cons_poses = np.stack([self.poses[0], self.poses[6], self.poses[0]])
        self.dims = self.res = None   # of the grid: set by the first Model
        for a in (self.verts, self.tris, self.depth_q, self.points, self.cons_frames, self.cons_poses, *self.clouds, *self.depths, *self.colors):
            a.setflags(write=False)


_inputs = []


def inputs():
    """The Inputs, rendered once a process (needs hfpf_synth built: ask for the synth_mod fixture)."""
    if not _inputs:
        _inputs.append(Inputs())
    return _inputs[0]


# ---- the model ----------------------------------------------------------------------------------------------------------------------

class Model:
    """What a handle holds, from what the project already has: an oracle grid with the colour extension, the hidden set H as sorted
    voxel keys (tests/hide_ref.py), and the log of the mutating operations so far.  A restore to an earlier snapshot is "hfpf_clear
    followed by putting that state in place": the oracle is rebuilt from the log's prefix up to the mark, H is what it was there."""

    def __init__(self, oracle_mod, x, **cfg):
        self.O, self.x, self.cfg = oracle_mod, x, cfg
        self.og = self._fresh()
        self.log, self.H, self.marks = [], np.zeros(0, np.int64), []
        self.dims, self.res = self.og.dims
        if x.dims is None:
            x.dims, x.res = self.dims, self.res
        assert (x.dims, x.res) == (self.dims, self.res), "one grid geometry for every model"
        self._rows = None

    def _fresh(self):
        return self.O.OracleGrid(resolution=RES, bbox=BBOX, fuse_color=True, **self.cfg)

    def close(self):
        self.og.close()

    def _do(self, op):
        if op[0] == "integrate":
            self.og.capture(self.x.clouds[op[1]], self.x.poses[op[1]], off_rgb=12)
        elif op[0] == "clean":
            self.og.clean()
        elif op[0] == "clear":
            self.og.clear()
        self._rows = None

    def integrate(self, f):
        self.log.append(("integrate", int(f)))
        self._do(self.log[-1])

    def clean(self):
        self.log.append(("clean",))
        self._do(self.log[-1])

    def clear(self):
        self.log.append(("clear",))
        self._do(self.log[-1])
        self.H = np.zeros(0, np.int64)

    def full_rows(self):
        """The oracle's rows with nothing hidden: F of tests/hide_ref.py."""
        if self._rows is None:
            self._rows = self.og.extract()
            self._rows.setflags(write=False)
        return self._rows

    def hide_voxels(self, voxels, op="hide"):
        Hv, counts = HR.hide_voxels(self.full_rows(), HR.voxels_of(self.H), self.dims, voxels, op)
        self.H = HR.keys(Hv)
        self.log.append(("hide_voxels", op, len(voxels)))
        return counts

    def hide_box(self, lo, hi, op="hide"):
        Hv, counts = HR.hide_box(self.full_rows(), HR.voxels_of(self.H), self.dims, lo, hi, op)
        self.H = HR.keys(Hv)
        self.log.append(("hide_box", op, tuple(int(v) for v in lo), tuple(int(v) for v in hi)))
        return counts

    def show_all(self):
        self.H = np.zeros(0, np.int64)
        self.log.append(("show_all",))

    def mark(self):
        self.marks.append((list(self.log), self.H.copy()))
        return len(self.marks) - 1

    def rollback(self, tag):
        log, H_then = self.marks[tag]
        self.og.close()
        self.og = self._fresh()
        self._rows = None
        for op in log:
            self._do(op)
        self.log, self.H = list(log), H_then.copy()

    def rows(self):
        return HR.visible(self.full_rows(), HR.voxels_of(self.H))

    def occupied(self):
        return self.og.occupied()

    def hidden(self):
        return HR.voxels_of(self.H)

    def dirty(self):
        return self.og.is_dirty()

    def frozen(self):
        """The four answers as they are now, to share among the cases of one state."""
        return Frozen(self.rows().copy(), self.occupied().copy(), self.hidden().copy(), self.dirty())


class Frozen(collections.namedtuple("Frozen", "rows_ occupied_ hidden_ dirty_")):
    def rows(self):
        return self.rows_

    def occupied(self):
        return self.occupied_

    def hidden(self):
        return self.hidden_

    def dirty(self):
        return self.dirty_


# ---- the inputs in HBM of one handle, uploaded BEFORE the state is built: no upload stands between the state and the read-out ----------

class DeviceInputs:
    def __init__(self, g, hfpf_mod, x):
        self.g, self.p = g, {}
        self.cloud_stride = W * H * 16
        self.depth_stride, self.color_stride = (W * H * 2 + 255) & ~255, (W * H * 3 + 255) & ~255
        self.desc = hfpf_mod.depth_desc(W, H, hfpf_mod.DEPTH_U16, W * 2, x.K, hfpf_mod.COLOR_RGB8, W * 3)
        self.desc_q = hfpf_mod.depth_desc(VW, VH, hfpf_mod.DEPTH_U16, VW * 2, x.K_q)
        self.desc_cons = hfpf_mod.depth_desc(W, H, hfpf_mod.DEPTH_U16, W * 2, x.K)
        try:
            for name, nbytes in (("clouds", self.cloud_stride * N_FRAMES), ("depths", self.depth_stride * N_FRAMES), ("colors", self.color_stride * N_FRAMES)):
                self.p[name] = g.device_alloc(nbytes)
            for f in range(N_FRAMES):
                g.device_upload(self.p["clouds"] + f * self.cloud_stride, x.clouds[f])
                g.device_upload(self.p["depths"] + f * self.depth_stride, x.depths[f])
                g.device_upload(self.p["colors"] + f * self.color_stride, x.colors[f])
            for name, a in (("verts", x.verts), ("tris", x.tris), ("points", x.points), ("depth_q", x.depth_q), ("cons", x.cons_frames)):
                self.p[name] = g.device_alloc(max(a.nbytes, 16))
                g.device_upload(self.p[name], a)
            # where the device forms leave their results
            self.p["q_hits"] = g.device_alloc(len(x.points) * hfpf_mod.QUERY_HIT_DTYPE.itemsize)
            self.p["q_rows"] = g.device_alloc(len(x.points) * hfpf_mod.ROW_DTYPE.itemsize)
            self.p["ray_hits"] = g.device_alloc(RW * RH * hfpf_mod.RAY_HIT_DTYPE.itemsize)
            for name, dt, ch in hfpf_mod.RENDER_PLANES:
                self.p["plane_" + name] = g.device_alloc(VW * VH * ch * np.dtype(dt).itemsize)
        except BaseException:
            self.free()
            raise

    def free(self):
        for ptr in self.p.values():
            self.g.device_free(ptr)
        self.p = {}


# ---- the read-outs ------------------------------------------------------------------------------------------------------------------
# call(e, x, mc, device) -> what the engine answers (e: Engine; device: the _device form, where there is one);
# ref(rows, occ, x, mc, m) -> the restatement's answer on extracted rows and an occupied list (m: the model, for H and dirtiness);
# same(got, ref, what) asserts; figure(ref) -> the non-triviality figure; floor: what a non-trivial figure exceeds (None: no floor).

ReadOut = collections.namedtuple("ReadOut", "name call ref same figure floor unit")

Z_RANGE = (0.05, 3.0)
T_RANGE = (0.30, 0.62)   # the default z-clip and a little more: where the scene's surfaces lie in front of a camera of the stream


def _gate(rows, mc):
    return rows[rows["count"] >= mc]


def _render_kw(mc):
    return dict(z_range=Z_RANGE, min_count=mc, splat_radius=2, max_splat_radius=4, cull_backfaces=True, world_normals=True)


def _render_call(e, x, mc, device):
    if not device:
        return e.g.render(x.poses[3], x.K_q, VW, VH, **_render_kw(mc))
    planes = {name: e.dev.p["plane_" + name] for name, _, _ in e.H.RENDER_PLANES}
    e.g.render_device(x.poses[3][None], x.K_q, VW, VH, planes, **_render_kw(mc))
    return {name: e.g.device_download(planes[name], VW * VH * ch * np.dtype(dt).itemsize).view(dt).reshape((VH, VW, ch) if ch > 1 else (VH, VW))
            for name, dt, ch in e.H.RENDER_PLANES}


def _render_ref(rows, occ, x, mc, m):
    return R.render(rows, x.poses[3], x.K_q, VW, VH, x.res, Z_RANGE, mc, 2, 4, R.CULL_BACKFACES | R.WORLD_NORMALS)


def _query_call(e, x, mc, device):
    if not device:
        return e.g.query(x.points, x.pose_q, radius=2, min_count=mc)
    n = len(x.points)
    e.g.query_device(e.dev.p["points"], n, x.pose_q, dev_hits=e.dev.p["q_hits"], dev_rows=e.dev.p["q_rows"], radius=2, min_count=mc)
    return (e.g.device_download(e.dev.p["q_hits"], n * e.H.QUERY_HIT_DTYPE.itemsize).view(e.H.QUERY_HIT_DTYPE),
            e.g.device_download(e.dev.p["q_rows"], n * e.H.ROW_DTYPE.itemsize).view(e.H.ROW_DTYPE))


def _query_depth_kw(x, mc):
    return dict(radius=1, min_count=mc, max_distance=3 * x.res, zclip=True)


TRACK_KW = dict(max_iterations=6, max_distance=0.03, damping=1e-6, eps_rotation=1e-6, eps_translation=1e-6)
TRACK_VIEW = dict(z_range=Z_RANGE, splat_radius=-1, max_splat_radius=4)


def _track_call(e, x, mc, device):
    kw = dict(TRACK_KW, **TRACK_VIEW, min_count=mc, cull_backfaces=True, stride=1)
    if device:
        return e.g.track_depth_device(e.dev.desc_q, e.dev.p["depth_q"], x.guess, **kw)
    return e.g.track_depth(x.depth_q, x.guess, x.K_q, **kw)


def _track_ref(rows, occ, x, mc, m):
    view = dict(TRACK_VIEW, K=x.K_q, width=VW, height=VH, min_count=mc, flags=R.CULL_BACKFACES)
    return TR.track(rows, TR.depth_points(x.depth_q, x.K_q, 1), x.guess, RES, view, G.Z_CLIP, min_inliers=6, **TRACK_KW)   # (RES: as gpu_support.track_reference)


def _ray_kw(mc):
    return dict(radius=2, min_count=mc, step=1.0, t_range=T_RANGE)


def _raycast_call(e, x, mc, device):
    if not device:
        return e.g.raycast_view(x.poses[0], x.K_r, RW, RH, **_ray_kw(mc))
    e.g.raycast_views_device(x.poses[0][None], x.K_r, RW, RH, dev_hits=e.dev.p["ray_hits"], **_ray_kw(mc))
    return e.g.device_download(e.dev.p["ray_hits"], RW * RH * e.H.RAY_HIT_DTYPE.itemsize).view(e.H.RAY_HIT_DTYPE).reshape(RH, RW)


def _comp_kw(mc):
    return dict(reach=2, min_normal_dot=0.9, min_rows=20, min_count=mc)


def _mesh_of(e, x, device):
    """The mesh arguments of a call on the fixed mesh: host arrays, or the copies in HBM."""
    if device:
        return (e.dev.p["verts"], e.dev.p["tris"]), dict(device=True, n_verts=len(x.verts), vertex_stride=12, n_tris=len(x.tris))
    return (x.verts, x.tris), {}


def _compare_call(e, x, mc, device):
    if device:
        return G.compare_device(e.g, e.H, e.dev.p["verts"], len(x.verts), 12, e.dev.p["tris"], len(x.tris), IDENT, min_count=mc, max_distance=3 * x.res)
    return e.g.compare_mesh(x.verts, x.tris, IDENT, min_count=mc, max_distance=3 * x.res)


def _cover_kw(x, mc):
    return dict(radius=2, min_count=mc, max_distance=2 * x.res, spacing=2 * x.res)


def _cover_call(e, x, mc, device):
    if device:
        return G.cover_device(e.g, e.H, e.dev.p["verts"], len(x.verts), 12, e.dev.p["tris"], len(x.tris), IDENT, **_cover_kw(x, mc))
    return e.g.cover_mesh(x.verts, x.tris, IDENT, **_cover_kw(x, mc))


def _align_kw(x, mc):
    return dict(max_iterations=5, stride=4, eps_rotation=1e-5, eps_translation=1e-5, min_count=mc, max_distance=8 * x.res)


def _align_call(e, x, mc, device):
    mesh, kw = _mesh_of(e, x, device)
    return e.g.align_mesh(*mesh, x.start, **kw, **_align_kw(x, mc))


def _plan_kw(x, mc):
    return dict(radius=2, min_count=mc, max_distance=2 * x.res, spacing=4 * x.res, z_range=(0.05, 2.0), splat_radius=1, min_cos=0.2, tolerance=1.5 * x.res,
                slope=0.0, max_views=4, model_occludes=True, view_min_count=mc)


def _plan_call(e, x, mc, device):
    if device:
        return PS.plan_device(e.g, e.H, e.dev.p["verts"], len(x.verts), 12, e.dev.p["tris"], len(x.tris), x.ring, IDENT, **x.plan_view, **_plan_kw(x, mc))
    return e.g.plan_views(x.verts, x.tris, x.ring, IDENT, **x.plan_view, **_plan_kw(x, mc))


def _cons_kw(mc):
    return dict(window=1, tolerance=0.004, min_cos=0.3, min_through=1, through_ratio=0.0, min_count=mc)


def _cons_call(e, x, mc, device):
    if not device:
        return e.g.depth_consistency(x.cons_frames, x.cons_poses, x.K, **_cons_kw(mc))
    r, c, nr, s = e.g.depth_consistency_device(e.dev.desc_cons, e.dev.p["cons"], x.cons_frames.strides[0], len(x.cons_frames), x.cons_poses, **_cons_kw(mc))
    rows, cons = G.download(e.g, (r, nr, e.H.ROW_DTYPE), (c, nr, e.H.ROW_CONSISTENCY_DTYPE))
    return rows, cons, s


def _same_cons(got, ref, what):
    G.same_records(got[:2], ref[:2], what, ("rows", "records"))
    G.same_summary(got[2], ref[2], CS.SUMMARY_KEYS, what)


def _same_rows(got, ref, what):
    G.same_records(got, ref, what, "rows")


def _same_voxels(got, ref, what):
    assert got.dtype == np.int32 and got.shape == ref.shape and got.tobytes() == np.ascontiguousarray(ref, np.int32).tobytes(), \
        "%s: %d voxels vs %d" % (what, len(got), len(ref))


def _same_flag(got, ref, what):
    assert got == ref, "%s: %r vs %r" % (what, got, ref)


READ_OUTS = (
    ReadOut("extract_filtered", lambda e, x, mc, device: e.g.extract_filtered(min_count=mc), lambda rows, occ, x, mc, m: _gate(rows, mc), _same_rows,
            len, 0, "rows"),
    ReadOut("render", _render_call, _render_ref, G.same_planes, lambda ref: int((~np.isnan(ref["depth"])).sum()), 100, "pixels drawn"),
    ReadOut("query", _query_call, lambda rows, occ, x, mc, m: Q.query(rows, occ, x.points, x.pose_q, BBOX, x.res, radius=2, min_count=mc), G.same_query,
            lambda ref: int((ref[0]["flags"] & Q.FOUND != 0).sum()), 100, "points FOUND"),
    ReadOut("query_depth", lambda e, x, mc, device: e.g.query_depth(x.depth_q, x.pose_q, x.K_q, **_query_depth_kw(x, mc)),
            lambda rows, occ, x, mc, m: Q.query(rows, occ, Q.depth_points(x.depth_q, x.K_q), x.pose_q, BBOX, x.res, G.Z_CLIP, **_query_depth_kw(x, mc)),
            G.same_query, lambda ref: int((ref[0]["flags"] & Q.FOUND != 0).sum()), 100, "pixels FOUND"),
    ReadOut("track_depth", _track_call, _track_ref, G.same_track, lambda ref: int(ref["inliers"]), 100, "inliers"),
    ReadOut("extract_mesh", lambda e, x, mc, device: G.mesh_device(e.g, radius=1, min_count=mc) if device else e.g.extract_mesh(radius=1, min_count=mc),
            lambda rows, occ, x, mc, m: M.mesh(rows, occ, BBOX, x.res, x.dims, radius=1, min_count=mc)[:2], G.same_mesh, lambda ref: len(ref[1]), 100,
            "triangles"),
    ReadOut("raycast_view", _raycast_call, lambda rows, occ, x, mc, m: RC.raycast_view(rows, occ, x.poses[0], x.K_r, RW, RH, BBOX, x.res, **_ray_kw(mc)),
            G.same_rays, lambda ref: int((ref["flags"] & RC.HIT != 0).sum()), 100, "hits"),
    ReadOut("extract_components", lambda e, x, mc, device: G.components_device(e.g, e.H, **_comp_kw(mc)) if device else e.g.extract_components(**_comp_kw(mc)),
            lambda rows, occ, x, mc, m: CR.components(rows, **_comp_kw(mc)), G.same_components, lambda ref: len(ref[2]), 0, "components"),
    ReadOut("compare_mesh", _compare_call, lambda rows, occ, x, mc, m: D.compare(rows, x.verts, 12, x.tris, IDENT, mc, 3 * x.res), G.same_deviation,
            lambda ref: int(ref[1]["n_found"]), 0, "rows found"),
    ReadOut("cover_mesh", _cover_call, lambda rows, occ, x, mc, m: V.cover(rows, occ, x.verts, 12, x.tris, IDENT, BBOX, x.res, **_cover_kw(x, mc)),
            G.same_coverage, lambda ref: int(ref[1]["n_covered"]), 0, "samples covered"),
    ReadOut("align_mesh", _align_call, lambda rows, occ, x, mc, m: A.align(rows, x.verts, 12, x.tris, x.start, BBOX, **_align_kw(x, mc)), G.same_align,
            lambda ref: int(ref["inliers"]), 0, "inliers"),
    ReadOut("plan_views", _plan_call,
            lambda rows, occ, x, mc, m: P.plan(rows, occ, x.verts, 12, x.tris, IDENT, x.ring, BBOX, x.res, x.plan_view["K"], VW, VH, **_plan_kw(x, mc)),
            PS.same_plan, lambda ref: int(ref[2]["coverage"]["n_covered"]), 0, "samples covered"),
    ReadOut("depth_consistency", _cons_call, lambda rows, occ, x, mc, m: CS.consistency(rows, x.cons_frames, x.cons_poses, x.K, **_cons_kw(mc)), _same_cons,
            lambda ref: len(ref[1]), 0, "records"),
    # the three calls that answer from the handle's state alone, against the model itself
    ReadOut("get_hidden", lambda e, x, mc, device: e.g.hidden(), lambda rows, occ, x, mc, m: m.hidden(), _same_voxels, len, None, "hidden voxels"),
    ReadOut("get_occupied", lambda e, x, mc, device: e.g.occupied(), lambda rows, occ, x, mc, m: m.occupied(), _same_voxels, len, None, "occupied cells"),
    ReadOut("is_dirty", lambda e, x, mc, device: e.g.state_changed, lambda rows, occ, x, mc, m: m.dirty(), _same_flag, int, None, "dirty"),
)
NAMES = tuple(r.name for r in READ_OUTS)
RESTATED = tuple(r for r in READ_OUTS if r.floor is not None)   # the read-outs of the model itself, without the three calls that answer from the state


def nontrivial(ro, figure):
    return ro.floor is not None and figure > ro.floor


def check(ro, e, m, index, what, mc=MIN_COUNT):
    """Read-out `ro` on engine e, as the first call to meet what the sequence left; then extract and the occupied list against model m;
    then the restatement on the engine's own rows.  Check `index` takes the device form when it is odd.  Returns (figure, rows)."""
    x = e.x
    got = ro.call(e, x, mc, bool(index & 1))
    rows, occ = e.g.extract(), e.g.occupied()
    scenes.compare_rows(m.rows(), rows)
    _same_voxels(occ, m.occupied(), "%s: hfpf_get_occupied against the model" % what)
    _same_voxels(e.g.hidden(), m.hidden(), "%s: hfpf_get_hidden against the model" % what)
    _same_flag(e.g.state_changed, m.dirty(), "%s: hfpf_is_dirty against the model" % what)
    ref = ro.ref(rows, occ, x, mc, m)
    ro.same(got, ref, "%s: %s, %s form" % (what, ro.name, "device" if index & 1 else "host"))
    return ro.figure(ref), rows


def model_figure(ro, m, x, mc=MIN_COUNT):
    """The figure of read-out `ro` on the model's own rows (no engine): what the script-coverage conditions count."""
    return ro.figure(ro.ref(m.rows(), m.occupied(), x, mc, m))


# ---- the engine side of an operation ---------------------------------------------------------------------------------------------------

HOST_KINDS, BATCH_KINDS = ("pageable", "pinned", "depth"), ("device_cloud", "device_depth")


class Engine:
    """One handle with the inputs in its HBM; a handoff replaces the handle (snapshot, close, create with the other update form, restore)."""

    def __init__(self, hfpf_mod, x, binned=True, frame_width=0, **cfg):
        self.H, self.x, self.cfg, self.binned, self.fw, self.flip = hfpf_mod, x, cfg, binned, frame_width, False
        self.g = self.dev = None
        self.blobs = []
        self._open()

    def _open(self):
        self.g = self.H.OccupancyGrid(resolution=RES, bbox=BBOX, fuse_color=True, binned_update=self.binned != self.flip, frame_width=self.fw, **self.cfg,
                                      **G.SMALL_CAPS)
        self.pinned = []
        try:
            self.dev = DeviceInputs(self.g, self.H, self.x)
        except BaseException:
            self.g.close()
            self.g = None
            raise

    def close(self, failed=False):
        """Syncs (pinned frames must stay untouched until then), frees the buffers and destroys the handle.  failed: the caller is already
        leaving with an exception, which an error of the clean-up (a handle that a device error has poisoned) must not replace."""
        if self.g is None:
            return
        try:
            self.g.sync()
            for b in self.pinned:
                self.g.host_free(b)
            self.dev.free()
        except self.H.HfpfError:
            if not failed:
                raise
        finally:
            self.g.close()
            self.g = None

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.close(failed=exc_type is not None)

    def integrate(self, kind, first, n=1):
        g, x, d = self.g, self.x, self.dev
        poses = np.stack([np.asarray(x.poses[f], np.float64).reshape(12) for f in range(first, first + n)])
        if kind == "pageable":
            g.integrate(x.clouds[first], x.poses[first])
        elif kind == "pinned":
            buf = g.host_alloc(x.clouds[first].nbytes)
            buf[...] = x.clouds[first].view(np.uint8).reshape(-1)
            self.pinned.append(buf)
            g.integrate_pinned(buf, x.poses[first])
        elif kind == "depth":
            g.integrate_depth(x.depths[first], x.poses[first], x.K, color=x.colors[first])
        elif kind == "device_cloud":
            g.integrate_device(d.p["clouds"] + first * d.cloud_stride, n, d.cloud_stride, W * H, poses)
        elif kind == "device_depth":
            g.integrate_depth_device(d.desc, d.p["depths"] + first * d.depth_stride, d.depth_stride, n, poses, dev_color=d.p["colors"] + first * d.color_stride,
                                     color_frame_stride=d.color_stride)
        else:
            raise AssertionError(kind)

    def mark(self):
        self.blobs.append(self.g.snapshot().tobytes())

    def handoff(self):
        blob, dirty = self.g.snapshot().tobytes(), self.g.state_changed
        self.close()
        self.flip = not self.flip
        self._open()
        self.g.restore(blob)
        assert self.g.state_changed == dirty, "a restored handle is as dirty as its source"


def as_rows(v):
    """Voxels as 64-byte row records: only ix, iy, iz are read by a list call, the rest is noise."""
    r = np.frombuffer(np.random.default_rng(5).bytes(64 * len(v)), CR.ROW_DTYPE).copy()
    r["ix"], r["iy"], r["iz"] = v[:, 0], v[:, 1], v[:, 2]
    return r


def hide_voxels_of(m, which):
    """The list a scripted hide call names, from the model's rows as they are (all of them: hidden ones can be shown again), with two
    entries that match nothing."""
    v = HR.row_voxels(m.full_rows()).astype(np.int32)
    pick = {"hashed": HR.hashed(m.full_rows()) if len(v) else np.zeros(0, bool), "third": np.arange(len(v)) % 3 == 0, "most": np.arange(len(v)) % 4 != 0}[which]
    return np.ascontiguousarray(np.vstack([v[pick], [[-1, 5, 5], [INT_MAX, 0, 0]]]).astype(np.int32))


def hide_box_of(m, which):
    """(lo, hi) of a scripted box: the middle third of the rows' x range, or its first three quarters."""
    rows = m.full_rows()
    if len(rows) == 0:
        return np.array([10, INT_MIN, INT_MIN], np.int32), np.array([200, INT_MAX, INT_MAX], np.int32)
    if which == "middle":
        return HR.middle_third(rows)
    x0, x1 = int(rows["ix"].min()), int(rows["ix"].max())
    return np.array([x0, INT_MIN, INT_MIN], np.int32), np.array([x0 + 3 * (x1 - x0 + 1) // 4, INT_MAX, INT_MAX], np.int32)


def resolve(op, m):
    """Applies one mutating operation of a script or a state to the model and returns it as an engine takes it: a hide call with the
    voxels or the box it names at this point and the counts the model expects."""
    kind = op[0]
    if kind == "integrate":
        for f in range(op[2], op[2] + op[3]):
            m.integrate(f)
    elif kind == "clean":
        m.clean()
    elif kind == "clear":
        m.clear()
    elif kind == "hide_list":
        _, hop, stride, which = op
        v = hide_voxels_of(m, which)
        return ("hide_list", hop, stride, v, m.hide_voxels(v, hop))
    elif kind == "hide_box":
        _, hop, which = op
        lo, hi = hide_box_of(m, which)
        return ("hide_box", hop, lo, hi, m.hide_box(lo, hi, hop))
    elif kind == "show_all":
        m.show_all()
    elif kind == "mark":
        return ("mark", m.mark())
    elif kind == "restore":
        m.rollback(op[1])
    else:
        raise AssertionError(op)
    return op


def engine_apply(op, e):
    """One resolved operation on an engine; the counts of a hide call are the model's."""
    kind = op[0]
    if kind == "integrate":
        e.integrate(op[1], op[2], op[3])
    elif kind == "clean":
        e.g.clean()
    elif kind == "clear":
        e.g.clear()
    elif kind == "hide_list":
        _, hop, stride, v, want = op
        got = e.g.hide_voxels(as_rows(v) if stride == 64 else v, hop)
        assert got == want, "hide_voxels %s, stride %d, %d entries: counts %r, the model's %r" % (hop, stride, len(v), got, want)
    elif kind == "hide_box":
        _, hop, lo, hi, want = op
        got = e.g.hide_box(lo, hi, hop)
        assert got == want, "hide_box %s %r .. %r: counts %r, the model's %r" % (hop, tuple(lo), tuple(hi), got, want)
    elif kind == "show_all":
        e.g.show_all()
    elif kind == "mark":
        e.mark()
        assert len(e.blobs) == op[1] + 1, "one blob per mark"
    elif kind == "restore":
        e.g.restore(e.blobs[op[1]])
    else:
        raise AssertionError(op)


def apply(op, m, engines=()):
    """One mutating operation on the model and on every engine."""
    resolved = resolve(op, m)
    for e in engines:
        engine_apply(resolved, e)


# ---- the states of the matrix ------------------------------------------------------------------------------------------------------------

def _batch(index, first, n):
    return ("integrate", BATCH_KINDS[index % 2], first, n)


def state_ops(state, index):
    """The mutating operations that build a state; `index` (the read-out's) alternates the forms an integrate call takes."""
    host = "pageable" if index % 2 == 0 else "depth"
    cleaned = [_batch(index, 0, 4), ("clean",)]
    return {
        "waiting_host_frames": cleaned + [("integrate", host, f, 1) for f in (4, 5, 6)],
        "device_batch_in_flight": cleaned + [_batch(index + 1, 4, 5)],
        "nowait_clean": cleaned + [("integrate", host, 4, 1), ("clean",)],
        "overlapped_clean": cleaned + [_batch(index + 1, 4, 4), ("clean",)],
        "after_clear": [_batch(index, 0, 6), ("clean",)] + [("integrate", host, f, 1) for f in (6, 7, 8)] + [("clean",), ("clear",), ("integrate", host, 0, 1),
                                                                                                           ("integrate", host, 1, 1), ("clean",)],
        "after_rollback": cleaned + [("mark",), _batch(index + 1, 4, 5), ("clean",), ("hide_box", "hide", "middle"), ("restore", 0)],
        "after_previous_readout": [_batch(index, 0, 6), ("clean",), ("integrate", host, 6, 1), ("clean",)],
        # the other direction of after_rollback: the snapshot holds a hidden set, what is hidden at the restore is another one
        "rollback_to_hidden": cleaned + [("hide_list", "hide", 64 if index % 2 else 12, "third"), ("mark",), _batch(index + 1, 4, 5), ("clean",), ("show_all",),
                                         ("hide_box", "hide", "middle"), ("restore", 0)],
    }[state]


STATES = ("waiting_host_frames", "device_batch_in_flight", "nowait_clean", "overlapped_clean", "after_clear", "after_rollback", "after_previous_readout",
          "rollback_to_hidden")


def model_key(ops):
    """Two lists of operations with the same key give the same model: the form of an integrate call is the engine's affair."""
    return tuple(("integrate", op[2], op[3]) if op[0] == "integrate" else (op[:2] + op[3:] if op[0] == "hide_list" else op) for op in ops)


# ---- the scripts -----------------------------------------------------------------------------------------------------------------------

SEED_BASE = 7000
N_CHECKS = 6          # per script: 72 checks over the 12 default seeds, 4 or 5 of each read-out
PREDECESSORS = ("integrate", "clean", "batch_clean", "clear", "restore", "hide", "check")


def config_of(seed):
    """(oracle and engine keywords, binned_update, frame_width) of a seed, varied as in the random-schedule tests."""
    rng = np.random.default_rng(SEED_BASE + 500 + seed)
    cfg = {}
    if rng.random() < 0.3:
        cfg["K"] = int(rng.integers(1, 5))
    if rng.random() < 0.3:
        cfg["gate"] = int(rng.integers(12, 30))
    if rng.random() < 0.2:
        cfg["pcl_shifted_cov"] = True
    return cfg, bool(seed % 2), (W if (seed // 2) % 2 else 0)


def script(seed):
    """The operations of one seed: an opening batch and pass, then N_CHECKS segments of a predecessor and a check.  Read-out k of check
    i is (seed * N_CHECKS + i) mod the table's length, so that the seeds share the table out evenly; everything else is drawn."""
    rng = np.random.default_rng(SEED_BASE + seed)
    ops, st = [], dict(f=0, marks=0, since_mark=0, refill=False)

    def integrate(batch=None, least=1):
        if batch is None:
            batch = rng.random() < 0.35
        n = int(rng.integers(max(least, 1), 7)) if batch else 1
        first = st["f"] if st["f"] + n <= N_FRAMES else 0
        st["f"] = (first + n) % N_FRAMES
        ops.append(("integrate", str(rng.choice(BATCH_KINDS if batch else HOST_KINDS)), first, n))
        st["since_mark"] += 1

    def clean():
        ops.append(("clean",))
        if rng.random() < 0.2:
            ops.append(("clean",))   # a second pass with nothing new

    def hide():
        r = rng.random()
        if r < 0.45:
            hop = str(rng.choice(("hide", "show", "hide_others")))
            ops.append(("hide_list", hop, int(rng.choice((12, 64))), "most" if hop == "hide_others" else str(rng.choice(("hashed", "third")))))
        elif r < 0.85:
            hop = str(rng.choice(("hide", "show", "hide_others")))
            ops.append(("hide_box", hop, "most" if hop == "hide_others" else "middle"))
        else:
            ops.append(("show_all",))
        st["since_mark"] += 1

    def mark():
        ops.append(("mark",))
        st["marks"] += 1
        st["since_mark"] = 0

    integrate(batch=True, least=4)
    ops.append(("clean",))
    mark()
    for i in range(N_CHECKS):
        if st["refill"]:
            kind, st["refill"] = "batch_clean", False
        else:
            kind = str(rng.choice(PREDECESSORS, p=(0.2, 0.15, 0.15, 0.1, 0.13, 0.15, 0.12)))
            if kind == "check" and (i == 0 or ops[-1][0] != "check"):
                kind = "integrate"
            if kind == "restore" and st["since_mark"] == 0:
                kind = "hide"
        if kind != "check":
            r = rng.random()
            if r < 0.15:
                ops.append(("handoff",))
            elif r < 0.35:
                mark()
        if kind == "integrate":
            for _ in range(int(rng.integers(1, 4))):
                integrate()
        elif kind == "clean":
            if rng.random() < 0.6:
                integrate()
            clean()
        elif kind == "batch_clean":
            integrate(batch=True, least=4)
            clean()
        elif kind == "clear":
            ops.append(("clear",))
            st.update(f=0, refill=True)
            st["since_mark"] += 1
        elif kind == "restore":
            ops.append(("restore", int(rng.integers(0, st["marks"]))))
            st["since_mark"] += 1
        elif kind == "hide":
            hide()
        ops.append(("check", (seed * N_CHECKS + i) % len(READ_OUTS)))
    return ops


def predecessors(ops, at):
    """The kinds of PREDECESSORS that stand directly before the check at ops[at]."""
    prev = ops[at - 1]
    if prev[0] == "check":
        return {"check"}
    if prev[0] == "integrate":
        return {"integrate"}
    if prev[0] == "clean":
        j = at - 1
        while ops[j][0] == "clean":
            j -= 1
        batch = ops[j][0] == "integrate" and ops[j][1] in BATCH_KINDS and ops[j][3] >= 4
        return {"clean", "batch_clean"} if batch else {"clean"}
    if prev[0] in ("clear", "restore"):
        return {prev[0]}
    if prev[0] in ("hide_list", "hide_box", "show_all"):
        return {"hide"}
    raise AssertionError("op %r stands before a check" % (prev,))


def run_script(ops, m, primary=None, twin=None, on_check=None):
    """Drives the model (and the two engines: the twin takes every mutating operation and no read-out, the primary also the handoffs) through
    a script; on_check(k, i) is called for the i-th check and its result collected."""
    out, i = [], 0
    engines = [e for e in (primary, twin) if e is not None]
    for op in ops:
        if op[0] == "check":
            out.append(on_check(op[1], i))
            i += 1
        elif op[0] == "handoff":
            if primary is not None:
                primary.handoff()
        else:
            apply(op, m, engines)
    return out


def model_run(oracle_mod, seed):
    """The script of a seed on the model alone: ([(read-out index, figure, predecessors)], seconds)."""
    x = inputs()
    cfg, _, _ = config_of(seed)
    ops = script(seed)
    at = [j for j, op in enumerate(ops) if op[0] == "check"]
    t0 = time.perf_counter()
    m = Model(oracle_mod, x, **cfg)
    try:
        figs = run_script(ops, m, on_check=lambda k, i: model_figure(READ_OUTS[k], m, x))
    finally:
        m.close()
    return [(ops[j][1], fig, predecessors(ops, j)) for j, fig in zip(at, figs)], time.perf_counter() - t0
