"""What the GPU tests share (imported by tests only): capacities and geometry, the schedule driver, the byte-for-byte comparators, the
device-form helpers and the input builders more than one file needs.  A test file never imports a test file: what two of them need
lives here, in scenes.py, in faces.py or in the *_ref.py whose contract it restates.  No test and no fixture is defined here (a fixture
could not be shared without a conftest of its own), and every assertion carries its message: pytest rewrites bare asserts in test
modules and conftests only."""
import contextlib
import ctypes as C
import math
import re

import numpy as np

import align_ref as A
import cover_ref as V
import deviation_ref as D
import faces
import mesh_ref as M
import scenes
import track_ref as TR

# ---- capacities and geometry ----------------------------------------------------------------------------------------------------

DEPTH_CAPS = dict(max_bricks=120000, max_log_points=8 << 20, max_normals=1 << 21, max_frames=4096)  # the 640 x 480 depth streams
SMALL_CAPS = dict(max_bricks=60000, max_log_points=4 << 20, max_normals=1 << 20, max_frames=4096)   # 160 x 120 to 320 x 240 clouds
BBOX = scenes.BBOX_1M
RES = 0.002
IDENT = np.eye(4)[:3]
Z_CLIP = (0.28, 0.6)   # the handle's default z-clip (node.cpp:92-93)
HELD_OUT = 40          # frame index of the synthetic depth stream that is looked at and never integrated
SEED, POSE_SEED = 0xD3F7, 0x5E3  # scenes.DepthScene's


def grid(hfpf_mod, resolution=RES, **kw):
    return hfpf_mod.OccupancyGrid(resolution=resolution, bbox=BBOX, fuse_color=True, **dict(DEPTH_CAPS, **kw))


def run(g, sc, between=None, integrate=None):
    """Drives g through the schedule of a scenes.DepthScene: integrate(g, f) per frame (the scene's own by default), between(g, i)
    after step i."""
    integrate = integrate or sc.integrate
    for i, ev in enumerate(sc.schedule()):
        if ev[0] == "integrate":
            integrate(g, ev[1])
        else:
            g.clean()
        if between:
            between(g, i)


def counters(g):
    c = g.counters()
    # sized by what was asked of the handle, not by what was fused: counts the scratch a render, track or read-out keeps
    # (include/hfpf.h), and the frame ring is sized by the bytes of a frame (~5 per pixel of a depth image instead of 16)
    c.pop("device_bytes")
    # how the binned update scheduled its work: depends on how host frames happened to be batched (a render, a track or a query
    # launches waiting frames first), not on what was fused
    for k in ("points_direct", "table_misses", "update_extra_rounds"):
        c.pop(k)
    return c


# hfpf_get_counters fields that results depend on (the contract's list)
CONTRACT = ("points_presented", "points_zclip_pass", "points_in_bbox", "points_buffered", "dep_pairs_tested", "dep_pairs_member",
            "voxels_occupied", "voxels_with_normal", "bricks_allocated", "registrations", "frames_integrated", "clean_passes", "replay_members")


def contract_counters(g):
    c = g.counters()
    return {k: c[k] for k in CONTRACT}


# ---- batches from HBM and what HFPF_TRACE_CLEAN=1 says of the passes behind them ---------------------------------------------------

class DeviceFrames:
    """The frames of a scenes.Scene in HBM of one handle, handed over in batches with hfpf_integrate_device.  clouds: the frames as one
    uint8 array (frame_bytes(sc)), so that several handles share one rendering of the scene."""

    def __init__(self, g, sc, clouds=None):
        self.g, self.sc = g, sc
        self.stride = sc.W * sc.H * 16
        clouds = frame_bytes(sc) if clouds is None else clouds
        assert clouds.nbytes == self.stride * sc.n_frames, "%d bytes for %d frames of %d" % (clouds.nbytes, sc.n_frames, self.stride)
        self.dev = g.device_alloc(clouds.nbytes)
        g.device_upload(self.dev, clouds)

    def integrate(self, first, n):
        poses = np.stack([np.asarray(self.sc.poses[f], np.float64).reshape(12) for f in range(first, first + n)])
        self.g.integrate_device(self.dev + first * self.stride, n, self.stride, self.sc.W * self.sc.H, poses)

    def free(self):
        self.g.device_free(self.dev)


def frame_bytes(sc):
    """Every frame of a scenes.Scene (packed 16-byte records), one behind the other."""
    return np.concatenate([np.ascontiguousarray(sc.frame(f)).view(np.uint8).reshape(-1) for f in range(sc.n_frames)])


# every variable that changes which form an integrate call or a clean pass takes: a run "with defaults" has none set
FORM_VARIABLES = ("HFPF_CLEAN_NOWAIT", "HFPF_CLEAN_OVERLAP", "HFPF_EARLY_REPLAY", "HFPF_STREAM_REPLAY", "HFPF_MAILBOX", "HFPF_BIN_SPARE",
                  "HFPF_BIN_SLACK", "HFPF_UPD_SHAPE", "HFPF_UPDATE_FORM", "HFPF_BINNED", "HFPF_HOST_BATCH", "HFPF_TEST_BIN_SCALE",
                  "HFPF_TEST_TABLE_SKIP", "HFPF_TEST_STREAM_MIN", "HFPF_TEST_SORT_MIN", "HFPF_TEST_REG_LARGE_MIN", "HFPF_TEST_GATE4_MIN")

# the clean pass's lowered thresholds (HFPF_TEST_*_MIN) and HFPF_CLEAN_NOWAIT=0, so that frames of test size take the size-gated forms
STREAM_MIN, SORT_MIN, REG_LARGE_MIN, GATE4_MIN = 256, 1024, 1024, 4096
WAITED = {"HFPF_CLEAN_NOWAIT": "0"}
STREAM = {"HFPF_TEST_STREAM_MIN": str(STREAM_MIN)}
SORT = {"HFPF_TEST_SORT_MIN": str(SORT_MIN)}
LARGE = {"HFPF_TEST_GATE4_MIN": str(GATE4_MIN), "HFPF_TEST_REG_LARGE_MIN": str(REG_LARGE_MIN)}

_PASS_LINE = re.compile(r"hfpf: clean pass (\d+): (\d+) candidates, front half (beside the update kernel|on the engine's stream), "
                        r"replay (fed from the registrations|behind the dependant-table update)$")
_FORMS_LINE = re.compile(r"hfpf: clean forms (\d+): gate tiles ([14]) \((\d+) pending \+ (\d+) new\), register (small|large), "
                         r"compacting (no|planned|after the incremental update ran out), "
                         r"(no-wait|waited: single (\d+), walked (\d+), (sorted|unsorted), use_marks ([01]))$")


def clean_trace(err):
    """What the stderr text of a run with HFPF_TRACE_CLEAN=1 says of its clean passes: (lines, passes).  lines: every `hfpf: clean`
    line as printed.  passes: one dict per pass that launched kernels, in order, from its two lines -- pass, candidates, beside (front
    half beside the update kernel), fed (replay fed from the registrations), gate_tiles, pending, new, register ('small' | 'large'),
    compacting ('no' | 'planned' | 'after the incremental update ran out'), waited, and for a waited pass single (cells streamed),
    walked, sorted, use_marks (0 and False for a no-wait pass).  A line with either prefix that does not parse fails, and so does a
    pass with one line of the two."""
    lines = [ln for ln in err.splitlines() if ln.startswith("hfpf: clean ")]
    first, second = {}, {}
    for ln in lines:
        if ln.startswith("hfpf: clean pass"):
            m = _PASS_LINE.match(ln)
            assert m, "trace line not understood: %r" % ln
            first[int(m.group(1))] = dict(candidates=int(m.group(2)), beside=m.group(3).startswith("beside"), fed=m.group(4).startswith("fed"))
        elif ln.startswith("hfpf: clean forms"):
            m = _FORMS_LINE.match(ln)
            assert m, "trace line not understood: %r" % ln
            waited = m.group(7) != "no-wait"
            second[int(m.group(1))] = dict(gate_tiles=int(m.group(2)), pending=int(m.group(3)), new=int(m.group(4)), register=m.group(5),
                                           compacting=m.group(6), waited=waited, single=int(m.group(8) or 0), walked=int(m.group(9) or 0),
                                           sorted=m.group(10) == "sorted", use_marks=int(m.group(11) or 0))
    assert sorted(first) == sorted(second), "passes with a `clean pass` line %r, with a `clean forms` line %r" % (sorted(first), sorted(second))
    return lines, [dict(first[n], **second[n], **{"pass": n}) for n in sorted(first)]


def held_out(synth_mod, W=640, H=480, f=HELD_OUT):
    pose = synth_mod.pose(POSE_SEED, f)
    depth, _, K = synth_mod.depth_frame(SEED, f, W, H, pose)
    return depth, K, pose


# ---- one fused scene of tests/faces.py ------------------------------------------------------------------------------------------

class Session:
    """One scene fused on the engine with colour, its rows and occupied list, and what the read-out tests share of it."""

    def __init__(self, hfpf_mod, name, caps=SMALL_CAPS, **kw):
        self.name, self.H = name, hfpf_mod
        self.sc = faces.FaceScene(name)
        self.bbox, self.model_box = self.sc.bbox, self.sc.model_box
        self.g = hfpf_mod.OccupancyGrid(resolution=self.sc.resolution, bbox=self.bbox, fuse_color=True, **self.sc.config, **caps, **kw)
        self._mesh = None
        try:
            self.rows = scenes.run(self.g, self.sc, "integrate").copy()
            self.occ = self.g.occupied().copy()
            self.dims, self.res = self.g.dims
            print("%s: dims %r, device_bytes %d" % (name, self.dims, self.g.counters()["device_bytes"]))
            faces.check_conditions(name, self.rows, self.occ, self.dims)
        except BaseException:
            self.g.close()
            raise
        self.counters = counters(self.g)
        for a in (self.rows, self.occ):
            a.setflags(write=False)

    def own_mesh(self):
        """The session's own mesh at radius 2: (host vertices, host triangles, device vertices, device triangles)."""
        if self._mesh is None:
            v, t = self.g.extract_mesh(radius=2)
            dv, nv, dt, nt = self.g.extract_mesh_device(radius=2)
            assert nv == len(v) and nt == len(t) and nt > 1000, "the own mesh: %d / %d vertices, %d / %d triangles" % (nv, len(v), nt, len(t))
            assert self.g.device_download(dv, nv * 32).tobytes() == v.tobytes() and self.g.device_download(dt, nt * 12).tobytes() == t.tobytes(), \
                "the own mesh: host and device forms differ"
            self._mesh = (v, t, dv, dt)
        return self._mesh

    def close(self):
        if self.g is None:
            return
        if self._mesh is not None:
            self.g.device_free(self._mesh[2]), self.g.device_free(self._mesh[3])
        self.g.close()
        self.g = None


# ---- comparators ------------------------------------------------------------------------------------------------------------------

def _records(a):
    """a as (records, bytes): an element of a structured array is a record, of a plain one a row along the first axis."""
    a = np.ascontiguousarray(a)
    n = a.size if a.dtype.names else len(a)
    return a.reshape(-1).view(np.uint8).reshape(n, a.nbytes // n if n else 0), (a.reshape(-1) if a.dtype.names else a)


def same_records(got, ref, what, unit="records", where=None):
    """got and ref, one array each or a tuple of arrays (unit: one word, or one per array), are equal byte for byte per record.  None
    on both sides is skipped, None on one side fails.  Reports how many records differ, the first index (and where(index), if
    given) and both records."""
    if not isinstance(got, (tuple, list)):
        got, ref = (got,), (ref,)
    assert len(got) == len(ref), "%s: %d arrays vs %d" % (what, len(got), len(ref))
    units = (unit,) * len(got) if isinstance(unit, str) else unit
    for x, y, name in zip(got, ref, units):
        if x is None and y is None:
            continue
        assert x is not None and y is not None, "%s: %s: None against an array" % (what, name)
        (a, xr), (b, yr) = _records(x), _records(y)
        assert len(a) == len(b), "%s: %d vs %d %s" % (what, len(a), len(b), name)
        assert a.shape == b.shape, "%s: %s of %d bytes vs %d" % (what, name, a.shape[1], b.shape[1])
        bad = np.flatnonzero((a != b).any(axis=1))
        if bad.size:
            i = int(bad[0])
            raise AssertionError("%s: %d of %d %s differ, first %d%s: %r vs %r" % (what, bad.size, len(a), name, i,
                                                                                 " = %s" % (where(i),) if where else "", xr[i], yr[i]))


def same_summary(got, ref, keys, what):
    for k in keys:
        assert got[k] == ref[k], "%s: summary %s: %r vs %r" % (what, k, got[k], ref[k])


def same_planes(got, ref, what):
    """The planes of a render: same_records per pixel, reported as (v, u)."""
    for name in got:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(ref[name])
        assert a.shape == b.shape, "%s: plane %s: %r vs %r" % (what, name, a.shape, b.shape)
        px = a.shape[0] * a.shape[1]
        same_records(a.reshape(px, -1), b.reshape(px, -1), "%s: plane %s" % (what, name), "pixels", lambda i, w=a.shape[1]: "(v, u) %s" % (divmod(i, w),))


def same_query(got, ref, what):
    same_records(got, ref, what, ("hits", "rows"))


def same_mesh(got, ref, what):
    same_records(got, ref, what, ("vertices", "triangles"))


def same_components(got, ref, what):
    same_records(got, ref, what, ("rows", "labels", "components"))


def same_rays(got, ref, what):
    same_records(got, ref, what, "rays")


def same_deviation(got, ref, what):
    """(records, summary) of hfpf_compare_mesh."""
    same_records(got[0], ref[0], what, "rows")
    same_summary(got[1], ref[1], D.SUMMARY_KEYS, what)


def same_coverage(got, ref, what):
    """(records, summary) of hfpf_cover_mesh."""
    same_records(got[0], ref[0], what, "triangles")
    same_summary(got[1], ref[1], V.SUMMARY_KEYS, what)


ALIGN_FIELDS = ("iterations", "flags", "rows_sampled", "inliers", "rms")


def same_align(got, ref, what):
    for k in ALIGN_FIELDS:
        assert got[k] == ref[k], "%s: %s: %r vs %r" % (what, k, got[k], ref[k])
    assert got["pose"].tobytes() == ref["pose"].tobytes(), "%s: pose\n%r\nvs\n%r" % (what, got["pose"], ref["pose"])
    assert got["information"].tobytes() == ref["information"].tobytes(), "%s: information" % what


def same_track(got, ref, what):
    pose, r = got
    assert pose.tobytes() == np.asarray(ref["pose"], np.float64).tobytes(), "%s: pose %r vs %r" % (what, pose, ref["pose"])
    for k in ("iterations", "flags", "inliers", "points_used"):
        assert r[k] == ref[k], "%s: %s %r vs %r" % (what, k, r[k], ref[k])
    assert np.float64(r["rms"]).tobytes() == np.float64(ref["rms"]).tobytes(), "%s: rms %r vs %r" % (what, r["rms"], ref["rms"])
    assert r["information"].tobytes() == np.asarray(ref["information"], np.float64).tobytes(), "%s: information" % what


def coverage_sums(cov, s):
    """The summary of a cover is the sum of its records."""
    for k in ("n_samples", "n_in_bbox", "n_covered", "sum_dist_q30"):
        assert s[k] == sum(int(x) for x in cov[k]), k
    valid = (cov["flags"] & V.VALID) != 0
    assert s["n_tris_valid"] == int(valid.sum()) and s["n_tris_invalid"] == int((~valid).sum()), "valid and invalid triangles"
    assert s["max_distance"] == (float(cov["max_distance"].max()) if len(cov) else 0.0) and s["pad"] == 0, "max_distance, pad"
    assert not cov[~valid].view(np.uint8).any(), "an invalid triangle's record is all zero"


# ---- device forms -----------------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def uploaded(g, *arrays):
    """The device pointers of copies of host arrays in fresh allocations (of 16 bytes at least), freed on exit."""
    ptrs = []
    try:
        for a in arrays:
            a = np.ascontiguousarray(a)
            ptrs.append(g.device_alloc(max(a.nbytes, 16)))
            g.device_upload(ptrs[-1], a)
        yield ptrs
    finally:
        for p in ptrs:
            g.device_free(p)


def download(g, *parts, free=()):
    """One array per part (pointer, n, dtype): n records of dtype downloaded from pointer, or the empty array of dtype where the
    pointer or n is 0.  Every non-null pointer of parts and of `free` is freed once, whether a download raised or not."""
    try:
        return tuple(g.device_download(p, n * np.dtype(dt).itemsize).view(dt) if p and n else np.zeros(0, dt) for p, n, dt in parts)
    finally:
        for p in dict.fromkeys([p for p, _, _ in parts] + list(free)):
            if p:
                g.device_free(p)


def components_device(g, H, **kw):
    """hfpf_extract_components_device, downloaded: (rows, labels, comps)."""
    r, l, nr, c, nc = g.extract_components(device=True, **kw)
    return download(g, (r, nr, H.ROW_DTYPE), (l, nr, np.uint32), (c, nc, H.COMPONENT_DTYPE))


def mesh_device(g, **kw):
    """hfpf_extract_mesh_device, downloaded: (vertices, triangles)."""
    dv, nv, dt, nt = g.extract_mesh_device(**kw)
    v, t = download(g, (dv, nv, M.VERTEX_DTYPE), (dt, 3 * nt, np.uint32))
    return v, t.reshape(-1, 3)


def compare_device(g, H, d_verts, n_verts, stride, d_tris, n_tris, pose, rows=False, **kw):
    """hfpf_compare_mesh_device on a mesh in HBM, downloaded: (dev, summary) or (rows, dev, summary)."""
    r, d, nr, s = g.compare_mesh(d_verts, d_tris, pose, device=True, rows=rows, n_verts=n_verts, vertex_stride=stride, n_tris=n_tris, **kw)
    dev, out_rows = download(g, (d, nr, H.DEVIATION_DTYPE), (r if rows else 0, nr, H.ROW_DTYPE), free=(r,))
    return (out_rows if nr else None, dev, s) if rows else (dev, s)


def cover_device(g, H, d_verts, n_verts, stride, d_tris, n_tris, pose, **kw):
    """hfpf_cover_mesh_device on a mesh in HBM, downloaded: (records, summary)."""
    c, s = g.cover_mesh(d_verts, d_tris, pose, device=True, n_verts=n_verts, vertex_stride=stride, n_tris=n_tris, **kw)
    return download(g, (c, n_tris, H.TRI_COVERAGE_DTYPE))[0], s


def align_device(g, verts, tris, pose, **kw):
    with uploaded(g, verts, tris) as (dv, dt):
        return g.align_mesh(dv, dt, pose, device=True, n_verts=len(verts), vertex_stride=verts.dtype.itemsize, n_tris=len(tris), **kw)


def rays_device(g, rays, pose, **kw):
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    with uploaded(g, rays) as (d,):
        return g.raycast_device(d, len(rays), pose, **kw)


# ---- "a read-out changes nothing" -------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def two_handles(hfpf_mod, sc, look, on_empty):
    """Handle a runs the scene alone; handle b takes on_empty(b) while it is empty and look(b, i) after every step i of the schedule.
    Their rows and counters are equal; then (a, b, rows) go to the caller for what its read-out gives on b, which ends with
    unchanged(a, b, rows) before anything else is integrated."""
    with grid(hfpf_mod) as a, grid(hfpf_mod) as b:
        run(a, sc)
        on_empty(b)
        run(b, sc, between=look)
        ra, rb = a.extract(), b.extract()
        assert len(ra) > 0 and ra.tobytes() == rb.tobytes(), "the rows differ after the read-outs between the steps"
        assert counters(a) == counters(b), "counters: %r vs %r" % (counters(a), counters(b))
        yield a, b, rb


def unchanged(a, b, rows):
    assert b.extract().tobytes() == rows.tobytes(), "the read-outs changed the rows"
    assert counters(a) == counters(b), "counters: %r vs %r" % (counters(a), counters(b))


# ---- align and track inputs ---------------------------------------------------------------------------------------------------------

ALIGN_MD = 6 * RES
ALIGN_KW = dict(max_iterations=8, max_distance=ALIGN_MD, eps_rotation=1e-5, eps_translation=1e-5)
# the start pose: 0.3 degrees about the bounding box's centre and 1.5 voxels of translation away from the true pose (the identity)
ALIGN_START = A.rigid(0.3, (0.5, 1.0, -0.4), (0.6 * 1.5 * RES, -0.64 * 1.5 * RES, 0.48 * 1.5 * RES), A.centre(BBOX))


def fitted(r):
    """A result that is a fit and not a failed one: most sampled rows are inliers and the residual went down."""
    return 2 * r["inliers"] > r["rows_sampled"] and r["flags"] in (0, A.CONVERGED) and r["iterations"] > 1


Z_RANGE = (0.05, 3.0)
TRACK_OPTS = dict(max_iterations=30, max_distance=0.03, damping=1e-6, eps_rotation=1e-6, eps_translation=1e-6, z_range=Z_RANGE,
                  splat_radius=-1, max_splat_radius=4, cull_backfaces=True)


def perturb(pose, deg, shift, axis=(1.0, -0.5, 0.3)):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    rot = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    return np.hstack([rot @ pose[:, :3], (pose[:, 3] + np.asarray(shift, np.float64)).reshape(3, 1)])


def pose_errors(pose, ref):
    """(metres, degrees) between two poses."""
    dR = pose[:, :3] @ ref[:, :3].T
    return float(np.linalg.norm(pose[:, 3] - ref[:, 3])), math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1) / 2))))


def track_reference(rows, points, pose, K, W, H, **kw):
    """track_ref on rows at RES under TRACK_OPTS (kw overrides them)."""
    o = dict(TRACK_OPTS, **kw)
    view = dict(K=K, width=W, height=H, z_range=Z_RANGE, splat_radius=-1, max_splat_radius=4, flags=1)
    return TR.track(rows, points, pose, RES, view, Z_CLIP, max_iterations=o["max_iterations"], min_inliers=6,
                    max_distance=o["max_distance"], damping=o["damping"], eps_rotation=o["eps_rotation"],
                    eps_translation=o["eps_translation"])


# ---- the specks of the component tests: two flat patches well clear of the surface ------------------------------------------------

PATCH_CELLS = 15         # a patch is PATCH_CELLS x PATCH_CELLS voxels, one voxel thick; its interior passes the gate of 20 neighbours
PATCH_CLEAR = 0.08       # metres between a patch's centre and the nearest occupied voxel (Chebyshev): 0.05 clear of its rim
PATCH_DEPTH = 0.4        # camera-frame z of a patch's points (inside the default z-clip 0.28 .. 0.6)


def free_spots(occ, bbox=BBOX, res=RES, clear=PATCH_CLEAR, cell=0.01):
    """Centres (fusion frame, voxel-centred in z) of two places at least `clear` (Chebyshev) from every occupied voxel and 0.1 m from
    the bounding box: the first and the last free cell of a 1 cm grid in lexicographic order."""
    lo = np.asarray(bbox, np.float64)[0::2]
    hi = np.asarray(bbox, np.float64)[1::2]
    n = np.round((hi - lo) / cell).astype(int)
    coarse = np.zeros(n, bool)
    c = np.clip(np.floor((np.asarray(occ, np.float64) + 0.5) * res / cell).astype(int), 0, n - 1)
    coarse[c[:, 0], c[:, 1], c[:, 2]] = True
    r = int(np.ceil(clear / cell)) + 1  # + 1: an occupied voxel may sit anywhere inside its coarse cell
    for axis in range(3):
        grown = coarse.copy()
        for s in range(1, r + 1):
            for sign in (1, -1):
                sh = np.roll(coarse, sign * s, axis=axis)
                idx = [slice(None)] * 3
                idx[axis] = slice(0, s) if sign == 1 else slice(n[axis] - s, None)
                sh[tuple(idx)] = False
                grown |= sh
        coarse = grown
    m = int(round(0.1 / cell))
    free = ~coarse
    inner = np.zeros_like(free)
    inner[m:n[0] - m, m:n[1] - m, m:n[2] - m] = True
    cells = np.argwhere(free & inner)
    assert len(cells) >= 2, "no room for the patches"
    spots = []
    for cc in (cells[0], cells[-1]):
        p = lo + (cc + 0.5) * cell
        p[2] = lo[2] + (np.floor((p[2] - lo[2]) / res) + 0.5) * res
        spots.append(p)
    assert np.abs(spots[0] - spots[1]).max() >= 0.1, "the two patches must be apart"
    return spots


def patch_cloud(centre, bbox=BBOX, res=RES, cells=PATCH_CELLS, per_cell=3):
    """(records, pose, voxel box) of one flat patch: per_cell^2 points in every voxel of a cells x cells square of the z-plane through
    `centre`, as packed 16-byte x, y, z, rgb records in the frame of a camera looking along +z from PATCH_DEPTH in front of it."""
    lo = np.asarray(bbox, np.float64)[0::2]
    v0 = np.floor((np.asarray(centre) - lo) / res).astype(int) - np.array([cells // 2, cells // 2, 0])
    t = (np.arange(cells * per_cell) + 0.5) / per_cell  # voxel units: no point on a voxel boundary
    u, v = np.meshgrid(t, t, indexing="ij")
    origin = lo + v0 * res  # the patch's low corner; z: the voxel's low face
    cam_t = np.array([origin[0], origin[1], origin[2] + 0.5 * res - PATCH_DEPTH])
    rec = np.zeros((u.size, 4), np.float32)
    rec[:, 0], rec[:, 1], rec[:, 2] = (u * res).ravel(), (v * res).ravel(), PATCH_DEPTH
    rec[:, 3] = np.array([0x00FF00FF], np.uint32).view(np.float32)[0]
    pose = np.hstack([np.eye(3), cam_t.reshape(3, 1)])
    box = (v0, v0 + np.array([cells - 1, cells - 1, 0]))
    return np.ascontiguousarray(rec), pose, box


def add_patches(g):
    """Integrates the two patches on top of what g holds and cleans; returns their voxel boxes."""
    boxes = []
    for centre in free_spots(g.occupied()):
        rec, pose, box = patch_cloud(centre)
        g.integrate(rec, pose)
        boxes.append(box)
    g.clean()
    return boxes


def in_boxes(rows, boxes):
    m = np.zeros(len(rows), bool)
    for lo, hi in boxes:
        m |= ((rows["ix"] >= lo[0]) & (rows["ix"] <= hi[0]) & (rows["iy"] >= lo[1]) & (rows["iy"] <= hi[1]) & (rows["iz"] >= lo[2]) &
              (rows["iz"] <= hi[2]))
    return m


# ---- the node shell -------------------------------------------------------------------------------------------------------------

def node_feed(n, sc):
    n.start()
    for f in range(sc.n_frames):
        depth, rgb, K = sc.frames[f]
        n._tf_py = lambda target, source, pose=sc.poses[f]: pose
        assert n.publish_depth(depth, K, color=rgb) == 1, "frame %d was not taken" % f


def node_grid(hfpf_mod, hfpf_node, n):
    """The node's engine handle as an OccupancyGrid (not owned: reset _h before it is collected)."""
    g = hfpf_mod.OccupancyGrid.__new__(hfpf_mod.OccupancyGrid)
    g._h, g._transport = C.c_void_p(hfpf_node.lib().hfpf_node_grid(n._h)), None
    return g


def deviation_csv(rows, dev):
    lines = ["ix,iy,iz,signed_distance,distance,tri,flags"]
    for r, d in zip(rows, dev):
        lines.append("%d,%d,%d,%s,%s,%d,%d" % (r["ix"], r["iy"], r["iz"], _g(d["signed_distance"]), _g(d["distance"]), d["tri"], d["flags"]))
    return "\n".join(lines) + "\n"


def _g(v):
    return "nan" if np.isnan(v) else "%.9g" % float(v)


def deviation_summary_csv(s):
    keys = ("n_rows", "n_found", "n_negative", "n_tris_valid", "n_tris_invalid", "max_abs", "sum_abs_q30", "sum_sq_q30")
    return ",".join(keys) + "\n" + ",".join(_g(s[k]) if k == "max_abs" else "%d" % s[k] for k in keys) + "\n"


# ---- virtual ranks ----------------------------------------------------------------------------------------------------------------

def run_virtual(hfpf_mod, sc, world, fuse_color=False, deal=None, gathered=False):
    import hfpf_dist
    grids = [hfpf_mod.OccupancyGrid(resolution=sc.resolution, bbox=sc.bbox, fuse_color=fuse_color, **SMALL_CAPS) for _ in range(world)]
    vr = hfpf_dist.LocalVirtualRanks(grids, gathered=gathered)
    deal = deal or (lambda f: f % world)
    fb = sc.W * sc.H * 16
    try:
        for ev in sc.schedule():
            if ev[0] == "integrate":
                f = ev[1]
                g = grids[deal(f)]
                dev = g.device_alloc(fb)
                g.device_upload(dev, sc.frame(f))
                g.integrate_device(dev, 1, fb, sc.W * sc.H, sc.poses[f].reshape(1, 12), frame_ids=np.array([f], np.uint32))
                g.sync()
                g.device_free(dev)
            else:
                vr.clean_all()
        rows = vr.extract(on=world - 1)
        occ = grids[0].occupied()
        ctrs = [g.counters() for g in grids]
    finally:
        for g in grids:
            g.close()
    return rows, occ, ctrs
