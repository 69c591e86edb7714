"""What the Python binding hands to the C ABI and what it makes of the results, seen by a fake library that records every call.
No GPU and no libhfpf.so: the grid is made without hfpf_create, and the fake fills the outputs through byref(...)._obj with
arrays from libc's malloc, as the engine does.  Every expectation here is written out by hand."""
import ctypes as C

import numpy as np
import pytest

import hfpf as H

libc = C.CDLL(None)
libc.malloc.restype = C.c_void_p
libc.malloc.argtypes = [C.c_size_t]
libc.free.argtypes = [C.c_void_p]

K = (100.0, 101.0, 8.0, 6.0)
IDENTITY = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
POSE = np.arange(12, dtype=np.float64).reshape(3, 4) + 0.5
POSES = np.arange(24, dtype=np.float64).reshape(2, 3, 4) - 3.0
V3 = np.arange(9, dtype=np.float32).reshape(3, 3)                 # 3 vertices as (3, 3) float32: stride 12
VR = np.zeros(3, H.MESH_VERTEX_DTYPE)                             # the same as records: stride 32
T1 = np.array([[0, 1, 2]], np.uint32)
V4 = np.arange(12, dtype=np.float32).reshape(4, 3)                # 2 triangles, for the per-triangle records
T2 = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
PLANES = np.array([[0.0, 0.0, 1.0, 0.5], [1.0, 0.0, 0.0, 0.25]])
FRAMES = np.zeros((2, 12, 16), np.uint16)


class FakeLib:
    """Stands in for hfpf.lib().  calls: (name, args) of every call, in order; on[name](*args) fills the outputs and gives the
    return code (0 without one)."""

    def __init__(self):
        self.calls, self.on, self.blocks = [], {"hfpf_last_error": lambda h: b"fake"}, []

    def __getattr__(self, name):
        if not name.startswith("hfpf_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return self.on.get(name, lambda *a: 0)(*args)
        return fn

    def named(self, name):
        return [args for n, args in self.calls if n == name]

    def give(self, a):
        """The address of a malloc'd copy of a's bytes."""
        p = libc.malloc(max(a.nbytes, 1))
        C.memmove(p, a.ctypes.data, a.nbytes)
        self.blocks.append(p)
        return p

    def hand_out(self, name, outs, counts, summary=None):
        """Let `name` hand out a copy of outs[i] through argument i (where the caller passed a pointer), set the counts and fill
        the summary {argument index: {field: value}}; returns {i: address handed out}."""
        given = {}

        def fill(*args):
            for i, a in outs.items():
                if args[i] is not None:
                    given[i] = args[i]._obj.value = self.give(a)
            for i, n in counts.items():
                args[i]._obj.value = n
            for i, fields in (summary or {}).items():
                for k, v in fields.items():
                    setattr(args[i]._obj, k, v)
            return 0
        self.on[name] = fill
        return given


@pytest.fixture
def fake(monkeypatch):
    f = FakeLib()
    monkeypatch.setattr(H, "_lib", f)
    yield f
    for p in f.blocks:
        libc.free(p)


@pytest.fixture
def grid(fake):
    g = H.OccupancyGrid.__new__(H.OccupancyGrid)
    g._h, g._transport = C.c_void_p(0x1234), None
    yield g
    g._h = None


def addr(arg):
    """The address a pointer argument holds; None for None (NULL)."""
    return None if arg is None else arg.value


def doubles(arg, n=12):
    return list((C.c_double * n).from_address(arg.value))


def rec(dtype, n, seed=0, shape=None):
    """n records of dtype with known bytes."""
    dtype = np.dtype(dtype)
    a = ((np.arange(n * dtype.itemsize * (int(np.prod(shape)) if shape else 1)) + seed) % 251).astype(np.uint8).view(dtype)
    return a.reshape((n,) + shape) if shape else a


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


# ---- the five mesh methods: mesh arguments at 2..6, the mesh pose at 7 ----
MESH_METHODS = {
    "compare_mesh": lambda g, v, t, **kw: g.compare_mesh(v, t, **kw),
    "align_mesh": lambda g, v, t, **kw: g.align_mesh(v, t, **kw),
    "cover_mesh": lambda g, v, t, **kw: g.cover_mesh(v, t, **kw),
    "section_mesh": lambda g, v, t, **kw: g.section_mesh(v, t, planes=PLANES, **kw),
    "plan_views": lambda g, v, t, **kw: g.plan_views(v, t, POSES, K=K, width=16, height=12, **kw),
}
V0, T0 = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32)
MESH_CASES = {  # name: (verts, tris, keywords, the five arguments expected)
    "f32": (V3, T1, {}, (V3.ctypes.data, 3, 12, T1.ctypes.data, 1)),
    "records": (VR, T1, {}, (VR.ctypes.data, 3, 32, T1.ctypes.data, 1)),
    "empty": (V0, T0, {}, (None, 0, 12, None, 0)),
    "n_verts": (V3, T1, dict(n_verts=2), (V3.ctypes.data, 2, 12, T1.ctypes.data, 1)),
    "vertex_stride": (V3, T1, dict(vertex_stride=16), (V3.ctypes.data, 3, 16, T1.ctypes.data, 1)),
    "n_tris": (V3, T1, dict(n_tris=0), (V3.ctypes.data, 3, 12, T1.ctypes.data, 0)),
    "device": (0x7000, 0x8000, dict(device=True, n_verts=3, vertex_stride=12, n_tris=1), (0x7000, 3, 12, 0x8000, 1)),
}


@pytest.mark.parametrize("case", sorted(MESH_CASES))
@pytest.mark.parametrize("method", sorted(MESH_METHODS))
def test_mesh_arguments(fake, grid, method, case):
    v, t, kw, want = MESH_CASES[case]
    MESH_METHODS[method](grid, v, t, **kw)
    name, args = fake.calls[0]
    assert name == "hfpf_" + method + ("_device" if case == "device" else "")
    assert args[0] is grid._h
    assert (addr(args[2]), args[3], args[4], addr(args[5]), args[6]) == want
    assert all(type(args[i]) is int for i in (3, 4, 6))
    assert doubles(args[7]) == IDENTITY


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("method", sorted(MESH_METHODS))
def test_mesh_pose(fake, grid, method, device):
    v, t, kw, _ = MESH_CASES["device" if device else "f32"]
    MESH_METHODS[method](grid, v, t, pose=POSE, **kw)
    assert doubles(fake.calls[0][1][7]) == [0.5 + i for i in range(12)]
    MESH_METHODS[method](grid, v, t, pose=POSE[:, ::-1].astype(np.float32), **kw)  # neither contiguous nor float64
    assert doubles(fake.named(fake.calls[0][0])[1][7]) == [3.5, 2.5, 1.5, 0.5, 7.5, 6.5, 5.5, 4.5, 11.5, 10.5, 9.5, 8.5]
    with pytest.raises(ValueError, match="cannot reshape array of size 5 into shape \\(12,\\)"):
        MESH_METHODS[method](grid, v, t, pose=np.zeros(5), **kw)


def test_mesh_vertices_that_need_a_copy(fake, grid):
    """float64 vertices and int64 triangles are converted: the pointers are those of float32 / uint32 copies with the same values."""
    grid.align_mesh(V3.astype(np.float64), T1.astype(np.int64))
    args = fake.calls[0][1]
    assert addr(args[2]) not in (None, V3.ctypes.data) and args[3:5] == (3, 12) and args[6] == 1
    assert list((C.c_float * 9).from_address(addr(args[2]))) == list(range(9))
    assert list((C.c_uint32 * 3).from_address(addr(args[5]))) == [0, 1, 2]


def test_section_mesh_planes_and_its_device_alias(fake, grid):
    grid.section_mesh(V3, T1)
    args = fake.calls[0][1]
    assert (args[8], args[9], args[16]) == (None, 0, None)
    recs = grid.section_mesh(V3, T1, planes=PLANES)[3]
    args = fake.calls[2][1]  # calls[1] is the first call's hfpf_free_section
    assert (addr(args[8]), args[9], addr(args[16])) == (PLANES.ctypes.data, 2, recs.ctypes.data)
    assert recs.dtype == H.SECTION_PLANE_DTYPE and recs.shape == (2,)
    fake.calls.clear()
    out = grid.section_mesh_device(0x7000, 3, 12, 0x8000, 1, POSE, PLANES)
    name, args = fake.calls[0]
    assert name == "hfpf_section_mesh_device" and len(fake.calls) == 1
    assert (addr(args[2]), args[3], args[4], addr(args[5]), args[6], args[9]) == (0x7000, 3, 12, 0x8000, 1, 2)
    assert out[:3] == ((0, 0), (0, 0), (0, 0))


def test_plan_views_scores_and_poses(fake, grid):
    scores = rec(H.VIEW_SCORE_DTYPE, 2, 9)
    fake.on["hfpf_plan_views"] = lambda *a: C.memmove(a[10].value, scores.ctypes.data, scores.nbytes) and 0
    got = grid.plan_views(V3, T1, POSES, K=K, width=16, height=12)
    args = fake.calls[0][1]
    assert (addr(args[8]), args[9]) == (POSES.ctypes.data, 2)
    same(got[0], scores)
    fake.calls.clear()
    del fake.on["hfpf_plan_views"]
    got = grid.plan_views(V3, T1, np.zeros((0, 3, 4)), K=K, width=16, height=12)
    args = fake.calls[0][1]
    assert (args[8], args[9]) == (None, 0) and addr(args[10]) is not None  # room for one score, never NULL
    assert got[0].dtype == H.VIEW_SCORE_DTYPE and got[0].shape == (0,)
    with pytest.raises(ValueError, match="cannot reshape"):
        grid.plan_views(V3, T1, np.zeros(13), K=K, width=16, height=12)


# ---- the eight sites that copy engine-owned host arrays out and free them ----
ROWS, LABELS, COMPS = rec(H.ROW_DTYPE, 2, 1), rec(np.uint32, 2, 2), rec(H.COMPONENT_DTYPE, 2, 3)
VERTS, TRIS = rec(H.MESH_VERTEX_DTYPE, 2, 4), rec(np.uint32, 2, 5, (3,))


def check_free(fake, name, want):
    """`name` ran exactly once, with these addresses (None = NULL)."""
    calls = fake.named(name)
    assert len(calls) == 1 and tuple(addr(a) for a in calls[0]) == tuple(want)


def test_read_ply(fake):
    given = fake.hand_out("hfpf_read_ply", {1: VERTS, 3: TRIS}, {2: 2, 4: 2})
    verts, tris = H.read_ply("some.ply")
    assert fake.calls[0][1][0] == b"some.ply"
    same(verts, VERTS)
    same(tris, TRIS)
    check_free(fake, "hfpf_free_mesh", (given[1], given[3]))


def test_read_ply_empty_and_failing(fake):
    verts, tris = H.read_ply("some.ply")
    same(verts, np.zeros(0, H.MESH_VERTEX_DTYPE))
    same(tris, np.zeros((0, 3), np.uint32))
    check_free(fake, "hfpf_free_mesh", (None, None))
    fake.calls.clear()
    fake.on["hfpf_read_ply"] = lambda *a: -6
    with pytest.raises(H.HfpfError, match="IO.*fake"):
        H.read_ply("some.ply")
    assert fake.named("hfpf_free_mesh") == []


def test_extract_mesh(fake, grid):
    given = fake.hand_out("hfpf_extract_mesh", {2: VERTS, 4: TRIS}, {3: 2, 5: 2})
    verts, tris = grid.extract_mesh(radius=3)
    o = fake.calls[0][1][1]._obj
    assert (type(o), o.struct_size, o.radius) == (H.MeshOpts, C.sizeof(H.MeshOpts), 3)
    same(verts, VERTS)
    same(tris, TRIS)
    check_free(fake, "hfpf_free_mesh", (given[2], given[4]))


@pytest.mark.parametrize("rows", (True, False))
def test_extract_components(fake, grid, rows):
    given = fake.hand_out("hfpf_extract_components", {2: ROWS, 3: LABELS, 5: COMPS}, {4: 2, 6: 2})
    out, labels, comps = grid.extract_components(rows=rows, reach=2)
    args = fake.calls[0][1]
    assert args[1]._obj.reach == 2 and (args[2] is None) == (not rows)
    if rows:
        same(out, ROWS)
    else:
        assert out is None
    same(labels, LABELS)
    same(comps, COMPS)
    check_free(fake, "hfpf_free_components", (given.get(2), given[3], given[5]))


@pytest.mark.parametrize("rows", (True, False))
def test_compare_mesh(fake, grid, rows):
    dev = rec(H.DEVIATION_DTYPE, 2, 6)
    given = fake.hand_out("hfpf_compare_mesh", {8: ROWS, 9: dev}, {10: 2}, {11: dict(n_rows=2, n_found=1, max_abs=0.25)})
    got = grid.compare_mesh(V3, T1, rows=rows, max_distance=0.5)
    args = fake.calls[0][1]
    assert args[1]._obj.max_distance == 0.5 and (args[8] is None) == (not rows)
    assert len(got) == (3 if rows else 2)
    if rows:
        same(got[0], ROWS)
    same(got[-2], dev)
    assert (got[-1]["n_rows"], got[-1]["n_found"], got[-1]["max_abs"]) == (2, 1, 0.25)
    check_free(fake, "hfpf_free_deviation", (given.get(8), given[9]))


def test_cover_mesh(fake, grid):
    cov = rec(H.TRI_COVERAGE_DTYPE, 2, 7)
    given = fake.hand_out("hfpf_cover_mesh", {8: cov}, {}, {9: dict(n_samples=7, area_q40_hi=1, area_q40_lo=1 << 31)})
    got, summary = grid.cover_mesh(V4, T2, spacing=0.01)
    assert fake.calls[0][1][1]._obj.spacing == 0.01
    same(got, cov)  # one record per triangle: n_tris of them
    assert summary["n_samples"] == 7 and summary["area"] == (2.0 ** 32 + 2.0 ** 31) / 2.0 ** 40
    check_free(fake, "hfpf_free_coverage", (given[8],))
    fake.calls.clear()
    same(grid.cover_mesh(V4, T2, n_tris=1)[0], cov[:1])


@pytest.mark.parametrize("tri_plan", (True, False))
def test_plan_views_records(fake, grid, tri_plan):
    plan = rec(H.TRI_PLAN_DTYPE, 2, 8)
    given = fake.hand_out("hfpf_plan_views", {11: plan}, {}, {12: dict(n_views=2, n_selected=1)})
    scores, got, summary = grid.plan_views(V4, T2, POSES, tri_plan=tri_plan, K=K, width=16, height=12)
    assert (fake.calls[0][1][11] is None) == (not tri_plan)
    if tri_plan:
        same(got, plan)
    else:
        assert got is None
    assert scores.shape == (2,) and (summary["n_views"], summary["n_selected"]) == (2, 1)
    check_free(fake, "hfpf_free_plan", (given.get(11),))


def test_section_mesh(fake, grid):
    points, segments, contours = rec(H.SECTION_POINT_DTYPE, 2, 9), rec(H.SECTION_SEGMENT_DTYPE, 2, 10), rec(H.SECTION_CONTOUR_DTYPE, 2, 11)
    given = fake.hand_out("hfpf_section_mesh", {10: points, 12: segments, 14: contours}, {11: 2, 13: 2, 15: 2}, {17: dict(n_segments=2)})
    got = grid.section_mesh(V3, T1, planes=PLANES)
    for a, b in zip(got[:3], (points, segments, contours)):
        same(a, b)
    assert got[4]["n_segments"] == 2
    check_free(fake, "hfpf_free_section", (given[10], given[12], given[14]))


@pytest.mark.parametrize("rows", (True, False))
def test_depth_consistency(fake, grid, rows):
    cons = rec(H.ROW_CONSISTENCY_DTYPE, 2, 12)
    given = fake.hand_out("hfpf_depth_consistency", {7: ROWS, 8: cons}, {9: 2}, {10: dict(n_rows=2, n_kept=1)})
    out, got, summary = grid.depth_consistency(FRAMES, POSES, K, rows=rows, window=1)
    args = fake.calls[0][1]
    d = args[2]._obj
    assert args[1]._obj.window == 1 and (d.width, d.height, d.depth_format, d.depth_step) == (16, 12, H.DEPTH_U16, 32)
    assert (addr(args[3]), args[4], args[5], addr(args[6])) == (FRAMES.ctypes.data, 384, 2, POSES.ctypes.data)
    assert (args[7] is None) == (not rows)
    if rows:
        same(out, ROWS)
    else:
        assert out is None
    same(got, cons)
    assert (summary["n_rows"], summary["n_kept"]) == (2, 1)
    check_free(fake, "hfpf_free_consistency", (given.get(7), given[8]))


def test_depth_consistency_without_frames(fake, grid):
    grid.depth_consistency(np.zeros((0, 12, 16), np.uint16), np.zeros((0, 3, 4)), K)
    args = fake.calls[0][1]
    assert (args[3], args[4], args[5], args[6]) == (None, 384, 0, None)


COPY_OUT_SITES = {  # method: (call, its free function with the number of pointers, the empty arrays expected with nothing handed out)
    "extract_mesh": (lambda g: g.extract_mesh(), ("hfpf_free_mesh", 2), [(H.MESH_VERTEX_DTYPE, (0,)), (np.uint32, (0, 3))]),
    "extract_components": (lambda g: g.extract_components(), ("hfpf_free_components", 3),
                           [(H.ROW_DTYPE, (0,)), (np.uint32, (0,)), (H.COMPONENT_DTYPE, (0,))]),
    "compare_mesh": (lambda g: g.compare_mesh(V3, T1, rows=True), ("hfpf_free_deviation", 2), [(H.ROW_DTYPE, (0,)), (H.DEVIATION_DTYPE, (0,))]),
    "cover_mesh": (lambda g: g.cover_mesh(V3, T1), ("hfpf_free_coverage", 1), [(H.TRI_COVERAGE_DTYPE, (0,))]),
    "section_mesh": (lambda g: g.section_mesh(V3, T1), ("hfpf_free_section", 3),
                     [(H.SECTION_POINT_DTYPE, (0,)), (H.SECTION_SEGMENT_DTYPE, (0,)), (H.SECTION_CONTOUR_DTYPE, (0,))]),
    "plan_views": (lambda g: g.plan_views(V3, T1, POSES, K=K, width=16, height=12)[1:], ("hfpf_free_plan", 1), [(H.TRI_PLAN_DTYPE, (0,))]),
    "depth_consistency": (lambda g: g.depth_consistency(FRAMES, POSES, K), ("hfpf_free_consistency", 2),
                          [(H.ROW_DTYPE, (0,)), (H.ROW_CONSISTENCY_DTYPE, (0,))]),
}


@pytest.mark.parametrize("method", sorted(COPY_OUT_SITES))
def test_nothing_to_copy_still_frees_once(fake, grid, method):
    call, (free, n), want = COPY_OUT_SITES[method]
    got = call(grid)
    for a, (dtype, shape) in zip(got, want):
        same(a, np.zeros(shape, dtype))
    check_free(fake, free, (None,) * n)


@pytest.mark.parametrize("method", sorted(COPY_OUT_SITES))
def test_a_failed_call_raises_and_frees_nothing(fake, grid, method):
    call, (free, _), _ = COPY_OUT_SITES[method]
    fake.on["hfpf_" + method] = lambda *a: -2
    with pytest.raises(H.HfpfError, match="BAD_ARG.*fake") as e:
        call(grid)
    assert e.value.code == -2 and fake.named(free) == []


def test_copy_out_frees_when_a_copy_cannot_be_made(fake, grid):
    fake.hand_out("hfpf_extract_mesh", {2: VERTS, 4: TRIS}, {3: 2, 5: 1 << 62})  # no room for that many triangles
    with pytest.raises((MemoryError, ValueError)):
        grid.extract_mesh()
    assert len(fake.named("hfpf_free_mesh")) == 1


# ---- results in device buffers: the caller's, or scratch buffers that come back as arrays ----
def device_memory(fake):
    """hfpf_device_alloc hands out 0x5100, 0x5200, ...; returns the list the allocations' sizes go to."""
    sizes = []

    def alloc(h, nbytes, out):
        sizes.append(nbytes)
        out._obj.value = 0x5000 + 0x100 * len(sizes)
        return 0
    fake.on["hfpf_device_alloc"] = alloc
    return sizes


DEVICE_SITES = {  # method: (call(grid, **kw), C function, index of the hits pointer, records, shape of the result)
    "query_device": (lambda g, **kw: g.query_device(0xA000, 5, POSE, rows=False, **kw), "hfpf_query_device", 9, 5, H.QUERY_HIT_DTYPE, (5,)),
    "raycast_device": (lambda g, **kw: g.raycast_device(0xA000, 5, POSE, **kw), "hfpf_raycast_device", 5, 5, H.RAY_HIT_DTYPE, (5,)),
    "raycast_views_device": (lambda g, **kw: g.raycast_views_device(POSES, K, 4, 3, **kw), "hfpf_raycast_view_device", 10, 24, H.RAY_HIT_DTYPE,
                             (2, 3, 4)),
}


@pytest.mark.parametrize("method", sorted(DEVICE_SITES))
def test_results_stay_in_the_callers_device_buffer(fake, grid, method):
    call, cfn, at, _, _, _ = DEVICE_SITES[method]
    assert call(grid, dev_hits=0xE000) is None
    assert [n for n, _ in fake.calls] == [cfn] and addr(fake.calls[0][1][at]) == 0xE000


@pytest.mark.parametrize("fails", (False, True))
@pytest.mark.parametrize("method", sorted(DEVICE_SITES))
def test_results_through_a_scratch_device_buffer(fake, grid, method, fails):
    call, cfn, at, n, dtype, shape = DEVICE_SITES[method]
    sizes = device_memory(fake)
    if fails:
        fake.on[cfn] = lambda *a: -4
        with pytest.raises(H.HfpfError, match="HIP"):
            call(grid)
    else:
        got = call(grid)
        got = got[0] if method == "query_device" else got
        assert got.dtype == dtype and got.shape == shape
        if method == "query_device":
            assert call(grid)[1] is None  # rows=False
    assert sizes[0] == n * 64 and addr(fake.named(cfn)[0][at]) == 0x5100
    downloads = fake.named("hfpf_device_download")[:1]
    assert [(addr(a[2]), a[3]) for a in downloads] == ([] if fails else [(0x5100, n * 64)])
    assert [addr(a[1]) for a in fake.named("hfpf_device_free")][:1] == [0x5100]
    assert len(fake.named("hfpf_device_alloc")) == len(fake.named("hfpf_device_free")) == (1 if fails else 1 + (method == "query_device"))


def test_query_device_rows_and_layout(fake, grid):
    sizes = device_memory(fake)
    hits, rows = grid.query_device(0xA000, 5, POSE, radius=2)
    assert sizes == [5 * 64, 5 * H.ROW_DTYPE.itemsize]
    name, args = fake.calls[2]
    assert name == "hfpf_query_device" and args[1]._obj.radius == 2
    assert (addr(args[2]), args[3:8], doubles(args[8]), addr(args[9]), addr(args[10])) == (0xA000, (5, 12, 0, 4, 8), list(POSE.ravel()), 0x5100, 0x5200)
    assert (hits.dtype, hits.shape, rows.dtype, rows.shape) == (H.QUERY_HIT_DTYPE, (5,), H.ROW_DTYPE, (5,))
    assert [(addr(a[2]), a[3]) for a in fake.named("hfpf_device_download")] == [(0x5100, 320), (0x5200, 5 * H.ROW_DTYPE.itemsize)]
    assert [addr(a[1]) for a in fake.named("hfpf_device_free")] == [0x5100, 0x5200]
    fake.calls.clear()
    assert grid.query_device(0xA000, 0, POSE, dict(point_step=16, off_x=4, off_y=8, off_z=12), dev_hits=0xB000, dev_rows=0xC000) is None
    args = fake.calls[0][1]
    assert (args[3:8], addr(args[9]), addr(args[10])) == ((0, 16, 4, 8, 12), 0xB000, 0xC000)
    grid.query_device(0xA000, 0, POSE, dev_hits=0xB000)
    assert fake.calls[1][1][10] is None
    fake.calls.clear()
    grid.query_device(0xA000, 0, POSE)
    assert sizes[2:] == [64, H.ROW_DTYPE.itemsize]  # a scratch buffer is never empty


def test_raycast_views_device_without_views(fake, grid):
    device_memory(fake)
    got = grid.raycast_views_device(np.zeros((0, 3, 4)), K, 4, 3)
    args = fake.named("hfpf_raycast_view_device")[0]
    assert args[2:10] == (4, 3, 100.0, 101.0, 8.0, 6.0, 0, None) and got.shape == (0, 3, 4)


# ---- cloud layouts and single poses ----
CLOUD = np.arange(12, dtype=np.float32).reshape(4, 3)
RECORDS = np.zeros(5, np.dtype([("rgb", "<u4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
LAYOUT = dict(point_step=16, off_x=4, off_y=8, off_z=12, off_rgb=0)


def test_cloud_layouts(fake, grid):
    hits, rows = grid.query(CLOUD, POSE)
    args = fake.calls[0][1]
    assert (addr(args[2]), args[3:8], doubles(args[8])) == (CLOUD.ctypes.data, (4, 12, 0, 4, 8), list(POSE.ravel()))
    assert (addr(args[9]), addr(args[10])) == (hits.ctypes.data, rows.ctypes.data)
    assert (hits.dtype, hits.shape, rows.dtype, rows.shape) == (H.QUERY_HIT_DTYPE, (4,), H.ROW_DTYPE, (4,))
    hits, rows = grid.query(RECORDS, POSE, LAYOUT, rows=False)
    args = fake.calls[1][1]
    assert (addr(args[2]), args[3:8], args[10], rows, hits.shape) == (RECORDS.ctypes.data, (5, 16, 4, 8, 12), None, None, (5,))
    assert grid.query(RECORDS, POSE, LAYOUT, n_points=2)[0].shape == (2,) and fake.calls[2][1][3] == 2
    grid.query(np.arange(6.0).reshape(2, 3), POSE)  # float64 triples are packed as float32
    args = fake.calls[3][1]
    assert args[3:8] == (2, 12, 0, 4, 8) and list((C.c_float * 6).from_address(addr(args[2]))) == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    fake.calls.clear()
    grid.track(RECORDS, LAYOUT, POSE, K, 16, 12, max_iterations=4)
    args = fake.calls[0][1]
    assert (args[1]._obj.max_iterations, addr(args[2]), args[3:8], doubles(args[8])) == (4, RECORDS.ctypes.data, (5, 16, 4, 8, 12), list(POSE.ravel()))
    assert type(args[9]._obj) is H.TrackResult
    grid.track(RECORDS, LAYOUT, POSE, K, 16, 12, n_points=3)
    assert fake.calls[1][1][3] == 3


def test_poses_of_the_integrate_calls(fake, grid):
    buf = np.zeros(64, np.uint8)
    grid.integrate(buf, POSE)
    grid.integrate_pinned(buf, POSE.ravel(), n_points=2)
    for (name, args), n in zip(fake.calls, (4, 2)):
        assert (addr(args[1]), args[2:8], doubles(args[8])) == (buf.ctypes.data, (n, 16, 0, 4, 8, 12), list(POSE.ravel()))
    grid.integrate_device(0xF000, 2, 64, 4, POSES, frame_ids=[3, 4])
    args = fake.calls[2][1]
    assert (addr(args[1]), args[2:10], addr(args[10])) == (0xF000, (2, 64, 4, 16, 0, 4, 8, 12), POSES.ctypes.data)
    assert list((C.c_uint32 * 2).from_address(addr(args[11]))) == [3, 4]
    with pytest.raises(ValueError, match="cannot reshape array of size 24 into shape \\(3,12\\)"):
        grid.integrate_device(0xF000, 3, 64, 4, POSES)
    for bad in (np.zeros(11), None):
        with pytest.raises(ValueError, match="cannot reshape"):
            grid.integrate(buf, bad)
    assert len(fake.calls) == 3


# ---- the generated and shared pieces ----
def test_every_structure_knows_its_size():
    made = [H.render_opts(K, 4, 3), H.track_opts(K, 4, 3), H.query_opts(), H.mesh_opts(), H.component_opts(), H.deviation_opts(), H.align_opts(),
            H.cover_opts(), H.section_opts(), H.plan_opts(K, 4, 3), H.consistency_opts(), H.hide_opts(), H.raycast_opts(),
            H.depth_desc(16, 12, H.DEPTH_U16, 32, K), H.track_result(), H.align_result(), H._snapshot_info_struct({})]
    made += [H.track_opts(K, 4, 3).view, H.align_opts().compare, H.plan_opts(K, 4, 3).cover, H.plan_opts(K, 4, 3).view]
    assert [type(o) for o in made[:17]] == [H.RenderOpts, H.TrackOpts, H.QueryOpts, H.MeshOpts, H.ComponentOpts, H.DeviationOpts, H.AlignOpts,
                                            H.CoverOpts, H.SectionOpts, H.PlanOpts, H.ConsistencyOpts, H.HideOpts, H.RaycastOpts, H.DepthImage,
                                            H.TrackResult, H.AlignResult, H.SnapshotInfo]
    for o in made:
        assert o.struct_size == C.sizeof(type(o)) > 0


def test_hide_results(fake, grid):
    def fill(*args):
        r = args[-1]._obj
        assert (type(r), r.struct_size) == (H.HideResult, 48)
        r.n_selected, r.n_matched, r.n_changed, r.n_hidden, r.n_full = 5, 4, 3, 2, 1
        return 0
    fake.on["hfpf_hide_voxels"] = fake.on["hfpf_hide_voxels_device"] = fake.on["hfpf_hide_box"] = fill
    want = dict(n_selected=5, n_matched=4, n_changed=3, n_hidden=2, n_full=1)
    assert grid.hide_voxels(np.zeros((2, 3), np.int32)) == want
    assert grid.hide_voxels(0x111, device=True, n=2, voxel_stride=12) == want
    assert grid.hide_box((0, 0, 0), (1, 2, 3), "show") == want
    assert [n for n, _ in fake.calls] == ["hfpf_hide_voxels", "hfpf_hide_voxels_device", "hfpf_hide_box"]
    assert fake.calls[2][1][1] == H.SHOW


@pytest.mark.parametrize("kind", ("component", "deviation", "align", "cover", "section", "plan", "consistency", "hide", "raycast"))
def test_check_opts(fake, kind):
    check = getattr(H, "check_%s_opts" % kind)
    assert check.__name__ == "check_%s_opts" % kind and check.__module__ == "hfpf"
    assert check.__doc__ == "hfpf_check_%s_opts: 0 (HFPF_OK) or the error code (host code, no handle, no GPU needed)." % kind
    fake.on["hfpf_check_%s_opts" % kind] = lambda o: -2 if o is None else 0
    assert check(None) == -2
    o = getattr(H, kind + "_opts")(*((K, 4, 3) if kind == "plan" else ()))
    assert check(o) == 0
    assert [n for n, _ in fake.calls] == ["hfpf_check_%s_opts" % kind] * 2
    assert fake.calls[0][1] == (None,) and fake.calls[1][1][0]._obj is o


def test_as_dict_keys():
    coverage = ["n_tris_valid", "n_tris_invalid", "n_tris_huge", "n_samples", "n_in_bbox", "n_covered", "sum_dist_q30", "area_q40_lo", "area_q40_hi",
                "covered_q40_lo", "covered_q40_hi", "max_distance", "pad", "area", "covered_area"]
    want = {
        H.DeviationSummary: ["n_rows", "n_found", "n_negative", "n_tris_valid", "n_tris_invalid", "max_abs", "pad", "sum_abs_q30", "sum_sq_q30"],
        H.CoverageSummary: coverage,
        H.SectionSummary: ["n_tris_valid", "n_tris_invalid", "n_tris_far", "n_segments", "n_points", "n_contours", "n_closed", "reserved"],
        H.PlanSummary: ["n_views", "n_selected", "n_targets", "n_reachable", "n_planned", "target_q40", "reachable_q40", "planned_q40", "coverage"],
        H.ConsistencySummary: ["n_rows", "n_seen", "n_supported", "n_contradicted", "n_kept", "pairs_tested", "pairs_support", "pairs_through"],
        H.HideResult: ["n_selected", "n_matched", "n_changed", "n_hidden", "n_full"],
    }
    for cls, keys in want.items():
        assert list(cls().as_dict()) == keys
    s = H.PlanSummary()
    s.coverage.covered_q40_lo, s.n_planned = 1 << 39, 7
    d = s.as_dict()
    assert list(d["coverage"]) == coverage and d["coverage"]["covered_area"] == 0.5 and d["n_planned"] == 7
