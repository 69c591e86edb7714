"""What the Python binding hands to hfpf_mesh_topology* and what it makes of the results, seen by a fake library that records every
call (the pattern of tests/test_binding_marshal.py).  No GPU and no libhfpf.so: the grid is made without hfpf_create, and the fake fills
the outputs through byref(...)._obj with arrays from libc's malloc, as the engine does.  Every expectation is written out by hand."""
import ctypes as C

import numpy as np
import pytest

import hfpf as H

libc = C.CDLL(None)
libc.malloc.restype = C.c_void_p
libc.malloc.argtypes = [C.c_size_t]
libc.free.argtypes = [C.c_void_p]

IDENTITY = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
POSE = np.arange(12, dtype=np.float64).reshape(3, 4) + 0.5
V4 = np.arange(12, dtype=np.float32).reshape(4, 3)
T2 = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
VR = np.zeros(4, H.MESH_VERTEX_DTYPE)


class FakeLib:
    """Stands in for hfpf.lib().  calls: (name, args) of every call, in order; on[name](*args) fills the outputs and gives the return
    code (0 without one)."""

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
        p = libc.malloc(max(a.nbytes, 1))
        C.memmove(p, a.ctypes.data, a.nbytes)
        self.blocks.append(p)
        return p


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
    return None if arg is None else arg.value


def rec(dtype, n, seed):
    dtype = np.dtype(dtype)
    return ((np.arange(n * dtype.itemsize) + seed) % 251).astype(np.uint8).view(dtype)


EDGES, LOOPS, SHELLS, PER_TRI = rec(H.TOPOLOGY_EDGE_DTYPE, 3, 1), rec(H.TOPOLOGY_LOOP_DTYPE, 2, 2), rec(H.TOPOLOGY_SHELL_DTYPE, 1, 3), rec(np.uint32, 2, 4)


def hand_out(fake, name):
    """Let `name` hand out the four arrays (tri_shell only where the caller passed a pointer), the counts and a summary."""
    given = {}

    def fill(*args):
        for i, a in ((8, EDGES), (10, LOOPS), (12, SHELLS), (14, PER_TRI)):
            if args[i] is not None:
                given[i] = args[i]._obj.value = fake.give(a)
        for i, n in ((9, 3), (11, 2), (13, 1)):
            args[i]._obj.value = n
        args[15]._obj.n_boundary, args[15]._obj.n_shells = 3, 1
        return 0
    fake.on[name] = fill
    return given


def test_the_structures_know_their_sizes():
    o = H.topology_opts()
    assert (type(o), o.struct_size, o.flags, o.reserved) == (H.TopologyOpts, 16, 0, 0) and C.sizeof(H.TopologySummary) == 128
    assert (H.TOPOLOGY_EDGE_DTYPE.itemsize, H.TOPOLOGY_LOOP_DTYPE.itemsize, H.TOPOLOGY_SHELL_DTYPE.itemsize) == (32, 64, 64)
    assert H.TOPOLOGY_LOOP_DTYPE.fields["length_q32"][1] == 24 and H.TOPOLOGY_LOOP_DTYPE.fields["area_q28"][1] == 32
    assert H.TOPOLOGY_SHELL_DTYPE.fields["area_q32"][1] == 40 and H.TOPOLOGY_SHELL_DTYPE.fields["volume_q40"][1] == 48
    assert list(H.TopologySummary().as_dict()) == ["n_tris_valid", "n_tris_invalid", "n_tris_far", "n_verts_used", "n_edges", "n_interior", "n_boundary",
                                                   "n_nonmanifold", "n_miswound", "n_loops", "n_closed_loops", "n_shells", "n_watertight"]
    assert (H.TOPOLOGY_BOUNDARY, H.TOPOLOGY_NONMANIFOLD, H.TOPOLOGY_MISWOUND, H.TOPOLOGY_NONE) == (1, 2, 3, 0xFFFFFFFF)
    assert (H.TOPOLOGY_LOOP_CLOSED, H.TOPOLOGY_LOOP_BRANCHED) == (1, 2)
    assert (H.TOPOLOGY_SHELL_OPEN, H.TOPOLOGY_SHELL_NONMANIFOLD, H.TOPOLOGY_SHELL_MISWOUND, H.TOPOLOGY_SHELL_WATERTIGHT) == (1, 2, 4, 8)
    for name in ("hfpf_check_topology_opts", "hfpf_mesh_topology", "hfpf_mesh_topology_device", "hfpf_free_topology"):
        assert name in H.EXPORTS


def test_mesh_arguments_and_pose(fake, grid):
    grid.mesh_topology(V4, T2)
    name, args = fake.calls[0]
    assert name == "hfpf_mesh_topology" and args[0] is grid._h and len(args) == 16
    o = args[1]._obj
    assert (type(o), o.struct_size) == (H.TopologyOpts, 16)
    assert (addr(args[2]), args[3], args[4], addr(args[5]), args[6]) == (V4.ctypes.data, 4, 12, T2.ctypes.data, 2)
    assert list((C.c_double * 12).from_address(args[7].value)) == IDENTITY
    assert type(args[15]._obj) is H.TopologySummary and all(a is not None for a in args[8:15])
    fake.calls.clear()
    grid.mesh_topology(VR, T2, pose=POSE, n_tris=1)
    args = fake.calls[0][1]
    assert (addr(args[2]), args[3], args[4], args[6]) == (VR.ctypes.data, 4, 32, 1)
    assert list((C.c_double * 12).from_address(args[7].value)) == [0.5 + i for i in range(12)]
    fake.calls.clear()
    mine = H.topology_opts()
    grid.mesh_topology(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32), opts=mine)
    args = fake.calls[0][1]
    assert args[1]._obj is mine and (args[2], args[3], args[5], args[6]) == (None, 0, None, 0)


@pytest.mark.parametrize("tri_shell", (True, False))
def test_results_are_copied_out_and_freed_once(fake, grid, tri_shell):
    given = hand_out(fake, "hfpf_mesh_topology")
    edges, loops, shells, per_tri, summary = grid.mesh_topology(V4, T2, tri_shell=tri_shell)
    assert (fake.calls[0][1][14] is None) == (not tri_shell)
    for got, want in ((edges, EDGES), (loops, LOOPS), (shells, SHELLS)):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    if tri_shell:
        assert per_tri.dtype == np.uint32 and per_tri.tobytes() == PER_TRI.tobytes()  # one word per triangle: n_tris of them
    else:
        assert per_tri is None
    assert (summary["n_boundary"], summary["n_shells"], summary["n_edges"]) == (3, 1, 0) and "reserved" not in summary
    frees = fake.named("hfpf_free_topology")
    assert len(frees) == 1 and tuple(addr(a) for a in frees[0]) == (given[8], given[10], given[12], given.get(14))


def test_nothing_to_copy_still_frees_once_and_a_failed_call_frees_nothing(fake, grid):
    edges, loops, shells, per_tri, _ = grid.mesh_topology(V4, T2)
    assert (edges.shape, loops.shape, shells.shape, per_tri.shape) == ((0,), (0,), (0,), (0,))
    assert (edges.dtype, loops.dtype, shells.dtype) == (H.TOPOLOGY_EDGE_DTYPE, H.TOPOLOGY_LOOP_DTYPE, H.TOPOLOGY_SHELL_DTYPE)
    assert [tuple(addr(a) for a in c) for c in fake.named("hfpf_free_topology")] == [(None, None, None, None)]
    fake.calls.clear()
    fake.on["hfpf_mesh_topology"] = lambda *a: -2
    with pytest.raises(H.HfpfError, match="BAD_ARG.*fake") as e:
        grid.mesh_topology(V4, T2)
    assert e.value.code == -2 and fake.named("hfpf_free_topology") == []


def test_the_device_alias(fake, grid):
    given = hand_out(fake, "hfpf_mesh_topology_device")
    out = grid.mesh_topology_device(0x7000, 4, 32, 0x8000, 2, POSE)
    name, args = fake.calls[0]
    assert name == "hfpf_mesh_topology_device" and len(fake.calls) == 1, "nothing is copied and nothing is freed"
    assert (addr(args[2]), args[3], args[4], addr(args[5]), args[6]) == (0x7000, 4, 32, 0x8000, 2)
    assert all(type(args[i]) is int for i in (3, 4, 6))
    assert out[:4] == ((given[8], 3), (given[10], 2), (given[12], 1), given[14]) and out[4]["n_boundary"] == 3
    fake.calls.clear()
    out = grid.mesh_topology_device(0x7000, 4, 32, 0x8000, 2, tri_shell=False)
    assert fake.calls[0][1][14] is None and out[3] == 0
    del fake.on["hfpf_mesh_topology_device"]
    assert grid.mesh_topology(0x7000, 0x8000, device=True, n_verts=4, vertex_stride=12, n_tris=2)[:4] == ((0, 0), (0, 0), (0, 0), 0)


def test_check_topology_opts(fake):
    assert H.check_topology_opts.__name__ == "check_topology_opts"
    fake.on["hfpf_check_topology_opts"] = lambda o: -2 if o is None else 0
    o = H.topology_opts()
    assert H.check_topology_opts(None) == -2 and H.check_topology_opts(o) == 0
    assert fake.calls[0][1] == (None,) and fake.calls[1][1][0]._obj is o
