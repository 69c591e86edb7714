"""CPU: the connected-components contract as tests/components_ref.py states it, on hand-built rows whose answer is known, on the
oracle's rows of a golden scene, and the host-side option check of the library."""
import importlib.util
import os

import numpy as np
import pytest

import components_ref as CR
import scenes

HERE = os.path.dirname(os.path.abspath(__file__))


def _rows(cells, normals=(0.0, 0.0, 1.0), counts=5):
    """hfpf_row records of the given cells in lexicographic order; normals and counts are one value or one per cell (as given)."""
    cells = np.asarray(cells, np.int32).reshape(-1, 3)
    n = len(cells)
    normals = np.broadcast_to(np.asarray(normals, np.float32), (n, 3))
    counts = np.broadcast_to(np.asarray(counts, np.uint32), (n,))
    order = np.lexsort((cells[:, 2], cells[:, 1], cells[:, 0]))
    rows = np.zeros(n, CR.ROW_DTYPE)
    rows["ix"], rows["iy"], rows["iz"] = cells[order].T
    rows["nx"], rows["ny"], rows["nz"] = normals[order].T
    rows["count"] = counts[order]
    rows["x"], rows["y"], rows["z"] = (cells[order].astype(np.float32) * np.float32(0.002)).T
    return rows


def _slab(x0, x1, y0, y1, z):
    return [(x, y, z) for x in range(x0, x1) for y in range(y0, y1)]


def _cube_faces(n=8, o=10):
    """The six faces of a cube of n^3 cells at offset o, every cell with the outward normal of its face; the 12 edges (cells on two or
    three faces) are left out, so a face's cells touch the next face's cells only diagonally."""
    cells, normals = [], []
    for axis in range(3):
        for side, sign in ((0, -1.0), (n - 1, 1.0)):
            for u in range(1, n - 1):
                for v in range(1, n - 1):
                    c = [0, 0, 0]
                    c[axis] = side
                    c[(axis + 1) % 3], c[(axis + 2) % 3] = u, v
                    nrm = [0.0, 0.0, 0.0]
                    nrm[axis] = sign
                    cells.append([o + k for k in c])
                    normals.append(nrm)
    return _rows(cells, normals)


def _check_invariants(rows_in, out, **opt):
    rows, labels, comps = out
    assert rows.dtype == CR.ROW_DTYPE and labels.dtype == np.uint32 and comps.dtype == CR.COMPONENT_DTYPE
    assert len(rows) == len(labels) and int(comps["n_rows"].sum()) == len(rows)
    if len(rows) == 0:
        return
    assert labels.max() == len(comps) - 1 and len(np.unique(labels)) == len(comps)
    first = np.array([np.flatnonzero(labels == c)[0] for c in range(len(comps))])
    assert np.array_equal(first, comps["first_row"]), "first_row is the first (smallest) output row of its component"
    assert (np.diff(first) > 0).all(), "components are numbered by ascending representative"
    gated = rows_in[CR.count_gate(rows_in, opt.get("min_count", 0.0))]
    assert rows[first].tobytes() == gated[comps["source_row"]].tobytes(), "source_row names the same row in the unfiltered row set"
    for c in range(len(comps)):
        mine = rows[labels == c]
        assert comps["n_rows"][c] == len(mine) and comps["points"][c] == mine["count"].astype(np.uint64).sum()
        assert np.array_equal(comps["lo"][c], [mine[f].min() for f in ("ix", "iy", "iz")])
        assert np.array_equal(comps["hi"][c], [mine[f].max() for f in ("ix", "iy", "iz")])
    assert not comps["reserved"].any()


def test_two_slabs_one_empty_voxel_apart():
    rows = _rows(_slab(0, 6, 0, 6, 3) + _slab(0, 6, 0, 6, 5))  # z = 4 is empty
    out1 = CR.components(rows, reach=1)
    assert len(out1[2]) == 2 and list(out1[2]["n_rows"]) == [36, 36]
    _check_invariants(rows, out1)
    out2 = CR.components(rows, reach=2)
    assert len(out2[2]) == 1 and out2[2]["n_rows"][0] == 72 and not out2[1].any()
    _check_invariants(rows, out2)
    assert out1[0].tobytes() == rows.tobytes() and out2[0].tobytes() == rows.tobytes()


def test_cube_faces_split_by_the_normal_gate():
    rows = _cube_faces()
    one = CR.components(rows, reach=1, min_normal_dot=-2.0)
    assert len(one[2]) == 1 and one[2]["n_rows"][0] == len(rows)
    six = CR.components(rows, reach=1, min_normal_dot=0.5)
    assert len(six[2]) == 6 and (six[2]["n_rows"] == 36).all()
    _check_invariants(rows, six, min_normal_dot=0.5)
    for c in range(6):  # a component is one face: one normal
        mine = six[0][six[1] == c]
        assert len(np.unique(np.stack([mine["nx"], mine["ny"], mine["nz"]], axis=1), axis=0)) == 1


def test_a_nan_normal_joins_nothing():
    rows = _rows(_slab(0, 3, 0, 3, 0))
    rows["nx"][4] = np.nan  # the centre cell
    out = CR.components(rows, reach=1, min_normal_dot=-2.0)
    assert len(out[2]) == 2 and sorted(out[2]["n_rows"]) == [1, 8]


def test_keep_largest_breaks_ties_by_representative():
    # four islands along x: sizes 4, 9, 9, 9
    cells = _slab(0, 2, 0, 2, 0) + _slab(10, 13, 0, 3, 0) + _slab(20, 23, 0, 3, 0) + _slab(30, 33, 0, 3, 0)
    rows = _rows(cells)
    allc = CR.components(rows)
    assert list(allc[2]["n_rows"]) == [4, 9, 9, 9]
    two = CR.components(rows, keep_largest=2)
    assert list(two[2]["source_row"]) == [4, 13] and list(two[2]["first_row"]) == [0, 9]
    assert (two[0]["ix"] < 23).all() and (two[0]["ix"] >= 10).all()
    _check_invariants(rows, two)
    assert len(CR.components(rows, keep_largest=4)[2]) == 4 and len(CR.components(rows, keep_largest=9)[2]) == 4
    # the rank counts only components that pass the other tests: min_rows = 5 leaves the three nines, of which the first one is kept
    one = CR.components(rows, keep_largest=1, min_rows=5)
    assert list(one[2]["source_row"]) == [4]


def test_min_rows_and_min_points_drop_the_expected_components():
    cells = _slab(0, 2, 0, 2, 0) + _slab(10, 13, 0, 3, 0) + _slab(20, 24, 0, 4, 0)
    counts = [100] * 4 + [1] * 9 + [2] * 16   # points: 400, 9, 32
    rows = _rows(cells, counts=counts)
    assert list(CR.components(rows)[2]["points"]) == [400, 9, 32]
    big = CR.components(rows, min_rows=5)
    assert list(big[2]["n_rows"]) == [9, 16] and list(big[2]["source_row"]) == [4, 13] and list(big[2]["first_row"]) == [0, 9]
    _check_invariants(rows, big)
    rich = CR.components(rows, min_points=10)
    assert list(rich[2]["points"]) == [400, 32] and len(rich[0]) == 20
    _check_invariants(rows, rich)
    both = CR.components(rows, min_rows=5, min_points=10)
    assert list(both[2]["n_rows"]) == [16] and both[0].tobytes() == rows[13:].tobytes() and not both[1].any()
    assert len(CR.components(rows, min_rows=17)[0]) == 0


def test_min_count_drops_rows_before_the_labelling():
    # a bridge of low-count cells joins two slabs: with the gate the bridge is gone and the slabs are apart
    cells = _slab(0, 3, 0, 3, 0) + [(3, 1, 0), (4, 1, 0)] + _slab(5, 8, 0, 3, 0)
    counts = [10] * 9 + [1, 2] + [10] * 9
    rows = _rows(cells, counts=counts)
    assert len(CR.components(rows)[2]) == 1
    out = CR.components(rows, min_count=3.0)
    assert len(out[2]) == 2 and len(out[0]) == 18 and (out[0]["count"] == 10).all()
    _check_invariants(rows, out, min_count=3.0)
    assert len(CR.components(rows, min_count=2.0)[0]) == 19  # count < min_count is dropped: 2 stays


def test_every_label_names_the_smallest_row_of_its_component():
    rng = np.random.default_rng(0xC0)
    cells = np.unique(rng.integers(0, 24, (700, 3)), axis=0)
    normals = rng.normal(size=(len(cells), 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    rows = _rows(cells, normals, rng.integers(0, 50, len(cells)))
    for opt in (dict(reach=1), dict(reach=2, min_normal_dot=0.0), dict(reach=1, min_normal_dot=0.3, min_count=10.0)):
        out = CR.components(rows, **opt)
        _check_invariants(rows, out, **opt)
        # brute force: flood fill over the pair list
        gated = rows[CR.count_gate(rows, opt.get("min_count", 0.0))]
        a, b = CR.neighbour_pairs(gated, opt["reach"])
        ok = CR.normal_gate(gated, a, b, opt.get("min_normal_dot", -2.0))
        adj = [[] for _ in range(len(gated))]
        for x, y in zip(a[ok], b[ok]):
            adj[x].append(y), adj[y].append(x)
        seen = np.full(len(gated), -1)
        for s in range(len(gated)):
            if seen[s] >= 0:
                continue
            seen[s] = s
            stack = [s]
            while stack:
                for y in adj[stack.pop()]:
                    if seen[y] < 0:
                        seen[y] = s
                        stack.append(y)
        assert np.array_equal(out[2]["source_row"][out[1]], seen), opt
        assert 3 < len(out[2]) < len(gated), "the case should hold both joined and separate rows"


def test_no_rows_give_empty_outputs():
    for rows in (np.zeros(0, CR.ROW_DTYPE), _rows([(1, 2, 3)], counts=1)):
        out = CR.components(rows, min_count=2.0)
        assert len(out[0]) == 0 and len(out[1]) == 0 and len(out[2]) == 0
        assert out[0].dtype == CR.ROW_DTYPE and out[1].dtype == np.uint32 and out[2].dtype == CR.COMPONENT_DTYPE


def test_oracle_rows_of_a_golden_scene(oracle_mod, synth_mod):
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    make_golden = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make_golden)
    gold = np.load(os.path.join(HERE, "golden", "scenes.npz"))
    name = sorted(make_golden.SCENES)[0]
    sc = scenes.Scene(**make_golden.SCENES[name])
    g = oracle_mod.OracleGrid(resolution=sc.resolution, bbox=sc.bbox)
    rows = np.ascontiguousarray(scenes.run(g, sc, "capture"))
    assert rows.tobytes() == gold[name + "__rows"].tobytes() and len(rows) > 100
    rows = rows.view(CR.ROW_DTYPE).reshape(-1)
    for reach in (1, 2):
        out = CR.components(rows, reach=reach)
        assert out[0].tobytes() == rows.tobytes(), "with every filter off the rows are all rows"
        assert len(out[1]) == len(rows) and int(out[2]["n_rows"].sum()) == len(rows)
        _check_invariants(rows, out)
        print("%s, reach %d: %d rows in %d components, largest %d" % (name, reach, len(rows), len(out[2]), out[2]["n_rows"].max()))


def test_the_library_checks_component_options(hfpf_mod):
    H = hfpf_mod
    assert H.COMPONENT_DTYPE == CR.COMPONENT_DTYPE and H.ROW_DTYPE == CR.ROW_DTYPE
    assert H.check_component_opts(H.component_opts()) == 0
    assert H.check_component_opts(H.component_opts(reach=4, min_count=3.0, min_normal_dot=1.0, min_rows=7, min_points=1 << 40, keep_largest=2)) == 0
    assert H.check_component_opts(None) == -2
    nan, inf = float("nan"), float("inf")
    bad = [("struct_size", 48), ("flags", 1), ("reserved0", 1), ("reserved", 1), ("reach", 0), ("reach", 5), ("reach", -1), ("min_count", nan),
           ("min_normal_dot", nan), ("min_normal_dot", -inf), ("min_normal_dot", inf), ("min_normal_dot", -2.5), ("min_normal_dot", 1.5)]
    for field, val in bad:
        o = H.component_opts()
        setattr(o, field, val)
        assert H.check_component_opts(o) == -2, (field, val)
