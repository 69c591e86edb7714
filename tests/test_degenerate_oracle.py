"""CPU: the lattice models of tests/lattice.py on the oracle alone.  What is asserted here keeps the GPU tests of
test_gpu_degenerate.py from passing vacuously: the models really produce rows with a NaN normal, rows with a zero normal and rows
whose normal is the patch's own, where they are said to and nowhere else.  The counts are printed."""
import numpy as np
import pytest

import faces
import lattice as L


def _rows(oracle_mod, model, upto=None):
    og = oracle_mod.OracleGrid(resolution=model.resolution, bbox=model.bbox, **model.config)
    assert og.dims[0] == L.DIMS
    model.run(og, "capture", upto)
    rows = og.extract()
    og.close()
    n, n_nan, n_zero, big = L.normal_counts(rows)
    print("%s: %d rows, %d with a NaN normal (%s), %d with a zero normal, %r with |n_axis| > 0.99" % (
        model.name, n, n_nan, ", ".join(L.nan_patterns(rows)) or "-", n_zero, big))
    odd = L.nan_mask(rows) | L.zero_mask(rows)
    assert (rows["count"][odd] == 0).all(), "%s: a row with a NaN or zero normal has members" % model.name
    nan_any = L.nan_mask(rows)
    nan_all = np.isnan(rows["nx"]) & np.isnan(rows["ny"]) & np.isnan(rows["nz"])
    assert np.array_equal(nan_any, nan_all), "%s: a normal with NaN in some components only" % model.name
    return rows, n_nan, n_zero, big


def test_flat_patch_near_the_origin_has_the_patch_normal(oracle_mod):
    for axis in (2, 0):
        rows, n_nan, n_zero, big = _rows(oracle_mod, L.flat_model(axis=axis))
        assert len(rows) == 44 * 44 and n_nan == 0 and n_zero == 0 and big[axis] == len(rows)


def test_flat_patch_at_128_m_has_nan_and_patch_normals(oracle_mod):
    rows, n_nan, n_zero, big = _rows(oracle_mod, L.flat_model(faces.SHIFT_128))
    assert len(rows) == 44 * 44 and n_nan >= 20 and big[2] >= 20 and n_zero == 0


def test_flat_patch_at_1024_m_has_nan_normals(oracle_mod):
    rows, n_nan, n_zero, big = _rows(oracle_mod, L.flat_model(faces.SHIFT_1024))
    assert len(rows) == 44 * 44 and n_nan >= 10 and n_zero == 0


@pytest.mark.parametrize("shift", [faces.SHIFT_128, faces.SHIFT_1024], ids=["128", "1024"])
def test_shifted_covariance_has_neither(oracle_mod, shift):
    rows, n_nan, n_zero, big = _rows(oracle_mod, L.flat_model(shift, shifted_cov=True))
    assert len(rows) == 44 * 44 and n_nan == 0 and n_zero == 0 and big[2] == len(rows)


@pytest.mark.parametrize("further", [False, True], ids=["two epochs", "further layer"])
def test_every_flat_model_keeps_to_its_size(oracle_mod, further):
    """The other flat models of the GPU test: their counts for the ledger, and the sizes that keep a test to seconds."""
    for shift in ((0.0, 0.0, 0.0), faces.SHIFT_128, faces.SHIFT_1024):
        for axis in (2, 0):
            for layers in (1, 2):
                m = L.flat_model(shift, axis, layers, further=further)
                rows = _rows(oracle_mod, m)[0]
                assert len(rows) <= 5000 and m.max_points <= 12000


def test_low_gates_have_zero_and_nan_normals(oracle_mod):
    got = {}
    for gate in (0, 1, 2, 4):
        rows, n_nan, n_zero, _ = _rows(oracle_mod, L.low_gate_model(gate))
        got[gate] = (len(rows), n_nan, n_zero)
    assert got[0][2] >= 10 and got[0][1] >= 50, got
    # gate: total > gate.  A single cell (total 1) passes gate 0 alone, a cell of a pair (total 2) gates 0 and 1: no fit, zero normal
    assert got[0][2] == L.LOW_GATE_SINGLES + 2 * L.LOW_GATE_PAIRS and got[1][2] == 2 * L.LOW_GATE_PAIRS, got
    assert got[2][2] == 0 and got[4][2] == 0 and got[2][1] >= 50 and got[4][1] >= 10, got


def test_placement_models(oracle_mod):
    cells, centres = L.placement_cells()
    assert len(centres) == 9 * len(L.GATE20) and len(L.GATE20) == 14
    for fam in L.GATE20:
        local = {tuple(v % 8 for v in c) for f, c in centres[:8 * len(L.GATE20)] if f == fam}
        assert local == {(a, b, c) for a in (0, 7) for b in (0, 7) for c in (0, 7)}, "%s: centres at %r" % (fam, sorted(local))
        face = [c for f, c in centres[8 * len(L.GATE20):] if f == fam]
        assert len(face) == 1 and face[0][1] == L.DIMS[1] - 3
    total_nan = 0
    for part in range(L.PLACEMENT_PARTS):
        for further in (False, True):
            m = L.placement_model(part, further=further)
            rows, n_nan, _, _ = _rows(oracle_mod, m)
            assert 0 < len(rows) <= 5000 and m.max_points <= 12000
            total_nan += n_nan
    assert total_nan >= 10


def test_stencil_families_and_canonical_nans():
    sizes = {k: int(m.sum()) for k, m in L.FAMILIES.items()}
    assert sizes == dict(single=1, pair=2, line_x=5, line_y=5, line_z=5, line_diag=5, plane_x0=25, plane_y0=25, plane_z0=25, plane_xy=25,
                         plane_xyz=19, slab2=50, slab3=75, planes_z2=50, half=75, octant=27, cross=45, corner=61, shell=98, checker=63,
                         cube=125), sizes
    hollow = [k for k, m in L.FAMILIES.items() if not m[62]]
    assert hollow == ["planes_z2", "shell"], "the families without their centre cell: %r" % hollow
    assert L.FAMILIES["line_x"].reshape(5, 5, 5)[:, 2, 2].all() and L.FAMILIES["line_z"].reshape(5, 5, 5)[2, 2, :].all(), "setK order: x outermost"
    import oracle
    rows = np.zeros(4, oracle.ROW_DTYPE)
    rows["nx"] = np.array([0xFFC00000, 0x7FC00001, 0x3F800000, 0], np.uint32).view(np.float32)
    rows["ny"][0] = np.nan
    out = L.canonical_nans(rows)
    assert out["nx"].view(np.uint32).tolist() == [L.QUIET_NAN, L.QUIET_NAN, 0x3F800000, 0] and out["ny"].view(np.uint32)[0] == L.QUIET_NAN
    assert rows["nx"].view(np.uint32)[0] == 0xFFC00000, "the input is left alone"
    assert L.nan_mask(rows).tolist() == [True, True, False, False] and L.zero_mask(rows).tolist() == [False, False, False, True]
    assert L.nan_patterns(rows) == ["0x7FC00000", "0x7FC00001", "0xFFC00000"]


@pytest.mark.parametrize("shifted", [False, True], ids=["default", "shifted"])
@pytest.mark.parametrize("box", list(L.LEAF_BOXES))
def test_leaf_inputs_contain_nan_zero_and_clipped_results(oracle_mod, box, shifted):
    """What the leaf test of test_gpu_degenerate.py relies on, on the oracle alone: every box and covariance form gives NaN results,
    zero results (totals 0, 1 and 2 among them) and stencils that the grid's faces clip."""
    res, bbox = L.LEAF_BOXES[box]
    og = oracle_mod.OracleGrid(resolution=res, bbox=bbox, pcl_shifted_cov=shifted)
    names, cells, occ, vps = L.leaf_inputs(og.dims[0], bbox, og.probe_center)
    assert len(cells) == L.LEAF_PER_FAMILY * len(L.FAMILIES) + L.LEAF_EMPTY <= 10000
    totals, normals = L.leaf_reference(og, cells, occ, vps)
    og.close()
    nan = np.isnan(normals).any(axis=1)
    zero = (normals == 0).all(axis=1)
    clipped = totals < occ.sum(axis=1)
    per_family = {f: int(nan[names == f].sum()) for f in L.FAMILIES if nan[names == f].any()}
    print("%s, %s: %d probes, %d NaN %r, %d zero, %d clipped, totals below 3: %r" % (
        box, "shifted" if shifted else "default", len(cells), nan.sum(), per_family, zero.sum(), clipped.sum(), [int((totals == t).sum()) for t in (0, 1, 2)]))
    assert np.array_equal(nan, np.isnan(normals).all(axis=1)), "a result with NaN in some components only"
    assert np.array_equal(zero, totals < 3), "exactly the stencils with fewer than three cells keep the zero normal"
    assert nan.sum() >= 20 and zero.sum() >= 2 * L.LEAF_PER_FAMILY and clipped.sum() >= 500
    assert all((totals == t).any() for t in (0, 1, 2)), "totals of 0, 1 and 2"
