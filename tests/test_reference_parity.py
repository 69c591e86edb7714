"""CPU: the oracle against the COMPILED REFERENCE grid -- the reference's own OccupancyGrid.hpp ("grid.hpp"), built unmodified into
oracle/_ref/libhfpf_ref.so against the stand-in Eigen/PCL headers of oracle/ref_shim (oracle/ref_driver.cpp, `make -C oracle ref`).
Skipped where that library is absent (no reference tree to build it from).

What a green run proves: the oracle's control flow, state machine, clean order and emit rule are the reference's.  What it does not:
the Eigen/PCL leaf arithmetic is stated once (oracle/pcl_leaves.h, oracle/ref_shim/Eigen/Core) for both sides -- common mode on purpose.

Every case (tests/ref_support.py) drives OracleGrid.add_points / clean / extract / occupied / dependants and the reference driver with
the same world-frame f32 clouds, the same viewpoints and the same clean schedule.

order_mode=1 (libstdc++ bucket order, the reference's own), EVERY case, bit for bit: the occupied set; the emitted row set and order;
count; normals; x, y, z, sdx, sdy, sdz, mean_dist, sd_dist (the oracle's Welford form, exact_moments off); the set of cells that hold
a dependants list and every list, in order.  Cases (the per-resolution ones at 1 mm and at 5 mm):
  sphere_1mm sphere_5mm plane_1mm plane_5mm   synthetic captures, 6 frames, a clean pass every 2: points arrive before and after a
                                              cell's normal is found (buffered points, replay at registration, live updates)
  contest            a registration contest on an unoccupied cell: last writer wins and survives occupation
  several_normals    a cell registered by several normals
  normal_leaves_grid a normal whose +-K steps leave the grid; the grid clipped by the stencil; cells at index == dim
  count_zero         count-zero rows (at 5 mm; at 1 mm the same cloud has members: see ref_support.count_zero)
  gate_20_21         a gate of exactly 20 and of exactly 21 neighbours
  boundary_points    points on a cell boundary and on min and max of the box, with their f32 neighbours (strict compares)
  viewpoint_latch    viewpoint latched at first occupancy
  erased_key         a second addPoints on cells whose key was erased from unprocessed_data_
  random_1/2/3       4000 random points in a slab of 30 x 30 x 6 cells under three seeded clean schedules
  settled_random     random cells that are all occupied before the first pass
  dyadic_boundary    the dyadic box of tests/faces.py: points EXACTLY on cell boundaries and faces
  lattice_flat, lattice_flat_x2_further, lattice_placement_0   models of tests/lattice.py (the second has NaN normals, the third
                                              stencils at brick corners and two cells from the faces)
  crafted_full_table, crafted_pre_dependant_lists              clouds of tests/crafted.py on its two-epoch base surface
(the other clouds of crafted.py and lattice.py drive engine limits with other gates or boxes moved 128 m and more from the origin,
which state nothing further about grid.hpp; crafted.occupancy_staging's box has 10^9 cells, over the cap.)

order_mode=0 (ascending (x, y, z), the canonical order of oracle and engine): ref_support.CANONICAL_NAMES must pass
scenes.compare_rows(reference rows, oracle rows) as it stands.  The cases whose rows depend on the order of a pass are compared
under order_mode=1 only, and under order_mode=0 the deviation itself is asserted (test_order_of_a_pass_decides_only_contested_cells):
  contest, random_1, random_2, random_3 (1 mm and 5 mm)   by design: several records of one pass register on one unoccupied cell,
                                                          which is occupied later
  sphere_1mm                                              a real capture does the same: 144 of its 11,419 rows change their count
  lattice_flat_x2_further, crafted_full_table, crafted_pre_dependant_lists
                                                          layers between two sheets are registered from above and from below in
                                                          one pass and occupied in the next epoch

Inputs left out because they reach the reference's own undefined behaviour:
  NaN coordinates       validPoints passes them (all compares false, grid.hpp:644) and voxels_ is indexed with (int)floor(NaN)
                        (grid.hpp:633 -> 203); ref_support.world_cloud drops them, as oracle and engine do
  ydim >= 2048          y << 20 in int (grid.hpp:154); the driver refuses such a box
  clearVoxels           stale keys, no return (grid.hpp:167-183): never called, grids are destroyed and recreated
  a NaN NORMAL is NOT left out: its steps are NaN points that reach (int)floor(NaN) at grid.hpp:633 too, but only validCoord reads
  the result (grid.hpp:410); x86-64 converts to INT_MIN under both build settings, and the oracle restates exactly that."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import ref_support as R
import scenes

pytestmark = pytest.mark.skipif(not R.available(), reason="oracle/_ref/libhfpf_ref.so is absent (built from the reference tree by build())")

STATE_KEYS = ("occupied", "rows", "dep_cells", "dep_lengths", "dep_lists")
_runs = {}


def _frozen(st):
    for a in st.values():
        a.setflags(write=False)
    return st


def reference_state(name, path=None):
    """The reference through the case, once per (case, library); shared and read-only."""
    key = ("ref", name, path)
    if key not in _runs:
        c = R.case(name)
        g = R.drive(R.ReferenceGrid(c.resolution, c.bbox, path), c)
        _runs[key] = _frozen(R.state(g))
        g.close()
    return _runs[key]


def oracle_state(oracle_mod, name, order_mode):
    key = ("oracle", name, order_mode)
    if key not in _runs:
        c = R.case(name)
        g = R.drive(oracle_mod.OracleGrid(resolution=c.resolution, bbox=c.bbox, order_mode=order_mode), c)
        _runs[key] = _frozen(R.state(g))
        g.close()
    return _runs[key]


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, "%s: %r %r vs %r %r" % (what, a.dtype, a.shape, b.dtype, b.shape)
    if a.tobytes() != b.tobytes():
        va, vb = a.reshape(len(a), -1).view(np.uint8).reshape(len(a), -1), b.reshape(len(b), -1).view(np.uint8).reshape(len(b), -1)
        bad = np.flatnonzero((va != vb).any(axis=1))
        raise AssertionError("%s: %d of %d records differ, first at %d: %r vs %r" % (what, len(bad), len(a), bad[0], a[bad[0]], b[bad[0]]))


@pytest.mark.parametrize("name", R.NAMES)
def test_bit_for_bit_in_the_references_order(oracle_mod, synth_mod, name):
    ref, got = reference_state(name), oracle_state(oracle_mod, name, 1)
    assert len(ref["rows"]) > 0 and len(ref["dep_cells"]) > 0
    for k in STATE_KEYS:
        _same(ref[k], got[k], "%s: %s" % (name, k))


@pytest.mark.parametrize("name", R.CANONICAL_NAMES)
def test_canonical_order_passes_compare_rows(oracle_mod, synth_mod, name):
    ref, got = reference_state(name), oracle_state(oracle_mod, name, 0)
    _same(ref["occupied"], got["occupied"], "%s: occupied" % name)
    scenes.compare_rows(ref["rows"], got["rows"])


@pytest.mark.parametrize("name", R.CONTEST_NAMES)
def test_order_of_a_pass_decides_only_contested_cells(oracle_mod, synth_mod, name):
    """The documented deviation (clean order = ascending (x, y, z) instead of libstdc++ bucket order), asserted as
    what it is.  Under the canonical order the occupied set, the row set and every normal are the reference's bit for bit; the rows
    of records that hold the same registrations on occupied cells under both orders (ref_support.order_dependent_rows) are the
    reference's bytes in every column; and the case does contain what it is listed for: rows whose count the order changed."""
    ref, got = reference_state(name), oracle_state(oracle_mod, name, 0)
    _same(ref["occupied"], got["occupied"], "%s: occupied" % name)
    for f in ("ix", "iy", "iz", "nx", "ny", "nz"):
        _same(np.ascontiguousarray(ref["rows"][f]), np.ascontiguousarray(got["rows"][f]), "%s: %s" % (name, f))
    dep = R.order_dependent_rows(ref["rows"], ref, got)
    changed = ref["rows"]["count"] != got["rows"]["count"]
    print("%s: %d rows, %d with a registration on an occupied cell that depends on the order, %d with another count" % (
        name, len(dep), int(dep.sum()), int(changed.sum())))
    _same(ref["rows"][~dep], got["rows"][~dep], "%s: rows whose registrations do not depend on the order" % name)
    assert changed.any() and not (changed & ~dep).any()


def test_cases_contain_what_they_are_for(synth_mod):
    """From the reference's output alone."""
    def rows(name):
        return reference_state(name)["rows"]
    for res in ("1mm", "5mm"):
        r = rows("gate_20_21_" + res)   # 21 neighbours: one row, the plate's centre; 20: none
        assert [(int(v["ix"]), int(v["iy"]), int(v["iz"])) for v in r] == [(28, 20, 20)]
        r = rows("viewpoint_latch_" + res)
        assert (r["nz"][r["iz"] == 14] > 0.99).all() and (r["nz"][r["iz"] == 26] < -0.99).all() and len(r) == 2 * 21 * 21
        st = reference_state("normal_leaves_grid_" + res)
        n = R.SMALL_CELLS
        assert (st["occupied"] == n).any(axis=1).sum() > 3 * n, "cells at index == dim"
        # a one-cell plate's stencil is 5 x 5: clipped to 3 or 4 columns by a face (or by index == dim, which validCoord excludes) it
        # holds 15 or 20 cells and fails the gate, so the rows start two cells from every face
        r = st["rows"]
        assert (r["ix"].min(), r["ix"].max(), r["iy"].min(), r["iy"].max()) == (2, n - 3, 2, n - 3) and sorted(set(r["iz"].tolist())) == [1, n - 1]
        lists = dict(zip(map(tuple, st["dep_cells"].tolist()), st["dep_lengths"].tolist()))
        assert (20, 20, 0) in lists and (20, 20, 4) in lists and not any(c[2] >= n for c in lists), "lines cut by the faces"
        b = reference_state("boundary_points_" + res)["occupied"]
        assert (b == n).any(axis=1).sum() >= 1, "a point one f32 step inside a maximum face lies in the cell at index == dim"
        several = reference_state("several_normals_" + res)
        assert several["dep_lengths"].max() >= 3
        assert rows("sphere_" + res)["count"].max() >= 3 and rows("plane_" + res)["count"].max() >= 3
    z = rows("count_zero_5mm")
    assert len(z) == 21 * 21 and (z["count"] == 0).all()
    for f in ("x", "y", "z", "sdx", "sdy", "sdz", "mean_dist", "sd_dist"):
        assert (z[f].view(np.uint32) == 0).all(), f
    assert np.isnan(rows("lattice_flat_x2_further")["nx"]).sum() > 10


def _module(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MAKE = os.path.join(R.HERE, "golden", "make_reference_golden.py")


def test_fixtures_regenerate_identically(oracle_mod, synth_mod):
    """tests/golden/reference_*.npz are what the generator makes of today's reference library: the same arrays, byte for byte."""
    gen = _module(MAKE, "make_reference_golden")
    for fixture in gen.FIXTURES:
        path = gen.path_of(fixture)
        assert os.path.getsize(path) < gen.MAX_BYTES
        with np.load(path) as have:
            want = gen.contents(fixture)
            assert sorted(have.files) == sorted(want), fixture
            for k, v in want.items():
                v = np.asarray(v)
                assert have[k].dtype == v.dtype and have[k].shape == v.shape and have[k].tobytes() == v.tobytes(), "%s: %s" % (fixture, k)


def test_the_other_build_setting_gives_identical_bytes(oracle_mod, synth_mod, tmp_path):
    """The recipe builds with g++ -O0 because three of the reference's bool functions fall off their ends; clang++ -O2
    -fno-strict-return is the other setting under which that is well-behaved (oracle/Makefile says why neither changes a value).
    Both builds give the same bytes on every case, the fixtures' among them."""
    clang = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    inc = os.path.join(R.REFERENCE_TREE, "pointcloud_fusion", "pointcloud_fusion", "include", "utilities", "OccupancyGrid.hpp")
    if not os.path.exists(clang) or not os.path.exists(inc):
        pytest.skip("needs clang++ and the reference tree")
    out = str(tmp_path / "libhfpf_ref_clang.so")
    subprocess.check_call(["make", "-s", "-C", os.path.join(R.ROOT, "oracle"), "ref", "REF_CXX=" + clang, "REF_OPT=-O2 -fno-strict-return",
                           "REF_OUT=" + out, "HFPF_REFERENCE=" + R.REFERENCE_TREE])
    for name in R.NAMES:
        a, b = reference_state(name), reference_state(name, out)
        for k in STATE_KEYS:
            _same(a[k], b[k], "%s: %s (g++ -O0 vs clang++ -O2 -fno-strict-return)" % (name, k))
