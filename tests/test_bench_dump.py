"""CPU: bench.py --dump-outputs writes the extract rows and occupied cells exactly (float32 / float64), and stays under 64 MB
with a seeded sample, the same one every time, when the output is larger."""
import os
import sys

import numpy as np

import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_is_exact(tmp_path, oracle_mod, synth_mod):
    sc = scenes.Scene(3, 96, 72, 0.005, clean_every=2)
    g = oracle_mod.OracleGrid(resolution=sc.resolution, bbox=sc.bbox)
    rows = scenes.run(g, sc, "capture")
    occ = g.occupied()
    assert len(rows) > 500
    bench.dump_outputs(str(tmp_path), rows, occ)
    d = _load(str(tmp_path))
    for a in d.values():
        assert a.dtype in (np.float32, np.float64)
    assert np.array_equal(d["sizes"], [len(rows), len(occ)])
    assert np.array_equal(d["occupied_cell"], occ)
    for name, fields in (("rows_cell", ("ix", "iy", "iz")), ("rows_xyz", ("x", "y", "z")), ("rows_normal", ("nx", "ny", "nz")),
                         ("rows_sd", ("sdx", "sdy", "sdz")), ("rows_dist", ("mean_dist", "sd_dist")), ("rows_count", ("count",)),
                         ("rows_rgb", ("rgb",))):
        got = d[name].reshape(len(rows), len(fields))
        for j, f in enumerate(fields):
            assert np.array_equal(got[:, j], rows[f]), f


def test_dump_of_a_large_output_is_a_fixed_sample_under_64_mb(tmp_path):
    n, m = bench.DUMP_MAX_ROWS + 12345, bench.DUMP_MAX_CELLS + 54321
    rows = np.zeros(n, dtype=bench.hfpf.ROW_DTYPE)
    rows["ix"] = np.arange(n)
    rows["x"] = np.arange(n, dtype=np.float32) * 0.5
    occ = np.repeat(np.arange(m, dtype=np.int32)[:, None], 3, axis=1)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), rows, occ)
    total = sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a")))
    assert total <= 64 << 20
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["sizes"], [n, m])
    assert a["rows_cell"].shape == (bench.DUMP_MAX_ROWS, 3) and a["occupied_cell"].shape == (bench.DUMP_MAX_CELLS, 3)
    picked = a["rows_cell"][:, 0]
    assert np.all(np.diff(picked) > 0) and picked[-1] < n  # distinct rows, in extract order
    assert np.array_equal(a["rows_xyz"][:, 0], picked * np.float32(0.5))  # the fields of a sampled row stay together
