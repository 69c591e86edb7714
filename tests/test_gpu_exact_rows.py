"""GPU: the engine's rows against the oracle's exact rows (exact_moments=True: the same integer words, the same f64 row expression,
tests/test_stats_ref.py) -- fourteen columns byte for byte, mean_dist / sd_dist within the bound derived in
scenes.compare_rows_exact from the one thing a CPU cannot reproduce, the hardware square root.  Every update form, scale set and
read-out that makes or reads the statistic words is driven once; scenes.compare_rows (the agreement with the reference's
recurrence) is asserted beside it, unchanged."""
import numpy as np
import pytest

import scenes
from gpu_support import IDENT, SMALL_CAPS, run_virtual
from stats_ref import STRADDLE_SCENE

pytestmark = pytest.mark.gpu

_oracle_cache = {}


def _oracle(oracle_mod, sc, key, **cfg):
    """(Welford rows, exact rows, moment records) of a scene, computed once per key and never modified."""
    if key not in _oracle_cache:
        og = oracle_mod.OracleGrid(resolution=sc.resolution, bbox=sc.bbox, exact_moments=True, **cfg)
        ref = scenes.run(og, sc, "capture", color=bool(cfg.get("fuse_color")))
        out = (ref, og.extract_exact(), og.moments())
        og.close()
        for a in out:
            a.setflags(write=False)
        _oracle_cache[key] = out
    return _oracle_cache[key]


def _check(oracle_mod, hfpf_mod, sc, key, engine_kw=None, **cfg):
    ref, exact, mom = _oracle(oracle_mod, sc, key, **cfg)
    with hfpf_mod.OccupancyGrid(resolution=sc.resolution, bbox=sc.bbox, **cfg, **(engine_kw or {}), **SMALL_CAPS) as eg:
        got = scenes.run(eg, sc, "integrate")
    scenes.compare_rows(ref, got)
    rep = scenes.compare_rows_exact(exact, got, cylinder_radius=cfg.get("cylinder_radius", 0.001))
    assert rep["exact_bytes_differing"] == 0
    return exact, got


FORMS_SCENE = dict(n_frames=7, W=160, H=120, resolution=0.001, fx=615.0, clean_every=2)  # the scene of the forced-form tests


def _forms_scene():
    return scenes.Scene(**FORMS_SCENE)


@pytest.mark.parametrize("res,W,H,fx,nf,ce", [
    (0.005, 160, 120, 0.0, 6, 3),
    (0.001, 160, 120, 615.0, 6, 3),
    (0.001, 160, 120, 615.0, 5, 1),    # clean after every frame: members arrive through replay and at integrate time
    (0.0005, 128, 96, 1968.0, 4, 2),
])
def test_stream_shapes(oracle_mod, hfpf_mod, synth_mod, res, W, H, fx, nf, ce):
    sc = scenes.Scene(nf, W, H, res, fx=fx, clean_every=ce)
    exact, got = _check(oracle_mod, hfpf_mod, sc, ("stream", res, W, nf, ce))
    assert len(got) > 100


def test_clean_only_at_the_end(oracle_mod, hfpf_mod, synth_mod):
    """No clean pass until every frame is in: every member arrives through the replay of buffered points."""
    sc = scenes.Scene(5, 160, 120, 0.001, fx=615.0, clean_every=0)
    exact, got = _check(oracle_mod, hfpf_mod, sc, "clean_at_end")
    assert got["count"].sum() > 10000


@pytest.mark.parametrize("which", ["dense", "coarse"])
def test_many_members_per_voxel(oracle_mod, hfpf_mod, synth_mod, which):
    """Words far beyond 32 bits.  dense: 2 cm voxels with 1 cm cylinders, more than 10,000 members in one voxel; coarse: the 2 cm
    scene of test_gpu_edge with the same cylinders under a zoomed camera (above 4096)."""
    if which == "dense":
        sc, cfg = scenes.dense_scene()
    else:
        sc, cfg = scenes.Scene(8, 160, 120, 0.02, fx=615.0, clean_every=1), dict(cylinder_radius=0.01)
    exact, got = _check(oracle_mod, hfpf_mod, sc, ("many", which), **cfg)
    assert exact["count"].max() >= 4096 and (exact["count"] == 0).any()
    m = _oracle(oracle_mod, sc, ("many", which))[2]["m"]
    assert np.abs(m[:, 1:5]).max(axis=0).min() > 1 << 32 and (m[:, 1] < 0).any()


K, RES, BALL_BELOW, BALL_ABOVE, _ = STRADDLE_SCENE


@pytest.mark.parametrize("cfg", [
    dict(K=1), dict(K=5), dict(cylinder_radius=0.0005), dict(cylinder_radius=0.003, ball_radius=0.03),
    dict(K=K, ball_radius=BALL_BELOW), dict(K=K, ball_radius=BALL_ABOVE),  # Bm on either side of 2^-2: fs differs by a factor two
    dict(pcl_shifted_cov=True),
], ids=["K1", "K5", "cyl0.5mm", "cyl3mm_ball30mm", "below_pow2", "above_pow2", "shifted_cov"])
def test_non_default_scales(oracle_mod, hfpf_mod, synth_mod, cfg):
    sc = scenes.Scene(5, 160, 120, 0.001, fx=615.0, clean_every=2)
    exact, got = _check(oracle_mod, hfpf_mod, sc, ("cfg", tuple(sorted(cfg.items()))), **cfg)
    assert len(got) > 50


def test_colour(oracle_mod, hfpf_mod, synth_mod):
    sc = scenes.Scene(5, 160, 120, 0.001, fx=615.0, clean_every=2)
    exact, got = _check(oracle_mod, hfpf_mod, sc, "colour", fuse_color=True)
    assert len(np.unique(got["rgb"])) > 1000


def test_tiny_grid_clips_the_stencil(oracle_mod, hfpf_mod, synth_mod):
    sc = scenes.Scene(3, 160, 120, 0.005, bbox=(-0.2, 0.2, -0.2, 0.2, 0.545, 0.566), clean_every=0)
    _check(oracle_mod, hfpf_mod, sc, "tiny")


def test_direct_update(oracle_mod, hfpf_mod, synth_mod):
    _check(oracle_mod, hfpf_mod, _forms_scene(), "forms", engine_kw=dict(binned_update=False))


def test_update_form_per_point(oracle_mod, hfpf_mod, synth_mod, monkeypatch):
    monkeypatch.setenv("HFPF_UPDATE_FORM", "p")
    _check(oracle_mod, hfpf_mod, _forms_scene(), "forms")


def test_update_shape_dense(oracle_mod, hfpf_mod, synth_mod, monkeypatch):
    monkeypatch.setenv("HFPF_UPD_SHAPE", "0")
    _check(oracle_mod, hfpf_mod, _forms_scene(), "forms")


def test_update_shape_wide(oracle_mod, hfpf_mod, synth_mod, monkeypatch):
    monkeypatch.setenv("HFPF_UPD_SHAPE", "1")
    _check(oracle_mod, hfpf_mod, _forms_scene(), "forms")


def test_forced_table_miss(oracle_mod, hfpf_mod, synth_mod, monkeypatch):
    """Records with an odd id never get an LDS slot: their words go through device atomics."""
    monkeypatch.setenv("HFPF_TEST_TABLE_SKIP", "1")
    _check(oracle_mod, hfpf_mod, _forms_scene(), "forms")


RANKS_SCENE = dict(n_frames=7, W=160, H=120, resolution=0.001, fx=615.0, clean_every=3)


def test_two_virtual_ranks(oracle_mod, hfpf_mod, synth_mod):
    """Each rank holds partial words; they are summed at extract."""
    sc = scenes.Scene(**RANKS_SCENE)
    ref, exact, mom = _oracle(oracle_mod, sc, "ranks")
    rows, occ, ctrs = run_virtual(hfpf_mod, sc, 2)
    assert all(c["frames_integrated"] > 0 for c in ctrs)
    scenes.compare_rows(ref, rows)
    assert scenes.compare_rows_exact(exact, rows)["exact_bytes_differing"] == 0


def test_query_winner_rows(oracle_mod, hfpf_mod, synth_mod):
    """hfpf_query returns the winner's row from another kernel (record_centroid / record_row in k_query): each returned row against
    the exact row of its voxel."""
    sc = scenes.Scene(**RANKS_SCENE)
    ref, exact, mom = _oracle(oracle_mod, sc, "ranks")
    live = exact[exact["count"] > 0]
    rng = np.random.default_rng(0xE7AC)
    pts = (np.stack([live["x"], live["y"], live["z"]], axis=1) + rng.normal(0.0, 0.0005, (len(live), 3))).astype(np.float32)
    with hfpf_mod.OccupancyGrid(resolution=sc.resolution, bbox=sc.bbox, **SMALL_CAPS) as eg:
        scenes.run(eg, sc, "integrate")
        hits, rows = eg.query(pts, IDENT, radius=1, rows=True)
    found = rows["ix"] >= 0
    assert found.sum() > 10000
    rows = rows[found]
    index = {(int(r["ix"]), int(r["iy"]), int(r["iz"])): i for i, r in enumerate(exact)}
    sel = np.array([index[(int(r["ix"]), int(r["iy"]), int(r["iz"]))] for r in rows])
    assert len(np.unique(sel)) > 5000
    assert scenes.compare_rows_exact(exact[sel], rows)["exact_bytes_differing"] == 0
