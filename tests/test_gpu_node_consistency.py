"""GPU: the node shell's depth-consistency report (hfpf_node_set_depth_consistency).  With it set, ~process writes consistency.csv
and consistency_summary.csv beside the cloud: hfpf_depth_consistency of the last depth images the node integrated, on the saved rows,
as tests/consistency_ref.py gives it; with NULL the files are byte-identical to those of a node that never called it."""
import os

import numpy as np
import pytest

import consistency_ref as CR
from gpu_support import BBOX, DEPTH_CAPS, RES, node_feed, node_grid
from scenes import DepthScene

pytestmark = pytest.mark.gpu
W, H = 160, 120
KW = dict(window=1, tolerance=0.004, min_cos=0.3)


def _read(d, *files):
    return [open(os.path.join(str(d), f), "rb").read() for f in files]


@pytest.mark.parametrize("filtered", [False, True], ids=["plain", "component_filter"])
def test_process_writes_the_consistency_files(hfpf_mod, synth_mod, tmp_path, filtered):
    import hfpf_node
    sc = DepthScene(4, W, H, clean_every=0)
    with hfpf_node.FusionNode(BBOX, directory_name=str(tmp_path), resolution=RES, final_clean_on_process=True, **DEPTH_CAPS) as n:
        for bad in (dict(keep_frames=0), dict(keep_frames=4097), dict(keep_frames=3, tolerance=0.0)):
            with pytest.raises(hfpf_mod.HfpfError) as e:
                n.set_depth_consistency(**dict(KW, **bad))
            assert e.value.code == -2
        # a ring of three: the report looks through frames 1, 2 and 3, numbered 0, 1 and 2; DROP is ignored (a report)
        n.set_depth_consistency(keep_frames=3, drop=True, **KW)
        node_feed(n, sc)
        frames = np.stack([sc.frames[f][0] for f in (1, 2, 3)])
        poses = [sc.poses[f] for f in (1, 2, 3)]
        g = node_grid(hfpf_mod, hfpf_node, n)
        try:
            g.clean()
            ghost = CR.ghost_cloud(RES)
            g.integrate(ghost, sc.poses[1])
            g.clean()
            rows = g.extract().copy()
            if filtered:
                ckw = dict(reach=1, min_count=2.0, min_rows=50)
                kept = g.extract_components(**ckw)[0]
                all_rows, rec, _ = CR.consistency(rows, frames, poses, sc.K, min_count=2.0, **KW)
                sel = np.searchsorted(CR.voxel_keys(all_rows), CR.voxel_keys(kept))
                assert 0 < len(kept) < len(all_rows) and all_rows[sel].tobytes() == kept.tobytes()
                rows, rec = kept, rec[sel].copy()
                _, summary = CR.finish(rec)
                n.set_component_filter(**ckw)
            else:
                rows, rec, summary = CR.consistency(rows, frames, poses, sc.K, **KW)
        finally:
            g._h = None
        assert len(rows) > 1000 and summary["n_contradicted"] > 50 and summary["pairs_support"] > 1000, summary
        rc, ok, msg = n.process()
        assert rc == 0 and ok, msg
        assert "saved %d points" % len(rows) in msg
    got = _read(tmp_path, "consistency.csv", "consistency_summary.csv")
    assert got[0].decode() == CR.csv(rows, rec)
    assert got[1].decode() == CR.summary_csv(summary)


def test_null_setting_writes_what_a_plain_node_writes(hfpf_mod, synth_mod, tmp_path):
    import hfpf_node
    sc = DepthScene(3, W, H, clean_every=0)
    out = {}
    for name in ("plain", "off"):
        d = tmp_path / name
        os.makedirs(str(d))
        with hfpf_node.FusionNode(BBOX, directory_name=str(d), resolution=RES, final_clean_on_process=True, **DEPTH_CAPS) as n:
            if name == "off":
                n.set_depth_consistency(keep_frames=8, **KW)
                n.set_depth_consistency(None)
            node_feed(n, sc)
            rc, ok, msg = n.process()
            assert rc == 0 and ok, msg
        out[name] = _read(d, "test_cloud.pcd", "meta.csv")
        assert sorted(os.listdir(str(d))) == ["meta.csv", "test_cloud.pcd"], "no consistency file without the setting"
    assert len(out["plain"][0]) > 10000 and out["plain"] == out["off"]


def test_reset_empties_the_ring(hfpf_mod, synth_mod, tmp_path):
    """After ~reset the report has no frames to look through: every record is zero with first_through = none."""
    import hfpf_node
    sc = DepthScene(3, W, H, clean_every=0)
    with hfpf_node.FusionNode(BBOX, directory_name=str(tmp_path), resolution=RES, final_clean_on_process=True, **DEPTH_CAPS) as n:
        n.set_depth_consistency(keep_frames=8, **KW)
        node_feed(n, sc)
        n.reset()
        rc, ok, msg = n.process()
        assert rc == 0 and ok, msg
    lines = open(os.path.join(str(tmp_path), "consistency.csv")).read().splitlines()
    assert len(lines) > 1000 and all(l.endswith(",0,0,0,0,0,%d,0" % CR.NONE) for l in lines[1:])
    head, values = open(os.path.join(str(tmp_path), "consistency_summary.csv")).read().splitlines()
    assert head == ",".join(CR.SUMMARY_KEYS) and values == "%d,0,0,0,%d,0,0,0" % (len(lines) - 1, len(lines) - 1)
