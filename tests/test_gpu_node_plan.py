"""GPU: the node shell's view plan (hfpf_node_set_view_candidates).  With a reference mesh and candidate views set, ~process writes
view_plan.csv and view_plan_summary.csv beside the deviation files: the direct call's scores and summary on the same rows, hidden
rows included, at the pose the deviation files use."""
import os

import numpy as np
import pytest

import plan_support as S
from gpu_support import BBOX, DEPTH_CAPS, IDENT, RES, node_feed, node_grid
from scenes import DepthScene

pytestmark = pytest.mark.gpu
HEADER = "view,rank,n_in_view,n_facing,n_visible,visible_q40,gain_q40,gain_samples"
SUMMARY = ("n_views", "n_selected", "n_targets", "n_reachable", "n_planned", "target_q40", "reachable_q40", "planned_q40")
COVERAGE = ("n_samples", "n_in_bbox", "n_covered")
PLAN = dict(S.MAIN, spacing=4 * RES, model_occludes=True)


@pytest.mark.parametrize("mode", ["plain", "hidden", "off"])
def test_process_writes_the_view_plan_files(hfpf_mod, synth_mod, tmp_path, mode):
    import hfpf_node
    sc = DepthScene(3, 160, 120, clean_every=0)
    verts, tris = S.sphere_and_box()
    poses = S.main_poses()
    with hfpf_node.FusionNode(BBOX, directory_name=str(tmp_path), resolution=RES, final_clean_on_process=True, **DEPTH_CAPS) as n:
        with pytest.raises(hfpf_mod.HfpfError) as e:
            n.set_view_candidates(poses, **S.VIEW, **dict(PLAN, tolerance=0.0))
        assert e.value.code == -2
        with pytest.raises(hfpf_mod.HfpfError):
            n.set_view_candidates(np.full((2, 12), np.nan), **S.VIEW, **PLAN)
        n.set_view_candidates(poses, **S.VIEW, **PLAN)  # without a reference mesh: no effect
        node_feed(n, sc)
        g = node_grid(hfpf_mod, hfpf_node, n)
        try:
            g.clean()
            rows = g.extract()
            if mode == "hidden":  # the half of the model with the larger x: its rows neither cover nor occlude
                mid = int(np.median(rows["ix"]))
                c = g.hide_box((mid, -1, -1), (1 << 20, 1 << 20, 1 << 20))
                assert 0 < c["n_hidden"] < len(rows), c
            scores, rec, s = g.plan_views(verts, tris, poses, IDENT, tri_plan=False, **S.VIEW, **PLAN)
            if mode == "hidden":
                g.show_all()
                shown = g.plan_views(verts, tris, poses, IDENT, tri_plan=False, **S.VIEW, **PLAN)
                assert shown[2]["n_targets"] < s["n_targets"], "hidden rows cover nothing"
                g.hide_box((mid, -1, -1), (1 << 20, 1 << 20, 1 << 20))
        finally:
            g._h = None
        assert s["n_selected"] >= 1 and 0 < s["n_planned"] <= s["n_reachable"] < s["n_targets"]
        n.set_reference_mesh(verts, tris, IDENT, max_distance=3 * RES)
        if mode == "off":
            with pytest.raises(hfpf_mod.HfpfError):
                n.set_view_candidates(poses, **S.VIEW, **dict(PLAN, max_views=0))  # refused: the setting stays as it was ...
            n.set_view_candidates(None)                                            # ... until it is turned off
        rc, ok, msg = n.process()
        assert rc == 0 and ok, msg
    files = [os.path.join(str(tmp_path), f) for f in ("view_plan.csv", "view_plan_summary.csv")]
    assert os.path.exists(os.path.join(str(tmp_path), "deviation.csv"))
    if mode == "off":
        assert not any(os.path.exists(f) for f in files)
        return
    head, *lines = open(files[0]).read().splitlines()
    assert head == HEADER and len(lines) == len(poses)
    got = np.zeros(len(lines), hfpf_mod.VIEW_SCORE_DTYPE)
    for v, line in enumerate(lines):
        f = [int(x) for x in line.split(",")]
        assert f[0] == v
        got[v] = tuple(f[1:])
    assert got.tobytes() == scores.tobytes()
    head, line = open(files[1]).read().splitlines()
    assert head == ",".join(SUMMARY + COVERAGE)
    assert [int(x) for x in line.split(",")] == [s[k] for k in SUMMARY] + [s["coverage"][k] for k in COVERAGE]
