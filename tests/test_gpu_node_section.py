"""GPU: the node shell's section planes (hfpf_node_set_section_planes).  With section planes and mesh output set, ~process cuts the mesh
it writes to mesh.ply and writes sections.csv and section_summary.csv beside it: the direct call's segments and plane records.
Without mesh output it fails with HFPF_ERR_STATE before anything is written, and the grid is kept."""
import os

import numpy as np
import pytest

from gpu_support import BBOX, DEPTH_CAPS, RES, node_feed, node_grid
from scenes import DepthScene

pytestmark = pytest.mark.gpu
PLANES = np.array([[0, 1.0, 0, -0.04], [0, 1.0, 0, 0.9], [1.0, 0, 0, 0.05], [0.6, 0.3, 1.0, 0.48]])  # plane 1 misses everything
HEADER = "plane,contour,tri,x0,y0,z0,x1,y1,z1"
SUMMARY = ("first_segment", "n_segments", "first_point", "n_points", "first_contour", "n_contours", "n_closed", "n_branched", "length_q32", "area_q28")
FILES = ("sections.csv", "section_summary.csv")


def _segments_csv(points, segments):
    lines = [HEADER]
    for s in segments:
        a, b = points[s["p0"]], points[s["p1"]]
        lines.append("%d,%d,%d,%s" % (a["plane"], s["contour"], s["tri"], ",".join("%.9g" % float(v) for v in (a["x"], a["y"], a["z"], b["x"], b["y"], b["z"]))))
    return "\n".join(lines) + "\n"


def _summary_csv(recs):
    lines = ["plane," + ",".join(SUMMARY)]
    for j, r in enumerate(recs):
        lines.append("%d,%s" % (j, ",".join("%d" % int(r[k]) for k in SUMMARY)))
    return "\n".join(lines) + "\n"


def test_process_writes_the_section_files(hfpf_mod, synth_mod, tmp_path):
    import hfpf_node
    sc = DepthScene(3, 160, 120, clean_every=0)
    with hfpf_node.FusionNode(BBOX, directory_name=str(tmp_path), resolution=RES, final_clean_on_process=True, **DEPTH_CAPS) as n:
        for bad in ([[0, 0, 0, 1.0]], [[np.nan, 0, 1, 0]], [[0, 0, 1, np.inf]]):
            with pytest.raises(hfpf_mod.HfpfError) as e:
                n.set_section_planes(bad)
            assert e.value.code == -2
        with pytest.raises(hfpf_mod.HfpfError) as e:
            n.set_section_planes(PLANES, n_planes=4097)
        assert e.value.code == -2
        o = hfpf_mod.section_opts()
        o.flags = 1
        with pytest.raises(hfpf_mod.HfpfError):
            n.set_section_planes(PLANES, opts=o)
        node_feed(n, sc)
        n.set_section_planes(PLANES)
        # without mesh output: refused before anything is written, and the model is still there
        rc, ok, msg = n.process()
        assert rc == -5 and not ok and "mesh output" in msg, (rc, ok, msg)
        assert not os.listdir(str(tmp_path))
        with pytest.raises(hfpf_mod.HfpfError):
            n.set_section_planes([[0, 0, 0, 0]])  # refused: the setting stays as it was
        n.set_mesh_output(radius=2)
        g = node_grid(hfpf_mod, hfpf_node, n)
        try:
            g.clean()
            verts, tris = g.extract_mesh(radius=2)
            points, segments, contours, recs, s = g.section_mesh(verts, tris, None, PLANES)
        finally:
            g._h = None
        assert len(tris) > 1000 and recs["n_segments"].tolist()[1] == 0 and recs["n_segments"].max() > 100, recs["n_segments"]
        rc, ok, msg = n.process()
        assert rc == 0 and ok, msg
    got = [open(os.path.join(str(tmp_path), f)).read() for f in FILES]
    assert os.path.exists(os.path.join(str(tmp_path), "mesh.ply"))
    assert got[0] == _segments_csv(points, segments), "sections.csv"
    assert got[1] == _summary_csv(recs), "section_summary.csv"
    assert len(got[0].splitlines()) == 1 + s["n_segments"] and len(got[1].splitlines()) == 1 + len(PLANES)


def test_turned_off_it_writes_neither_file(hfpf_mod, synth_mod, tmp_path):
    import hfpf_node
    sc = DepthScene(2, 160, 120, clean_every=0)
    with hfpf_node.FusionNode(BBOX, directory_name=str(tmp_path), resolution=RES, final_clean_on_process=True, **DEPTH_CAPS) as n:
        n.set_mesh_output(radius=2)
        n.set_section_planes(PLANES)
        n.set_section_planes(None)
        node_feed(n, sc)
        rc, ok, msg = n.process()
        assert rc == 0 and ok, msg
    assert os.path.exists(os.path.join(str(tmp_path), "mesh.ply")) and not any(os.path.exists(os.path.join(str(tmp_path), f)) for f in FILES)
