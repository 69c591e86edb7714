"""GPU: the node shell's reference coverage (hfpf_node_set_reference_coverage).  With a reference mesh and coverage options set,
~process writes coverage.csv and coverage_summary.csv beside the deviation files: the direct call's records and summary at the pose
the deviation files use, which is the refined pose when alignment is on."""
import os

import numpy as np
import pytest

from gpu_support import ALIGN_KW, ALIGN_MD, ALIGN_START, BBOX, DEPTH_CAPS, RES, node_feed, node_grid
from scenes import DepthScene

pytestmark = pytest.mark.gpu
COVER = dict(radius=2, max_distance=2 * RES, spacing=RES, min_normal_dot=0.3)
HEADER = "tri,n_samples,n_in_bbox,n_covered,flags,area,max_distance,sum_dist_q30"
SUMMARY = ("n_tris_valid", "n_tris_invalid", "n_tris_huge", "n_samples", "n_in_bbox", "n_covered", "sum_dist_q30", "area_q40_lo", "area_q40_hi",
           "covered_q40_lo", "covered_q40_hi", "max_distance")


def _parse(path, dtype):
    """coverage.csv back into records: the floats went out as %.9g, which a float32 survives."""
    head, *lines = open(path).read().splitlines()
    assert head == HEADER
    cov = np.zeros(len(lines), dtype)
    for k, line in enumerate(lines):
        v = line.split(",")
        assert int(v[0]) == k
        cov[k] = (int(v[1]), int(v[2]), int(v[3]), int(v[4]), np.float32(v[5]), np.float32(v[6]), int(v[7]))
    return cov


@pytest.mark.parametrize("mode", ["plain", "aligned", "off"])
def test_process_writes_the_coverage_files(hfpf_mod, synth_mod, tmp_path, mode):
    import hfpf_node
    sc = DepthScene(3, 160, 120, clean_every=0)
    with hfpf_node.FusionNode(BBOX, directory_name=str(tmp_path), resolution=RES, final_clean_on_process=True, **DEPTH_CAPS) as n:
        with pytest.raises(hfpf_mod.HfpfError) as e:
            n.set_reference_coverage(spacing=0.0)
        assert e.value.code == -2
        n.set_reference_coverage(**COVER)  # without a reference mesh: no effect
        node_feed(n, sc)
        g = node_grid(hfpf_mod, hfpf_node, n)
        try:
            g.clean()
            verts, tris = g.extract_mesh()
            tris = np.ascontiguousarray(tris[::8])  # spread over the whole model, so that an align has something to hold on to
            fit = g.align_mesh(verts, tris, ALIGN_START, **ALIGN_KW) if mode == "aligned" else None
            pose = fit["pose"] if fit else ALIGN_START
            cov, s = g.cover_mesh(verts, tris, pose, **COVER)
            at_start = g.cover_mesh(verts, tris, ALIGN_START, **COVER)[1]
        finally:
            g._h = None
        assert len(tris) > 1000 and 0 < s["n_covered"] < s["n_samples"]
        n.set_reference_mesh(verts, tris, ALIGN_START, max_distance=ALIGN_MD)
        if mode == "aligned":
            n.set_reference_alignment(**ALIGN_KW)
        if mode == "off":
            with pytest.raises(hfpf_mod.HfpfError):
                n.set_reference_coverage(radius=9)  # refused: the setting stays as it was ...
            n.set_reference_coverage(None)          # ... until it is turned off
        rc, ok, msg = n.process()
        assert rc == 0 and ok, msg
    files = [os.path.join(str(tmp_path), f) for f in ("coverage.csv", "coverage_summary.csv")]
    assert os.path.exists(os.path.join(str(tmp_path), "deviation.csv"))
    if mode == "off":
        assert not any(os.path.exists(f) for f in files)
        return
    if mode == "aligned":
        line = open(os.path.join(str(tmp_path), "alignment.csv")).read().splitlines()[1].split(",")
        assert np.array([float(x) for x in line[5:]]).tobytes() == np.ascontiguousarray(pose, np.float64).tobytes()
        print("covered at the start pose %d, at the refined pose %d of %d samples" % (at_start["n_covered"], s["n_covered"], s["n_samples"]))
        assert not np.array_equal(np.asarray(pose), np.asarray(ALIGN_START)), "the align moved the mesh"
    got = _parse(files[0], hfpf_mod.TRI_COVERAGE_DTYPE)
    assert got.tobytes() == cov.tobytes()
    head, line = open(files[1]).read().splitlines()
    assert head == ",".join(SUMMARY)
    vals = line.split(",")
    assert [int(x) for x in vals[:-1]] == [s[k] for k in SUMMARY[:-1]] and np.float32(vals[-1]) == np.float32(s["max_distance"])
