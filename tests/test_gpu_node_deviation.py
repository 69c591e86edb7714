"""GPU: the node shell's reference mesh (hfpf_node_set_reference_mesh).  With it set, ~process writes deviation.csv and
deviation_summary.csv beside the cloud: the direct call's output on the saved rows, formatted the same way."""
import os

import numpy as np
import pytest

from gpu_support import BBOX, DEPTH_CAPS, RES, deviation_csv, deviation_summary_csv, node_feed, node_grid
from scenes import DepthScene

pytestmark = pytest.mark.gpu
MD = 4 * RES


@pytest.mark.parametrize("filtered", [False, True], ids=["plain", "component_filter"])
def test_process_writes_the_deviation_files(hfpf_mod, synth_mod, tmp_path, filtered):
    import deviation_ref as D
    import hfpf_node
    sc = DepthScene(4, 320, 240, clean_every=0)
    with hfpf_node.FusionNode(BBOX, directory_name=str(tmp_path), resolution=RES, final_clean_on_process=True, **DEPTH_CAPS) as n:
        with pytest.raises(hfpf_mod.HfpfError) as e:
            n.set_reference_mesh(np.zeros((3, 3), np.float32), [[0, 1, 2]], max_distance=-1.0)
        assert e.value.code == -2
        node_feed(n, sc)
        g = node_grid(hfpf_mod, hfpf_node, n)
        try:
            g.clean()
            verts, tris = g.extract_mesh()
            if filtered:
                kw = dict(reach=1, min_count=2.0, min_rows=50)
                kept = g.extract_components(**kw)[0]
                all_rows, dev, _ = g.compare_mesh(verts, tris, rows=True, min_count=2.0, max_distance=MD)
                key = lambda r: (r["ix"].astype(np.int64) << 42) | (r["iy"].astype(np.int64) << 21) | r["iz"].astype(np.int64)
                sel = np.searchsorted(key(all_rows), key(kept))
                assert 0 < len(kept) < len(all_rows) and all_rows[sel].tobytes() == kept.tobytes()
                rows, dev = kept, dev[sel]
                summary = D.summary(dev)
                full = g.compare_mesh(verts, tris, min_count=2.0, max_distance=MD)[1]
                summary["n_tris_valid"], summary["n_tris_invalid"] = full["n_tris_valid"], full["n_tris_invalid"]
                n.set_component_filter(**kw)
            else:
                rows, dev, summary = g.compare_mesh(verts, tris, rows=True, max_distance=MD)
        finally:
            g._h = None
        assert len(rows) > 1000 and summary["n_found"] > 0
        n.set_reference_mesh(verts, tris, max_distance=MD)
        rc, ok, msg = n.process()
        assert rc == 0 and ok, msg
    assert open(os.path.join(str(tmp_path), "deviation.csv")).read() == deviation_csv(rows, dev)
    assert open(os.path.join(str(tmp_path), "deviation_summary.csv")).read() == deviation_summary_csv(summary)
