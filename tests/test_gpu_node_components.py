"""GPU: the node shell's component filter (hfpf_node_set_component_filter).  With it set, ~process writes test_cloud.pcd and meta.csv
from the rows hfpf_extract_components keeps; with NULL the files are byte-identical to those of a node that never called it."""
import os

import numpy as np
import pytest

import components_ref as CR
from gpu_support import BBOX, DEPTH_CAPS, RES, add_patches, in_boxes, node_feed, node_grid
from scenes import DepthScene

pytestmark = pytest.mark.gpu
FILES = ("test_cloud.pcd", "meta.csv")


def _read(d):
    return [open(os.path.join(str(d), f), "rb").read() for f in FILES]


def test_process_writes_the_kept_rows(hfpf_mod, synth_mod, tmp_path):
    import hfpf_node
    sc = DepthScene(6, 320, 240, clean_every=0)
    published = []
    with hfpf_node.FusionNode(BBOX, directory_name=str(tmp_path), resolution=RES, final_clean_on_process=True,
                              publisher=lambda rows, frame: published.append(rows), **DEPTH_CAPS) as n:
        with pytest.raises(hfpf_mod.HfpfError) as e:
            n.set_component_filter(reach=7)
        assert e.value.code == -2
        node_feed(n, sc)
        g = node_grid(hfpf_mod, hfpf_node, n)
        try:
            g.clean()
            boxes = add_patches(g)  # two specks well clear of the surface
            rows = g.extract().copy()
            ref = CR.components(rows, reach=2)
            patch = in_boxes(rows, boxes)
            min_rows = int(ref[2]["n_rows"][np.unique(ref[1][patch])].max()) + 1
            assert patch.sum() > 0 and min_rows < ref[2]["n_rows"].max()
            kept = g.extract_components(reach=2, min_rows=min_rows)[0]
        finally:
            g._h = None
        assert kept.tobytes() == CR.components(rows, reach=2, min_rows=min_rows)[0].tobytes()
        assert 0 < len(kept) < len(rows) and not in_boxes(kept, boxes).any()
        n.set_component_filter(reach=2, min_rows=min_rows)
        rc, ok, msg = n.process()
        assert rc == 0 and ok, msg
        assert "saved %d points" % len(kept) in msg
    want = tmp_path / "want"
    os.makedirs(str(want))
    hfpf_mod.write_pcd(kept, str(want / FILES[0]))
    hfpf_mod.write_meta_csv(kept, str(want / FILES[1]))
    assert _read(tmp_path) == _read(want)
    assert len(published) == 1 and published[0].tobytes() == kept.tobytes()


def test_null_filter_writes_what_a_plain_node_writes(hfpf_mod, synth_mod, tmp_path):
    import hfpf_node
    sc = DepthScene(4, 320, 240, clean_every=0)
    out = {}
    for name in ("plain", "off"):
        d = tmp_path / name
        os.makedirs(str(d))
        with hfpf_node.FusionNode(BBOX, directory_name=str(d), resolution=RES, final_clean_on_process=True, **DEPTH_CAPS) as n:
            if name == "off":
                n.set_component_filter(reach=1, min_rows=1000)
                n.set_component_filter(None)
            node_feed(n, sc)
            rc, ok, msg = n.process()
            assert rc == 0 and ok, msg
        out[name] = _read(d)
    assert len(out["plain"][0]) > 100000 and out["plain"] == out["off"]
