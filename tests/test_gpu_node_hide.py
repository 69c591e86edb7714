"""GPU: the node shell and the hidden set (hfpf_node_set_hide_filtered, hfpf_node_hide_box).  With hide_filtered on and a component
filter set, ~process hides what the filter drops: test_cloud.pcd and meta.csv are those of the filter alone, and every file is
byte-identical to that of a plain node on whose grid the same rows were hidden with hfpf_hide_voxels -- the direct calls on a handle
with those rows hidden.  With it off every file is that of a node that never called it.  hfpf_node_hide_box hides the voxel box
tests/hide_ref.py computes from the metres."""
import os

import numpy as np
import pytest

import hide_ref as HR
from gpu_support import ALIGN_KW, ALIGN_MD, BBOX, DEPTH_CAPS, RES, add_patches, in_boxes, node_feed, node_grid
from scenes import DepthScene

pytestmark = pytest.mark.gpu
W, H = 320, 240
CLOUD = ("test_cloud.pcd", "meta.csv")
REPORTS = ("mesh.ply", "deviation.csv", "deviation_summary.csv", "coverage.csv", "coverage_summary.csv", "alignment.csv", "consistency.csv",
           "consistency_summary.csv", "test_cloud_50.pcd", "test_cloud_100.pcd", "test_cloud_classified.pcd", "test_cloud_normals.pcd")


def _files(d):
    return {f: open(os.path.join(str(d), f), "rb").read() for f in sorted(os.listdir(str(d)))}


def _run(hfpf_mod, d, sc, mode, shared):
    """One node through the stream, the two specks and ~process, with every report on.  mode: "filter" (the component filter alone),
    "hide" (filter + hide_filtered), "off" (hide_filtered switched on and off again), "direct" (no filter: the rows the filter drops
    are hidden on the node's grid with hfpf_hide_voxels).  Returns the files."""
    import hfpf_node
    os.makedirs(str(d))
    with hfpf_node.FusionNode(BBOX, directory_name=str(d), resolution=RES, final_clean_on_process=True, write_variants=True, **DEPTH_CAPS) as n:
        n.set_depth_consistency(keep_frames=3, window=1, tolerance=0.004, min_cos=0.3)
        node_feed(n, sc)
        g = node_grid(hfpf_mod, hfpf_node, n)
        try:
            g.clean()
            boxes = add_patches(g)  # two specks well clear of the surface
            rows = g.extract().copy()
            if "ckw" not in shared:
                patch = in_boxes(rows, boxes)
                rv, labels, comps = g.extract_components(reach=2)
                shared["ckw"] = dict(reach=2, min_rows=int(comps["n_rows"][np.unique(labels[patch])].max()) + 1)
                shared["mesh"] = g.extract_mesh(radius=2)
                shared["rows"], shared["boxes"] = rows, boxes
            assert rows.tobytes() == shared["rows"].tobytes(), "every node fuses the same model"
            kept = g.extract_components(**shared["ckw"])[0]
            assert 0 < len(kept) < len(rows) and not in_boxes(kept, boxes).any() and in_boxes(rows, boxes).sum() > 100
            shared["kept"] = kept
            if mode == "direct":
                c = g.hide_voxels(kept, "hide_others")
                assert c["n_hidden"] == len(rows) - len(kept) and c["n_matched"] == len(kept), c
        finally:
            g._h = None
        v, t = shared["mesh"]
        n.set_mesh_output(radius=2)
        n.set_reference_mesh(v, t, max_distance=3 * RES)
        n.set_reference_alignment(**dict(ALIGN_KW, max_iterations=3, max_distance=ALIGN_MD))
        n.set_reference_coverage(radius=2, max_distance=2 * RES, spacing=2 * RES)
        if mode != "direct":
            n.set_component_filter(**shared["ckw"])
        if mode in ("hide", "off"):
            n.set_hide_filtered(True)
        if mode == "off":
            n.set_hide_filtered(False)
        rc, ok, msg = n.process()
        assert rc == 0 and ok, msg
        assert "saved %d points" % len(kept) in msg
        g = node_grid(hfpf_mod, hfpf_node, n)
        try:
            assert len(g.hidden()) == 0 and len(g.extract()) == 0, "~process clears the grid, which empties the hidden set"
        finally:
            g._h = None
    return _files(d)


def test_hide_filtered(hfpf_mod, synth_mod, tmp_path):
    sc = DepthScene(4, W, H, clean_every=0)
    shared = {}
    out = {mode: _run(hfpf_mod, tmp_path / mode, sc, mode, shared) for mode in ("filter", "hide", "direct", "off")}
    for mode, files in out.items():
        assert sorted(files) == sorted(CLOUD + REPORTS + ("test_cloud_150.pcd", "test_cloud_200.pcd", "test_cloud_250.pcd", "test_cloud_300.pcd")), (mode, sorted(files))
    # the cloud is that of the filter alone
    for f in CLOUD:
        assert len(out["filter"][f]) > 10000 and out["hide"][f] == out["filter"][f], f
    # every file is that of the direct calls on a handle with the same rows hidden
    for f in CLOUD + REPORTS:
        assert out["hide"][f] == out["direct"][f], "%s: hide_filtered against a plain node on a grid with the dropped rows hidden" % f
    # and the filter alone does not filter them: the specks are in its mesh, its variants and its reports
    for f in ("mesh.ply", "test_cloud_normals.pcd", "test_cloud_classified.pcd"):
        assert out["hide"][f] != out["filter"][f], "%s: the filter alone leaves the specks in" % f
    assert len(out["hide"]["test_cloud_normals.pcd"]) < len(out["filter"]["test_cloud_normals.pcd"])
    # off: every file is that of a node that never called it
    assert out["off"] == out["filter"], [f for f in out["off"] if out["off"][f] != out["filter"][f]]


def test_hide_box_in_metres(hfpf_mod, synth_mod, tmp_path):
    import hfpf_node
    sc = DepthScene(3, W, H, clean_every=0)
    with hfpf_node.FusionNode(BBOX, directory_name=str(tmp_path), resolution=RES, final_clean_on_process=True, **DEPTH_CAPS) as n:
        node_feed(n, sc)
        g = node_grid(hfpf_mod, hfpf_node, n)
        try:
            g.clean()
            rows = g.extract().copy()
            dims, res = g.dims
            x = np.sort(rows["x"].astype(np.float64))
            z = np.sort(rows["z"].astype(np.float64))
            boxes = [("hide", [x[len(x) // 4], x[len(x) // 2], -10.0, 10.0, -10.0, 10.0]),                      # a slab: "erase this"
                     ("hide_others", [-1e30, 1e30, float("-inf"), float("inf"), z[len(z) // 10], z[-len(z) // 10]]),  # "crop to this"
                     ("show", [x[len(x) // 4], x[len(x) // 3], -0.01, 0.01, 0.0, 1.0]),
                     ("hide", [0.2, 0.1, -1.0, 1.0, -1.0, 1.0])]                                                   # min > max: the empty box
            H_ref = None
            for op, box in boxes:
                got = n.hide_box(box, op)
                lo, hi = HR.box_of_metres(box, BBOX, res)
                H_ref, want = HR.hide_box(rows, H_ref, dims, lo, hi, op)
                print("%s %r -> %r .. %r: %r" % (op, box, lo.tolist(), hi.tolist(), got))
                assert got == want, (op, box, got, want)
                assert g.hidden().tobytes() == H_ref.tobytes() and g.extract().tobytes() == HR.visible(rows, H_ref).tobytes(), (op, box)
            assert len(rows) // 10 < len(H_ref) < len(rows), "the boxes hid a part of the model"
            with pytest.raises(hfpf_mod.HfpfError) as e:
                n.hide_box([float("nan"), 0, 0, 0, 0, 0])
            assert e.value.code == -2
            with pytest.raises(hfpf_mod.HfpfError) as e:
                n.hide_box([0, 1, 0, 1, 0, 1], 7)
            assert e.value.code == -2 and g.hidden().tobytes() == H_ref.tobytes()
        finally:
            g._h = None
        rc, ok, msg = n.process()   # the saved cloud leaves the hidden rows out
        assert rc == 0 and ok and "saved %d points" % (len(rows) - len(H_ref)) in msg, msg
