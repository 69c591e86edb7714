"""GPU: the node shell's mesh topology (hfpf_node_set_mesh_topology).  With it and mesh output set, ~process also writes mesh_edges.csv,
mesh_loops.csv, mesh_shells.csv and mesh_topology_summary.csv beside mesh.ply: the direct call's records on the mesh that file holds.
Without mesh output it fails with HFPF_ERR_STATE before anything is written, and the grid is kept."""
import os

import pytest

import topology_ref as T
from gpu_support import BBOX, DEPTH_CAPS, RES, node_feed, node_grid
from scenes import DepthScene

pytestmark = pytest.mark.gpu
FILES = ("mesh_edges.csv", "mesh_loops.csv", "mesh_shells.csv", "mesh_topology_summary.csv")
EDGE = ("p0", "p1", "tri", "kind", "uses", "loop", "shell")
LOOP = ("first_vertex", "n_verts", "n_edges", "n_ends", "flags", "shell", "length_q32")
SHELL = ("first_vertex", "n_verts", "n_tris", "flags", "n_edges", "n_boundary", "n_nonmanifold", "n_miswound", "n_loops", "area_q32", "volume_q40")


def _csv(header, lines):
    return "\n".join([header] + lines) + "\n"


def _files(edges, loops, shells, s):
    return [_csv(",".join(EDGE), [",".join("%d" % int(e[k]) for k in EDGE) for e in edges]),
            _csv("loop," + ",".join(LOOP) + ",area_q28_x,area_q28_y,area_q28_z",
                 ["%d,%s,%s" % (i, ",".join("%d" % int(l[k]) for k in LOOP), ",".join("%d" % int(a) for a in l["area_q28"])) for i, l in enumerate(loops)]),
            _csv("shell," + ",".join(SHELL), ["%d,%s" % (i, ",".join("%d" % int(h[k]) for k in SHELL)) for i, h in enumerate(shells)]),
            _csv(",".join(T.SUMMARY_KEYS), [",".join("%d" % s[k] for k in T.SUMMARY_KEYS)])]


def test_process_writes_the_topology_files(hfpf_mod, synth_mod, tmp_path):
    import hfpf_node
    sc = DepthScene(3, 160, 120, clean_every=0)
    with hfpf_node.FusionNode(BBOX, directory_name=str(tmp_path), resolution=RES, final_clean_on_process=True, **DEPTH_CAPS) as n:
        o = hfpf_mod.topology_opts()
        o.flags = 1
        with pytest.raises(hfpf_mod.HfpfError) as e:
            n.set_mesh_topology(opts=o)
        assert e.value.code == -2
        node_feed(n, sc)
        n.set_mesh_topology()
        # without mesh output: refused before anything is written, and the model is still there
        rc, ok, msg = n.process()
        assert rc == -5 and not ok and "mesh output" in msg, (rc, ok, msg)
        assert not os.listdir(str(tmp_path))
        n.set_mesh_output(radius=2)
        g = node_grid(hfpf_mod, hfpf_node, n)
        try:
            g.clean()
            verts, tris = g.extract_mesh(radius=2)
            edges, loops, shells, _, s = g.mesh_topology(verts, tris)
        finally:
            g._h = None
        assert len(tris) > 1000 and s["n_boundary"] > 0 and len(loops) > 0 and len(shells) > 0, s
        rc, ok, msg = n.process()
        assert rc == 0 and ok, msg
    assert os.path.exists(os.path.join(str(tmp_path), "mesh.ply"))
    for name, got, want in zip(FILES, [open(os.path.join(str(tmp_path), f)).read() for f in FILES], _files(edges, loops, shells, s)):
        assert got == want, name


def test_turned_off_it_writes_none_of_the_files(hfpf_mod, synth_mod, tmp_path):
    import hfpf_node
    sc = DepthScene(2, 160, 120, clean_every=0)
    with hfpf_node.FusionNode(BBOX, directory_name=str(tmp_path), resolution=RES, final_clean_on_process=True, **DEPTH_CAPS) as n:
        n.set_mesh_output(radius=2)
        n.set_mesh_topology()
        n.set_mesh_topology(False)
        node_feed(n, sc)
        rc, ok, msg = n.process()
        assert rc == 0 and ok, msg
    assert os.path.exists(os.path.join(str(tmp_path), "mesh.ply")) and not any(os.path.exists(os.path.join(str(tmp_path), f)) for f in FILES)
