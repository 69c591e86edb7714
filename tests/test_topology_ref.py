"""CPU: the topology contract (include/hfpf.h) as tests/topology_ref.py restates it, pinned with closed forms on small meshes: the
cube, the cube without a face, a non-manifold fan, two triangles of opposite winding, a soup, the plan tests' sphere and box and a lone
triangle.  tests/test_gpu_topology.py compares the engine with this restatement byte for byte."""
import numpy as np
import pytest

import plan_support as PS
import section_support as S
import topology_ref as T
import topology_support as TS


def run(verts, tris, **kw):
    out = TS.reference(verts, tris, **kw)
    TS.consistent(*out)
    return out


def normals(verts, tris):
    P0, P1, P2 = (verts[tris[:, k]].astype(np.float64) for k in range(3))
    return np.cross(P1 - P0, P2 - P0)


def test_cube_is_one_watertight_shell_of_unit_volume():
    edges, loops, shells, tri_shell, s = run(*S.cube())
    assert (s["n_tris_valid"], s["n_edges"], s["n_interior"], len(edges), len(loops)) == (12, 18, 18, 0, 0)
    assert len(shells) == 1 and s["n_watertight"] == 1 and (tri_shell == 0).all()
    sh = shells[0]
    assert (sh["first_vertex"], sh["n_verts"], sh["n_tris"], sh["n_edges"], sh["flags"]) == (0, 8, 12, 18, T.SHELL_WATERTIGHT)
    assert sh["area_q32"] == 6 * TS.Q32
    # six triangles do not contain the representative; each term is rint(2^40 / 6)
    assert sh["volume_q40"] == 6 * int(np.rint(2.0 ** 40 / 6.0)) == TS.Q40 + 2 and abs(int(sh["volume_q40"]) - TS.Q40) <= 12


def test_cube_without_its_top_face_has_one_closed_rim():
    edges, loops, shells, _, s = run(*TS.open_cube())
    assert (s["n_tris_valid"], s["n_interior"], s["n_boundary"], s["n_nonmanifold"], s["n_miswound"]) == (10, 13, 4, 0, 0)
    assert [(int(e["p0"]), int(e["p1"])) for e in edges] == [(1, 3), (5, 1), (3, 7), (7, 5)], "1 -> 3 -> 7 -> 5 -> 1, listed in (va, vb) order"
    assert (edges["kind"] == T.BOUNDARY).all() and (edges["uses"] == np.where(edges["p0"] < edges["p1"], 1, 1 << 16)).all()
    assert len(loops) == 1 and s["n_closed_loops"] == 1
    lp = loops[0]
    assert (lp["first_vertex"], lp["n_verts"], lp["n_edges"], lp["n_ends"], lp["flags"], lp["shell"]) == (1, 4, 4, 0, T.LOOP_CLOSED, 0)
    assert lp["length_q32"] == 4 * TS.Q32 and lp["area_q28"].tolist() == [0, 0, -TS.Q28], "the rim of a hole points against the outward normal"
    assert shells[0]["flags"] == T.SHELL_OPEN and shells[0]["n_loops"] == 1 and s["n_watertight"] == 0


def test_fan_of_three_has_one_non_manifold_edge():
    edges, loops, shells, _, s = run(*S.fan(3))
    nm = edges[edges["kind"] == T.NONMANIFOLD]
    assert len(nm) == 1 and (nm[0]["p0"], nm[0]["p1"], nm[0]["uses"], nm[0]["tri"], nm[0]["loop"]) == (0, 1, 3, 0, T.NONE)
    assert s["n_boundary"] == 6 and s["n_nonmanifold"] == 1 and s["n_interior"] == 0
    assert len(loops) == 1 and loops[0]["flags"] == T.LOOP_BRANCHED and loops[0]["n_verts"] == 5
    assert shells[0]["flags"] == T.SHELL_OPEN | T.SHELL_NONMANIFOLD


def test_bow_has_one_miswound_edge():
    edges, loops, shells, _, s = run(*S.bow())
    mw = edges[edges["kind"] == T.MISWOUND]
    assert len(mw) == 1 and (mw[0]["p0"], mw[0]["p1"], mw[0]["uses"]) == (0, 1, 2) and s["n_boundary"] == 4
    assert len(loops) == 1 and loops[0]["flags"] == T.LOOP_BRANCHED and loops[0]["n_ends"] == 0
    assert shells[0]["flags"] == T.SHELL_OPEN | T.SHELL_MISWOUND


def test_a_triangle_listed_twice_shows_as_three_miswound_edges():
    verts, tris = TS.lone_triangle()
    edges, loops, shells, _, s = run(verts, np.concatenate([tris, tris]))
    assert (edges["kind"] == T.MISWOUND).all() and len(edges) == 3 and len(loops) == 0 and shells[0]["n_tris"] == 2


def test_unwelded_cube_is_all_boundary():
    verts, tris = S.unweld(*S.cube())
    edges, loops, shells, tri_shell, s = run(verts, tris)
    assert s["n_boundary"] == 36 == len(edges) and len(shells) == 12 and len(loops) == 12 and s["n_closed_loops"] == 12
    assert (loops["n_edges"] == 3).all() and (tri_shell == np.arange(12)).all()
    N = normals(verts, tris)
    assert (loops["area_q28"] == np.rint(0.5 * N * TS.Q28).astype(np.int64)).all(), "each loop's vector area is 0.5 N of its triangle"


def test_a_lone_triangles_loop_has_half_its_normal():
    verts, tris = TS.lone_triangle()
    edges, loops, shells, _, s = run(verts, tris)
    assert len(edges) == 3 and len(loops) == 1 and loops[0]["flags"] == T.LOOP_CLOSED
    want = 0.5 * normals(verts, tris)[0] * TS.Q28
    assert np.abs(loops[0]["area_q28"] - want).max() <= 2, "three rounded terms, two of them zero"
    assert abs(int(shells[0]["area_q32"]) - 0.5 * np.linalg.norm(normals(verts, tris)[0]) * TS.Q32) <= 1


def test_sphere_and_box_counts_and_the_boxs_volume():
    verts, tris = PS.sphere_and_box()
    edges, loops, shells, tri_shell, s = run(verts, tris)
    assert (len(tris), s["n_tris_invalid"], s["n_tris_valid"], s["n_tris_far"]) == (2316, 96, 2220, 0)
    assert (s["n_interior"], s["n_boundary"], s["n_nonmanifold"], s["n_miswound"]) == (3234, 192, 0, 0), "the unwelded polar fans are the boundary"
    tight = shells[(shells["flags"] & T.SHELL_WATERTIGHT) != 0]
    box = tight[tight["n_tris"] == 12]
    assert len(box) == 1, "the box is a watertight shell of its own"
    (x0, x1), (y0, y1), (z0, z1) = S.BOX
    want = (x1 - x0) * (y1 - y0) * (z1 - z0)
    assert abs(want - 0.12 * 0.20 * 0.20) < 1e-12
    # 12 terms rounded to 2^-40 m^3, and f32 corners: 1e-7 relative on each side
    assert abs(int(box[0]["volume_q40"]) / TS.Q40 - want) < 3 * 1e-7 * want + 12 * 2.0 ** -40


def test_invalid_and_far_triangles_are_in_no_shell():
    verts, tris = S.soup()
    edges, loops, shells, tri_shell, s = run(verts, tris)
    assert (s["n_tris_invalid"], s["n_tris_far"], s["n_tris_valid"]) == (78, 20, 832 - 78)
    n_used = 832 - 98
    assert len(shells) == n_used == len(loops) and len(edges) == 3 * n_used and int((tri_shell == T.NONE).sum()) == 98
    far = S.cube(lo=TS.FAR_LO)
    assert run(*far)[4]["n_tris_far"] == 12 and len(run(*far)[2]) == 0
    edges, loops, shells, _, s = run(*far, bbox=TS.FAR_BBOX)
    assert s["n_watertight"] == 1 and shells[0]["area_q32"] == 6 * TS.Q32 and abs(int(shells[0]["volume_q40"]) - TS.Q40) <= 12


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_welded_strip_is_one_shell_with_one_closed_rim(n):
    edges, loops, shells, _, s = run(*TS.welded_strip(n))
    assert (s["n_shells"], s["n_loops"], s["n_closed_loops"], s["n_interior"], s["n_boundary"]) == (1, 1, 1, n - 1, n + 2)
    assert shells[0]["area_q32"] == n * int(TS.STRIP_PITCH * TS.STRIP_HALF * TS.Q32)
    if n % 2 == 0:
        assert loops[0]["length_q32"] == n * int(TS.STRIP_PITCH * TS.Q32) + 2 * int(2 * TS.STRIP_HALF * TS.Q32)


def test_components_follow_long_chains():
    n = 5000
    a = np.arange(n - 1)
    label = T.components(n + 3, a + 1, a)  # a path over 0 .. n - 1 and three vertices of their own
    assert (label[:n] == 0).all() and label[n:].tolist() == [n, n + 1, n + 2]
