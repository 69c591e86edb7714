"""CPU: the section contract's numpy restatement (tests/section_ref.py) pinned from first principles on meshes whose sections are known
in closed form, and the binding's mirrors of the records.  The GPU tests compare hfpf_section_mesh* with this restatement byte for
byte; here the restatement itself is held against literal expectations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import plan_support as PS
import section_ref as X
import section_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUBE_V, CUBE_T = S.cube()


def cut(verts, tris, planes, pose=S.IDENT, bbox=S.BBOX):
    sec = S.reference(verts, tris, pose, np.asarray(planes, np.float64).reshape(-1, 4), bbox)
    S.consistent(*sec)
    return sec


def test_the_cube_is_wound_outwards():
    assert S.outward(CUBE_V, CUBE_T, (0.0, 0.0, 0.5)).all()


def test_an_axis_plane_cuts_the_cube_into_one_closed_unit_square():
    points, segments, contours, recs, s = cut(CUBE_V, CUBE_T, [0, 0, 1, 0.25])
    assert (len(points), len(segments), len(contours)) == (8, 8, 1)
    c = contours[0]
    assert c["flags"] == X.CLOSED and c["n_points"] == 8 and c["n_segments"] == 8 and c["n_ends"] == 0 and c["first_point"] == 0
    assert c["area_q28"] == S.Q28 and c["length_q32"] == 4 * S.Q32
    assert (points["ends"] == (1 | 1 << 16)).all() and (points["z"] == np.float32(0.25)).all()
    assert recs[0]["n_closed"] == 1 and recs[0]["area_q28"] == S.Q28 and recs[0]["length_q32"] == 4 * S.Q32
    assert s == dict(n_tris_valid=12, n_tris_invalid=0, n_tris_far=0, n_segments=8, n_points=8, n_contours=1, n_closed=1, reserved=0)


def test_the_area_does_not_depend_on_the_normals_length_or_side():
    a = cut(CUBE_V, CUBE_T, [0, 0, 1, 0.25])
    b = cut(CUBE_V, CUBE_T, [0, 0, -2, -0.5])
    assert a[2][0]["area_q28"] == S.Q28 and b[2][0]["area_q28"] == S.Q28 and b[2][0]["flags"] == X.CLOSED
    assert b[2][0]["length_q32"] == 4 * S.Q32
    # the same points, the segments run the other way round
    assert a[0][["x", "y", "z", "va", "vb"]].tobytes() == b[0][["x", "y", "z", "va", "vb"]].tobytes()
    assert (a[1]["p0"] == b[1]["p1"]).all() and (a[1]["p1"] == b[1]["p0"]).all()


def test_a_closed_outward_mesh_runs_counter_clockwise_seen_from_the_normals_side():
    points, segments, contours, _, _ = cut(CUBE_V, CUBE_T, [0, 0, 1, 0.25])
    P = np.stack([points["x"], points["y"]], axis=1).astype(np.float64)
    shoelace = 0.5 * sum(P[a, 0] * P[b, 1] - P[b, 0] * P[a, 1] for a, b in zip(segments["p0"], segments["p1"]))
    assert shoelace == 1.0


def test_the_diagonal_plane_through_the_centre_is_a_hexagon_with_twelve_points():
    points, segments, contours, _, _ = cut(CUBE_V, CUBE_T, [1, 1, 1, 0.5])
    assert (len(points), len(segments), len(contours)) == (12, 12, 1)
    assert contours[0]["flags"] == X.CLOSED
    # a regular hexagon of side sqrt(2) / 2: perimeter 3 sqrt(2), area 3 sqrt(3) / 4; twelve roundings of half an ulp of q32 / q28 each
    assert abs(int(contours[0]["length_q32"]) - 3 * np.sqrt(2.0) * S.Q32) <= 12
    assert abs(int(contours[0]["area_q28"]) - 0.75 * np.sqrt(3.0) * S.Q28) <= 12


def test_a_plane_through_three_corners_keeps_its_zero_length_segments():
    points, segments, contours, _, _ = cut(CUBE_V, CUBE_T, [1, 1, 1, 1.0])  # through (0.5, 0.5, 0), (0.5, -0.5, 1) and (-0.5, 0.5, 1)
    assert len(contours) == 1 and contours[0]["flags"] == X.CLOSED
    P = np.stack([points[k] for k in "xyz"], axis=1)
    zero = (P[segments["p0"]] == P[segments["p1"]]).all(axis=1)
    assert zero.any() and not zero.all(), "zero-length segments at the corners, real ones across the faces"
    # the triangle with corners at those three: side sqrt(2), area sqrt(3) / 2
    assert abs(int(contours[0]["area_q28"]) - 0.5 * np.sqrt(3.0) * S.Q28) <= len(segments)
    assert abs(int(contours[0]["length_q32"]) - 3 * np.sqrt(2.0) * S.Q32) <= len(segments)


def test_a_plane_on_a_face_gives_nothing():
    points, segments, contours, recs, s = cut(CUBE_V, CUBE_T, [0, 0, 1, 0.0])  # s == 0 on the bottom face is outside, as everything above
    assert len(points) == len(segments) == len(contours) == 0 and s["n_segments"] == 0 and s["n_tris_valid"] == 12
    assert recs.tobytes() == bytes(64)


def test_three_triangles_on_one_edge_are_branched():
    points, segments, contours, _, _ = cut(*S.fan(3), [0, 0, 1, 0.5])
    assert len(contours) == 1 and len(segments) == 3 and len(points) == 4
    assert contours[0]["flags"] == X.BRANCHED and contours[0]["n_ends"] == 3
    shared = points[(points["va"] == 0) & (points["vb"] == 1)][0]
    assert shared["ends"] in (3, 3 << 16), "three segments start (or three end) at the point on the shared edge"


def test_two_triangles_of_opposite_winding_meet_with_n_in_two():
    points, segments, contours, _, _ = cut(*S.bow(), [0, 0, 1, 0.5])
    assert len(contours) == 1 and len(segments) == 2 and len(points) == 3
    shared = points[(points["va"] == 0) & (points["vb"] == 1)][0]
    assert shared["ends"] == 2 << 16, "both segments end at the shared point: n_in == 2, n_out == 0"
    assert contours[0]["flags"] == X.BRANCHED and contours[0]["n_ends"] == 2
    # the same two triangles wound consistently: an open chain, not branched
    v, t = S.bow()
    t[1] = t[1][[1, 0, 2]]
    points, segments, contours, _, _ = cut(v, t, [0, 0, 1, 0.5])
    assert contours[0]["flags"] == 0 and contours[0]["n_ends"] == 2 and len(points) == 3


def test_an_unwelded_soup_gives_one_open_contour_per_segment():
    v, t = S.unweld(CUBE_V, CUBE_T)
    points, segments, contours, _, s = cut(v, t, [0, 0, 1, 0.25])
    assert len(segments) == 8 and len(contours) == 8 and len(points) == 16 and s["n_closed"] == 0
    assert (contours["n_ends"] == 2).all() and (contours["flags"] == 0).all() and (contours["n_segments"] == 1).all()
    assert int(contours["length_q32"].sum()) == 4 * S.Q32  # equal coordinates are not merged, the geometry is the same


def test_invalid_and_far_triangles_are_counted_and_skipped():
    v, t = S.cube()
    v = np.concatenate([v, [[np.nan, 0, 0], [40.0, 0.0, 0.5]]]).astype(np.float32)
    t = np.concatenate([t, [[0, 1, 99], [0, 1, 8], [0, 0, 1], [0, 1, 9]]]).astype(np.uint32)  # index, NaN, repeated; far
    s = cut(v, t, [0, 0, 1, 0.25])[4]
    assert (s["n_tris_valid"], s["n_tris_invalid"], s["n_tris_far"], s["n_segments"]) == (13, 3, 1, 8)
    # exactly 32 m from the centre of the box is not in range
    v[9] = (32.0, 0.0, 0.5)
    assert cut(v, t, [0, 0, 1, 0.25])[4]["n_tris_far"] == 1
    v[9] = (np.nextafter(np.float32(32.0), np.float32(0.0)), 0.0, 0.5)
    s = cut(v, t, [0, 0, 1, 0.25])[4]
    assert s["n_tris_far"] == 0 and s["n_segments"] == 9


def test_areas_are_taken_about_the_representative_far_from_the_origin():
    shift = np.array([1024.0, -512.0, 256.0])
    v, t = S.cube(lo=tuple(shift + (-0.5, -0.5, 0.0)))
    bbox = (1023.5, 1024.5, -512.5, -511.5, 256.0, 257.0)
    c = cut(v, t, [0, 0, 1, 256.25], bbox=bbox)[2]
    assert len(c) == 1 and c[0]["flags"] == X.CLOSED and c[0]["area_q28"] == S.Q28 and c[0]["length_q32"] == 4 * S.Q32
    assert cut(v, t, [0, 0, 1, 256.25], bbox=S.BBOX)[4]["n_tris_far"] == 12


SHAPE_V, SHAPE_T = PS.sphere_and_box()


@pytest.mark.parametrize("planes", [S.parallel_planes(1), S.parallel_planes(64), S.parallel_planes(65), S.mixed_planes(65)], ids=["1", "64", "65", "mixed"])
def test_the_closed_sphere_and_box_give_closed_contours_only(planes):
    points, segments, contours, recs, s = cut(SHAPE_V, SHAPE_T, planes)
    assert s["n_tris_invalid"] == 2 * 48, "the polar triangles"
    assert len(contours) > 0 and (contours["flags"] == X.CLOSED).all() and s["n_closed"] == len(contours)
    assert (contours["area_q28"] > 0).all(), "outward winding: every section runs counter-clockwise about its plane's normal"
    assert recs["n_contours"].max() == 2, "a plane that meets both shapes"
    if len(planes) > 1:
        assert (recs["n_contours"] == 0).any(), "a plane that misses everything"


def test_sixty_five_planes_cut_down_to_sixty_four():
    a = cut(SHAPE_V, SHAPE_T, S.mixed_planes(65))
    b = cut(SHAPE_V, SHAPE_T, S.mixed_planes(65)[:64])
    for x, y in zip(S.cut_to_planes(a, 64), b[:4]):
        assert x.tobytes() == y.tobytes()


def test_a_sphere_section_has_the_circles_area():
    (cx, cy, cz), r = PS.SPHERE
    c = cut(SHAPE_V, SHAPE_T[:2 * 24 * 48], [0, 1, 0, 0.03])[2]  # the sphere alone, 3 cm above its centre
    assert len(c) == 1
    circle = np.pi * (r * r - 0.03 ** 2)
    assert 0.98 * circle < c[0]["area_q28"] / S.Q28 < circle, "a polygon inscribed in a slightly smaller circle"


def test_struct_sizes_and_mirrors(hfpf_mod):
    H = hfpf_mod
    for mine, theirs in ((X.POINT_DTYPE, H.SECTION_POINT_DTYPE), (X.SEGMENT_DTYPE, H.SECTION_SEGMENT_DTYPE), (X.CONTOUR_DTYPE, H.SECTION_CONTOUR_DTYPE),
                         (X.PLANE_DTYPE, H.SECTION_PLANE_DTYPE)):
        assert mine == theirs
    assert (H.SECTION_CLOSED, H.SECTION_BRANCHED) == (X.CLOSED, X.BRANCHED)
    assert (H.SECTION_MAX_PLANES, H.SECTION_MAX_PLANE_SEGMENTS) == (X.MAX_PLANES, X.MAX_PLANE_SEGMENTS)
    hdr = open(os.path.join(ROOT, "include", "hfpf.h")).read()
    for name, size in (("hfpf_section_opts", C.sizeof(H.SectionOpts)), ("hfpf_section_point", 32), ("hfpf_section_segment", 16), ("hfpf_section_contour", 48),
                       ("hfpf_section_plane", 64), ("hfpf_section_summary", C.sizeof(H.SectionSummary))):
        assert re.search(r"static_assert\(sizeof\(%s\) == %d," % (name, size), hdr), name
    assert tuple(k for k, _ in H.SectionSummary._fields_) == X.SUMMARY_KEYS


def test_check_section_opts_rejects_every_bad_field(hfpf_mod):
    H = hfpf_mod
    assert H.check_section_opts(H.section_opts()) == 0
    assert H.check_section_opts(None) == -2
    for field, value in (("struct_size", 12), ("flags", 1), ("reserved", 1)):
        o = H.section_opts()
        setattr(o, field, value)
        assert H.check_section_opts(o) == -2, field
