"""CPU: the render contract (tests/render_ref.py) on hand-built rows with known answers."""
import numpy as np

import hfpf
import render_ref as R

K = (100.0, 100.0, 15.5, 9.5)  # a 32x20 image whose centre pixel is (16, 10) after floor(u + 0.5)
W, H = 32, 20
IDENT = np.hstack([np.eye(3), np.zeros((3, 1))])
RES = 0.002


def rows_of(*specs):
    """specs: (ix, iy, iz, x, y, z, count[, normal[, rgb]]), given in lexicographic voxel order as extract returns them."""
    r = np.zeros(len(specs), dtype=hfpf.ROW_DTYPE)
    for i, s in enumerate(specs):
        r[i]["ix"], r[i]["iy"], r[i]["iz"] = s[:3]
        r[i]["x"], r[i]["y"], r[i]["z"] = s[3:6]
        r[i]["count"] = s[6]
        r[i]["nx"], r[i]["ny"], r[i]["nz"] = s[7] if len(s) > 7 else (0.0, 0.0, -1.0)
        r[i]["rgb"] = s[8] if len(s) > 8 else 0x123456
    return r


def drawn(img):
    return np.argwhere(~np.isnan(img["depth"]))


def test_row_on_the_optical_axis_lands_on_the_principal_point():
    img = R.render(rows_of((0, 0, 0, 0.0, 0.0, 0.5, 3)), IDENT, K, W, H, RES)
    assert drawn(img).tolist() == [[10, 16]]  # (v, u) = (round(9.5), round(15.5)), halves rounding up
    assert img["depth"][10, 16] == np.float32(0.5)
    assert img["count"][10, 16] == 3 and img["rgb"][10, 16] == 0x123456 and img["voxel"][10, 16].tolist() == [0, 0, 0]
    assert img["normal"][10, 16].tolist() == [0.0, 0.0, -1.0]
    # empty pixels
    assert img["count"][0, 0] == 0 and img["rgb"][0, 0] == 0 and img["voxel"][0, 0].tolist() == [-1, -1, -1]
    assert img["depth"].view(np.uint32)[0, 0] == R.NAN_BITS and (img["normal"].view(np.uint32)[0, 0] == R.NAN_BITS).all()


def test_projection_of_an_offset_row():
    # x = 0.1 at z = 0.5: u = (0.1 / 0.5) * 100 + 15.5 = 35.5 -> off the 32-pixel image; x = 0.05: u = 25.5 -> 26
    img = R.render(rows_of((0, 0, 0, 0.05, -0.02, 0.5, 1), (1, 0, 0, 0.1, 0.0, 0.5, 1)), IDENT, K, W, H, RES)
    assert drawn(img).tolist() == [[int(np.floor((-0.02 / 0.5) * 100 + 9.5 + 0.5)), 26]]


def test_a_nearer_row_occludes_whatever_its_index():
    far, near = (0, 0, 0, 0.0, 0.0, 0.8, 1, (0, 0, -1), 0xAA), (5, 5, 5, 0.0, 0.0, 0.4, 1, (0, 0, -1), 0xBB)
    for rows in (rows_of(far, near), rows_of(near, far)):
        img = R.render(rows, IDENT, K, W, H, RES)
        assert img["rgb"][10, 16] == 0xBB and img["depth"][10, 16] == np.float32(0.4)


def test_an_equal_depth_tie_goes_to_the_smaller_voxel():
    a = (1, 2, 3, 0.0, 0.0, 0.5, 4, (0, 0, -1), 0xAA)
    b = (1, 2, 4, 0.0, 0.0, 0.5, 9, (0, 0, -1), 0xBB)
    img = R.render(rows_of(a, b), IDENT, K, W, H, RES)
    assert img["voxel"][10, 16].tolist() == [1, 2, 3] and img["count"][10, 16] == 4
    # depths that differ in f64 but round to the same f32 tie too
    b2 = (1, 2, 4, 0.0, 0.0, float(np.nextafter(0.5, 0.0)), 9, (0, 0, -1), 0xBB)
    assert np.float32(b2[5]) == np.float32(0.5)
    img = R.render(rows_of(a, b2), IDENT, K, W, H, RES)
    assert img["voxel"][10, 16].tolist() == [1, 2, 3]


def test_the_radius_footprint_is_clipped_at_the_borders():
    # pixel (0, 0): u = v = 0 -> x = (0 - 15.5) / 100 * z
    z = 0.5
    row = (0, 0, 0, (0 - 15.5) / 100 * z, (0 - 9.5) / 100 * z, z, 1)
    img = R.render(rows_of(row), IDENT, K, W, H, RES, splat_radius=2)
    got = drawn(img)
    assert sorted(map(tuple, got.tolist())) == [(v, u) for v in range(3) for u in range(3)]
    # a row in the middle gets the full (2r + 1)^2 square
    img = R.render(rows_of((0, 0, 0, 0.0, 0.0, 0.5, 1)), IDENT, K, W, H, RES, splat_radius=3)
    assert len(drawn(img)) == 49 and set(drawn(img)[:, 0]) == set(range(7, 14)) and set(drawn(img)[:, 1]) == set(range(13, 20))


def test_culling_and_z_range():
    facing = (0, 0, 0, 0.0, 0.0, 0.5, 1, (0.0, 0.0, -1.0))
    away = (0, 0, 0, 0.0, 0.0, 0.5, 1, (0.0, 0.0, 1.0))
    for row, want in ((facing, 1), (away, 0)):
        assert len(drawn(R.render(rows_of(row), IDENT, K, W, H, RES, flags=R.CULL_BACKFACES))) == want
        assert len(drawn(R.render(rows_of(row), IDENT, K, W, H, RES))) == 1
    # strict bounds on both ends
    assert len(drawn(R.render(rows_of(facing), IDENT, K, W, H, RES, z_range=(0.5, 1.0)))) == 0
    assert len(drawn(R.render(rows_of(facing), IDENT, K, W, H, RES, z_range=(0.1, 0.5)))) == 0
    assert len(drawn(R.render(rows_of(facing), IDENT, K, W, H, RES, z_range=(0.49, 0.51)))) == 1


def test_min_count_and_empty_rows():
    rows = rows_of((0, 0, 0, 0.0, 0.0, 0.4, 0), (0, 0, 1, 0.0, 0.0, 0.5, 3), (0, 0, 2, 0.0, 0.0, 0.6, 7))
    assert R.render(rows, IDENT, K, W, H, RES)["count"][10, 16] == 3  # count 0 is never drawn
    assert R.render(rows, IDENT, K, W, H, RES, min_count=5)["count"][10, 16] == 7
    assert R.render(rows, IDENT, K, W, H, RES, min_count=7.5)["count"][10, 16] == 0


def test_auto_radius_formula():
    # r = min(max, floor(((0.5 * res) * max(fx, fy)) / zc)): (0.001 * 1000) / 0.25 = 4, / 0.3 = 3.33 -> 3
    assert R.auto_radius(0.002, 1000.0, 900.0, 0.25, 15) == 4
    assert R.auto_radius(0.002, 900.0, 1000.0, 0.3, 15) == 3
    assert R.auto_radius(0.002, 1000.0, 1000.0, 0.25, 2) == 2
    assert R.auto_radius(0.002, 1000.0, 1000.0, 5.0, 15) == 0
    Kb = (1000.0, 900.0, 15.5, 9.5)
    img = R.render(rows_of((0, 0, 0, 0.0, 0.0, 0.3, 1)), IDENT, Kb, W, H, 0.002, splat_radius=-1, max_splat_radius=15)
    assert len(drawn(img)) == 7 * 7
    img = R.render(rows_of((0, 0, 0, 0.0, 0.0, 0.3, 1)), IDENT, Kb, W, H, 0.002, splat_radius=-1, max_splat_radius=1)
    assert len(drawn(img)) == 9


def test_normals_in_the_camera_frame_and_a_rotated_pose():
    # camera at (0, 0, -1) looking along +x of the world: R's columns are the camera axes in the world frame
    Rm = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])  # camera z -> world x, camera x -> world y, camera y -> world z
    pose = np.hstack([Rm, [[0.0], [0.0], [-1.0]]])
    row = (0, 0, 0, 0.5, 0.0, -1.0, 2, (-1.0, 0.0, 0.0))  # 0.5 m in front of the camera, facing it
    img = R.render(rows_of(row), pose, K, W, H, RES, flags=R.CULL_BACKFACES)
    assert img["depth"][10, 16] == np.float32(0.5)
    assert img["normal"][10, 16].tolist() == [0.0, 0.0, -1.0]
    img = R.render(rows_of(row), pose, K, W, H, RES, flags=R.WORLD_NORMALS)
    assert img["normal"][10, 16].tolist() == [-1.0, 0.0, 0.0]
