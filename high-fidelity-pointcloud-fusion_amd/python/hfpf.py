"""ctypes binding of libhfpf.so (include/hfpf.h) -- the host-side mirror used by tests and bench.py.

`OccupancyGrid` mirrors the public members of the reference's `class OccupancyGrid`
(pointcloud_fusion/pointcloud_fusion/include/utilities/OccupancyGrid.hpp:99-136) as the node uses them
(.../src/pointcloud_fusion_and_filter.cpp:161-164,293,311,398,438): construct, addPoints (here `integrate`,
which also folds in the decode / z-clip / transform of the capture threads), state_changed,
updateThicknessVectors (`clean`), downloadData (`extract` / `download_data`), clearVoxels (`clear`).

There is no CPU path: constructing a grid raises HfpfError when libhfpf.so is missing or no HIP device
is usable.  This module never imports the oracle.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.dirname(_HERE)
CSRC_DIR = os.path.join(PKG_DIR, "csrc")
LIB_PATH = os.environ.get("HFPF_LIB") or os.path.join(CSRC_DIR, "libhfpf.so")  # HFPF_LIB: A/B builds during tuning

FLAG_FUSE_COLOR = 1
FLAG_PCL_SHIFTED_COV = 2
FLAG_DIRECT_UPDATE = 4
STATUS = {0: "OK", -1: "BAD_CONFIG", -2: "BAD_ARG", -3: "CAPACITY", -4: "HIP", -5: "STATE", -6: "IO", -7: "DIST"}


class HfpfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("hfpf status %d (%s): %s" % (code, STATUS.get(code, "?"), msg))
        self.code = code


def _sized(cls):
    """A structure of the C ABI with its struct_size filled in."""
    r = cls()
    r.struct_size = C.sizeof(cls)
    return r


def _or(opts, make, *a, **kw):
    """The caller's ready `opts`, or make(*a, **kw) without one."""
    return opts if opts is not None else make(*a, **kw)


def _opts_checker(kind):
    """The module-level check_<kind>_opts(o) of hfpf_check_<kind>_opts."""
    def check(o):
        return getattr(lib(), "hfpf_check_%s_opts" % kind)(C.byref(o) if o is not None else None)
    check.__name__ = check.__qualname__ = "check_%s_opts" % kind
    check.__doc__ = "hfpf_check_%s_opts: 0 (HFPF_OK) or the error code (host code, no handle, no GPU needed)." % kind
    return check


class _Record(C.Structure):
    """A summary or result structure of the C ABI: as_dict() gives its fields (those DICT_FIELDS names, or all)."""
    DICT_FIELDS = None

    def as_dict(self):
        return {k: getattr(self, k) for k in self.DICT_FIELDS or [n for n, _ in self._fields_]}


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("resolution", C.c_float),
        ("bbox", C.c_double * 6),
        ("k", C.c_int32),
        ("K", C.c_int32),
        ("gate", C.c_int32),
        ("cylinder_radius", C.c_double),
        ("ball_radius", C.c_double),
        ("z_clip_min", C.c_double),
        ("z_clip_max", C.c_double),
        ("device", C.c_int32),
        ("flags", C.c_uint32),
        ("max_bricks", C.c_uint64),
        ("max_log_points", C.c_uint64),
        ("max_normals", C.c_uint64),
        ("max_frames", C.c_uint64),
        ("frame_width", C.c_uint32),
        ("reserved0", C.c_uint32),
        ("max_call_points", C.c_uint64),
    ]


class ExtractOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("classify_threshold", C.c_int32), ("min_count", C.c_double),
                ("paint_white", C.c_int32), ("reserved0", C.c_int32)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "points_presented", "points_zclip_pass", "points_in_bbox", "points_buffered", "dep_pairs_tested",
        "dep_pairs_member", "voxels_occupied", "voxels_with_normal", "bricks_allocated", "registrations",
        "dep_entries", "frames_integrated", "clean_passes", "device_bytes", "replay_members", "points_direct", "table_misses", "update_extra_rounds")]


ROW_DTYPE = np.dtype(
    [
        ("ix", "<i4"), ("iy", "<i4"), ("iz", "<i4"), ("count", "<u4"),
        ("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
        ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
        ("sdx", "<f4"), ("sdy", "<f4"), ("sdz", "<f4"),
        ("mean_dist", "<f4"), ("sd_dist", "<f4"), ("rgb", "<u4"),
    ]
)

# every symbol include/hfpf.h and include/hfpf_probe.h declare
EXPORTS = [
    "hfpf_default_config", "hfpf_abi_version", "hfpf_create", "hfpf_destroy", "hfpf_last_error", "hfpf_get_dims",
    "hfpf_integrate", "hfpf_integrate_pinned", "hfpf_host_alloc", "hfpf_host_free", "hfpf_integrate_device", "hfpf_is_dirty", "hfpf_clean", "hfpf_extract", "hfpf_extract_filtered", "hfpf_free_rows",
    "hfpf_write_pcd", "hfpf_write_meta_csv", "hfpf_write_pcd_xyzrgb", "hfpf_write_pcd_binary", "hfpf_clear", "hfpf_sync", "hfpf_get_counters", "hfpf_get_occupied",
    "hfpf_device_alloc", "hfpf_device_free", "hfpf_device_upload", "hfpf_kernel_timing", "hfpf_get_kernel_time",
    "hfpf_probe_points", "hfpf_probe_normals", "hfpf_probe_project", "hfpf_probe_trig",
    "hfpf_dist_unique_id", "hfpf_dist_init", "hfpf_dist_info", "hfpf_dist_disable", "hfpf_epoch_export", "hfpf_epoch_import", "hfpf_stats_export",
    "hfpf_extract_with_stats", "hfpf_device_download", "hfpf_device_copy", "hfpf_epoch_import_gathered",
    "hfpf_integrate_depth", "hfpf_integrate_depth_pinned", "hfpf_integrate_depth_device", "hfpf_probe_depth",
    "hfpf_render", "hfpf_render_device",
    "hfpf_track_depth", "hfpf_track_depth_device", "hfpf_track",
    "hfpf_query", "hfpf_query_device", "hfpf_query_depth",
    "hfpf_extract_mesh", "hfpf_extract_mesh_device", "hfpf_free_mesh", "hfpf_write_ply", "hfpf_check_mesh_opts",
    "hfpf_check_component_opts", "hfpf_extract_components", "hfpf_extract_components_device", "hfpf_free_components",
    "hfpf_check_deviation_opts", "hfpf_compare_mesh", "hfpf_compare_mesh_device", "hfpf_free_deviation", "hfpf_read_ply",
    "hfpf_check_align_opts", "hfpf_align_mesh", "hfpf_align_mesh_device",
    "hfpf_check_cover_opts", "hfpf_cover_mesh", "hfpf_cover_mesh_device", "hfpf_free_coverage",
    "hfpf_check_plan_opts", "hfpf_plan_views", "hfpf_plan_views_device", "hfpf_free_plan",
    "hfpf_check_section_opts", "hfpf_section_mesh", "hfpf_section_mesh_device", "hfpf_free_section",
    "hfpf_check_topology_opts", "hfpf_mesh_topology", "hfpf_mesh_topology_device", "hfpf_free_topology",
    "hfpf_check_consistency_opts", "hfpf_depth_consistency", "hfpf_depth_consistency_device", "hfpf_free_consistency",
    "hfpf_check_hide_opts", "hfpf_hide_voxels", "hfpf_hide_voxels_device", "hfpf_hide_box", "hfpf_show_all", "hfpf_get_hidden",
    "hfpf_check_raycast_opts", "hfpf_raycast", "hfpf_raycast_device", "hfpf_raycast_view", "hfpf_raycast_view_device",
    "hfpf_snapshot", "hfpf_free_snapshot", "hfpf_restore", "hfpf_save", "hfpf_load", "hfpf_snapshot_info", "hfpf_config_from_snapshot",
]

# hfpf_depth_image formats (include/hfpf.h)
DEPTH_U16, DEPTH_F32 = 1, 2
COLOR_NONE, COLOR_RGB8, COLOR_BGR8, COLOR_RGBA8, COLOR_BGRA8 = 0, 1, 2, 3, 4
COLOR_BPP = {COLOR_NONE: 0, COLOR_RGB8: 3, COLOR_BGR8: 3, COLOR_RGBA8: 4, COLOR_BGRA8: 4}


class DepthImage(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("depth_format", C.c_uint32),
                ("depth_step", C.c_uint32), ("depth_scale", C.c_float), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("color_format", C.c_uint32), ("color_step", C.c_uint32),
                ("reserved", C.c_uint64)]


def depth_desc(width, height, depth_format, depth_step, K, color_format=COLOR_NONE, color_step=0, depth_scale=0.001):
    """An hfpf_depth_image; K = (fx, fy, cx, cy)."""
    d = _sized(DepthImage)
    d.width, d.height, d.depth_format, d.depth_step = width, height, depth_format, depth_step
    d.depth_scale = depth_scale
    d.fx, d.fy, d.cx, d.cy = (float(k) for k in K)
    d.color_format, d.color_step = color_format, color_step
    return d


def _image_desc(depth, K, color, color_format, depth_scale):
    """Descriptor of numpy images: the depth dtype picks the format (uint16 counts / float32 metres), the row strides give the
    steps (rows may be padded: a view of a wider array), a 3- or 4-channel uint8 colour image defaults to RGB8 / RGBA8."""
    if depth.ndim != 2 or depth.dtype not in (np.uint16, np.float32) or depth.strides[1] != depth.itemsize:
        raise ValueError("depth must be a 2-D uint16 or float32 image with contiguous rows")
    fmt = DEPTH_U16 if depth.dtype == np.uint16 else DEPTH_F32
    H, W = depth.shape
    cstep = 0
    if color is None:
        color_format = COLOR_NONE
    else:
        if color.dtype != np.uint8 or color.ndim != 3 or color.shape[:2] != depth.shape or color.strides[2] != 1 or color.strides[1] != color.shape[2]:
            raise ValueError("color must be a HxWx3 or HxWx4 uint8 image with contiguous rows, the size of the depth image")
        if color_format is None:
            color_format = COLOR_RGB8 if color.shape[2] == 3 else COLOR_RGBA8
        if COLOR_BPP.get(color_format) != color.shape[2]:
            raise ValueError("color_format %r does not match a %d-channel image" % (color_format, color.shape[2]))
        cstep = color.strides[0]
    return depth_desc(W, H, fmt, depth.strides[0], K, color_format, cstep, depth_scale)

# hfpf_render_opts.flags (include/hfpf.h)
RENDER_CULL_BACKFACES = 1
RENDER_WORLD_NORMALS = 2
# render planes: (name, numpy dtype, channels); empty pixels hold NaN (depth, normal), 0 (rgb, count) or -1 (voxel)
RENDER_PLANES = (("depth", np.float32, 1), ("normal", np.float32, 3), ("rgb", np.uint32, 1), ("count", np.uint32, 1), ("voxel", np.int32, 3))


class RenderOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("z_near", C.c_double), ("z_far", C.c_double), ("min_count", C.c_double),
                ("splat_radius", C.c_int32), ("max_splat_radius", C.c_int32), ("reserved", C.c_uint64)]


class RenderPlanes(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _, _ in RENDER_PLANES]


def render_opts(K, width, height, z_range=(0.01, 100.0), min_count=0.0, splat_radius=0, max_splat_radius=4, cull_backfaces=False,
                world_normals=False):
    """An hfpf_render_opts; K = (fx, fy, cx, cy), splat_radius -1 = auto (capped at max_splat_radius)."""
    o = _sized(RenderOpts)
    o.width, o.height = int(width), int(height)
    o.flags = (RENDER_CULL_BACKFACES if cull_backfaces else 0) | (RENDER_WORLD_NORMALS if world_normals else 0)
    o.fx, o.fy, o.cx, o.cy = (float(k) for k in K)
    o.z_near, o.z_far = (float(z) for z in z_range)
    o.min_count = float(min_count)
    o.splat_radius, o.max_splat_radius = int(splat_radius), int(max_splat_radius)
    return o


# hfpf_track_result.flags (include/hfpf.h)
TRACK_CONVERGED, TRACK_DEGENERATE, TRACK_TOO_FEW = 1, 2, 4


class TrackOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_iterations", C.c_uint32), ("stride", C.c_uint32), ("min_inliers", C.c_uint32),
                ("view", RenderOpts), ("max_distance", C.c_double), ("damping", C.c_double), ("eps_rotation", C.c_double),
                ("eps_translation", C.c_double), ("reserved", C.c_uint64)]


class TrackResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("points_used", C.c_uint64), ("inliers", C.c_uint64), ("rms", C.c_double), ("information", C.c_double * 36),
                ("pose", C.c_double * 12)]


def track_opts(K, width, height, max_iterations=10, stride=1, min_inliers=6, max_distance=0.02, damping=1e-6, eps_rotation=1e-6,
               eps_translation=1e-6, z_range=(0.01, 100.0), min_count=0.0, splat_radius=-1, max_splat_radius=4, cull_backfaces=True):
    """An hfpf_track_opts; the view is a render_opts of (K, width, height) with the view keywords."""
    o = _sized(TrackOpts)
    o.max_iterations, o.stride, o.min_inliers = int(max_iterations), int(stride), int(min_inliers)
    o.view = render_opts(K, width, height, z_range=z_range, min_count=min_count, splat_radius=splat_radius,
                         max_splat_radius=max_splat_radius, cull_backfaces=cull_backfaces)
    o.max_distance, o.damping = float(max_distance), float(damping)
    o.eps_rotation, o.eps_translation = float(eps_rotation), float(eps_translation)
    return o


def track_result():
    return _sized(TrackResult)


def _refine_out(r, own):
    """The result dict of an hfpf_track_result or hfpf_align_result; own names the field only that one has."""
    return {"iterations": r.iterations, "flags": r.flags, own: getattr(r, own), "inliers": r.inliers, "rms": r.rms,
            "information": np.array(r.information[:], np.float64).reshape(6, 6), "pose": np.array(r.pose[:], np.float64).reshape(3, 4)}


def _track_out(r):
    """(3x4 pose, result dict) of an hfpf_track_result."""
    out = _refine_out(r, "points_used")
    return out["pose"], out


# hfpf_query_opts.flags and hfpf_query_hit.flags (include/hfpf.h)
QUERY_ZCLIP = 1
QHIT_USED, QHIT_IN_BBOX, QHIT_OCCUPIED, QHIT_HAS_ROW, QHIT_FOUND = 1, 2, 4, 8, 16
QUERY_HIT_DTYPE = np.dtype([("voxel", "<i4", (3,)), ("flags", "<u4"), ("row_voxel", "<i4", (3,)), ("row_count", "<u4"),
                            ("p", "<f4", (3,)), ("distance", "<f4"), ("signed_distance", "<f4"), ("reserved", "<u4", (3,))])
assert QUERY_HIT_DTYPE.itemsize == 64


class QueryOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("radius", C.c_int32), ("reserved0", C.c_int32),
                ("min_count", C.c_double), ("max_distance", C.c_double), ("reserved", C.c_uint64)]


def query_opts(radius=1, min_count=0.0, max_distance=float("inf"), zclip=False):
    """An hfpf_query_opts: the (2 radius + 1)^3 voxel window, the count and distance gates, HFPF_QUERY_ZCLIP."""
    o = _sized(QueryOpts)
    o.flags = QUERY_ZCLIP if zclip else 0
    o.radius = int(radius)
    o.min_count, o.max_distance = float(min_count), float(max_distance)
    return o


class MeshOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("radius", C.c_int32), ("min_count", C.c_double), ("max_distance", C.c_double),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


# hfpf_mesh_vertex (include/hfpf.h); triangles are (n, 3) uint32 vertex indices
MESH_VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("rgb", "<u4"),
                              ("count", "<u4")])
assert MESH_VERTEX_DTYPE.itemsize == 32


def mesh_opts(radius=2, min_count=0.0, max_distance=float("inf")):
    """An hfpf_mesh_opts: the query window of the corner samples (1..4), the count gate and the distance gate."""
    o = _sized(MeshOpts)
    o.radius = int(radius)
    o.min_count, o.max_distance = float(min_count), float(max_distance)
    return o


class ComponentOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("reach", C.c_int32), ("reserved0", C.c_int32),
                ("min_count", C.c_double), ("min_normal_dot", C.c_double), ("min_rows", C.c_uint32), ("keep_largest", C.c_uint32),
                ("min_points", C.c_uint64), ("reserved", C.c_uint64)]


# hfpf_component (include/hfpf.h)
COMPONENT_DTYPE = np.dtype([("first_row", "<u4"), ("n_rows", "<u4"), ("points", "<u8"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)),
                            ("source_row", "<u4"), ("reserved", "<u4")])
assert COMPONENT_DTYPE.itemsize == 48


def component_opts(reach=1, min_count=0.0, min_normal_dot=-2.0, min_rows=0, min_points=0, keep_largest=0):
    """An hfpf_component_opts: the neighbour reach in voxels (1..4), the count gate of the row set, the normal gate of an edge (-2 =
    off) and the three keep tests of a component (0 = off)."""
    o = _sized(ComponentOpts)
    o.reach = int(reach)
    o.min_count, o.min_normal_dot = float(min_count), float(min_normal_dot)
    o.min_rows, o.keep_largest, o.min_points = int(min_rows), int(keep_largest), int(min_points)
    return o


check_component_opts = _opts_checker("component")


class DeviationOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("min_count", C.c_double), ("max_distance", C.c_double),
                ("reserved", C.c_uint64)]


class DeviationSummary(_Record):
    _fields_ = [("n_rows", C.c_uint64), ("n_found", C.c_uint64), ("n_negative", C.c_uint64), ("n_tris_valid", C.c_uint64),
                ("n_tris_invalid", C.c_uint64), ("max_abs", C.c_float), ("pad", C.c_uint32), ("sum_abs_q30", C.c_int64),
                ("sum_sq_q30", C.c_int64)]


# hfpf_deviation and its flags (include/hfpf.h)
DEV_FOUND, DEV_ON_EDGE, DEV_ON_VERTEX = 1, 2, 4
DEVIATION_DTYPE = np.dtype([("signed_distance", "<f4"), ("distance", "<f4"), ("tri", "<u4"), ("flags", "<u4"), ("q", "<f4", (3,)),
                            ("reserved", "<u4")])
assert DEVIATION_DTYPE.itemsize == 32


def deviation_opts(min_count=0.0, max_distance=0.01):
    """An hfpf_deviation_opts: the count gate of the row set and the largest distance (metres, at most 32 voxels) a winner may have."""
    o = _sized(DeviationOpts)
    o.min_count, o.max_distance = float(min_count), float(max_distance)
    return o


check_deviation_opts = _opts_checker("deviation")


# hfpf_align_result.flags and hfpf_align_opts.flags (include/hfpf.h)
ALIGN_CONVERGED, ALIGN_DEGENERATE, ALIGN_TOO_FEW = 1, 2, 4
ALIGN_SKIP_BOUNDARY = 1


class AlignOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("max_iterations", C.c_uint32), ("stride", C.c_uint32),
                ("min_inliers", C.c_uint32), ("reserved0", C.c_uint32), ("compare", DeviationOpts), ("damping", C.c_double),
                ("eps_rotation", C.c_double), ("eps_translation", C.c_double), ("reserved", C.c_uint64)]


class AlignResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("rows_sampled", C.c_uint64), ("inliers", C.c_uint64), ("rms", C.c_double), ("information", C.c_double * 36),
                ("pose", C.c_double * 12)]


assert C.sizeof(AlignOpts) == 88 and C.sizeof(AlignResult) == 424


def align_opts(max_iterations=10, stride=1, min_inliers=6, min_count=0.0, max_distance=0.01, damping=1e-6, eps_rotation=1e-6,
               eps_translation=1e-6, skip_boundary=False):
    """An hfpf_align_opts; min_count and max_distance (the capture range, at most 32 voxels) fill the embedded hfpf_deviation_opts."""
    o = _sized(AlignOpts)
    o.flags = ALIGN_SKIP_BOUNDARY if skip_boundary else 0
    o.max_iterations, o.stride, o.min_inliers = int(max_iterations), int(stride), int(min_inliers)
    o.compare = deviation_opts(min_count, max_distance)
    o.damping, o.eps_rotation, o.eps_translation = float(damping), float(eps_rotation), float(eps_translation)
    return o


def align_result():
    return _sized(AlignResult)


check_align_opts = _opts_checker("align")


# hfpf_tri_coverage.flags, hfpf_cover_opts.flags and hfpf_tri_coverage (include/hfpf.h)
COV_VALID, COV_CAPPED, COV_HUGE = 1, 2, 4
COVER_ABS_NORMAL = 1
TRI_COVERAGE_DTYPE = np.dtype([("n_samples", "<u4"), ("n_in_bbox", "<u4"), ("n_covered", "<u4"), ("flags", "<u4"), ("area", "<f4"),
                               ("max_distance", "<f4"), ("sum_dist_q30", "<i8")])
assert TRI_COVERAGE_DTYPE.itemsize == 32


class CoverOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("radius", C.c_int32), ("max_subdivision", C.c_uint32),
                ("min_count", C.c_double), ("max_distance", C.c_double), ("spacing", C.c_double), ("min_normal_dot", C.c_double),
                ("reserved", C.c_uint64)]


class CoverageSummary(_Record):
    _fields_ = [(k, C.c_uint64) for k in ("n_tris_valid", "n_tris_invalid", "n_tris_huge", "n_samples", "n_in_bbox", "n_covered")] + [
        ("sum_dist_q30", C.c_int64), ("area_q40_lo", C.c_uint64), ("area_q40_hi", C.c_uint64), ("covered_q40_lo", C.c_uint64),
        ("covered_q40_hi", C.c_uint64), ("max_distance", C.c_float), ("pad", C.c_uint32)]

    def as_dict(self):
        """The fields, and the two areas in m^2 the q40 words stand for: area and covered_area."""
        d = super().as_dict()
        d["area"] = ((d["area_q40_hi"] << 32) + d["area_q40_lo"]) / 2.0 ** 40
        d["covered_area"] = ((d["covered_q40_hi"] << 32) + d["covered_q40_lo"]) / 2.0 ** 40
        return d


assert C.sizeof(CoverOpts) == 56 and C.sizeof(CoverageSummary) == 96


def cover_opts(radius=2, min_count=0.0, max_distance=0.01, spacing=0.005, max_subdivision=64, min_normal_dot=-2.0, abs_normal=False):
    """An hfpf_cover_opts: the sample test's voxel window, count gate and largest distance (metres), the sample spacing (metres) and
    its cap, and the normal gate (-2 = off; abs_normal passes either orientation)."""
    o = _sized(CoverOpts)
    o.flags = COVER_ABS_NORMAL if abs_normal else 0
    o.radius, o.max_subdivision = int(radius), int(max_subdivision)
    o.min_count, o.max_distance, o.spacing, o.min_normal_dot = float(min_count), float(max_distance), float(spacing), float(min_normal_dot)
    return o


check_cover_opts = _opts_checker("cover")


# hfpf_section_contour.flags and the section records (include/hfpf.h)
SECTION_CLOSED, SECTION_BRANCHED = 1, 2
SECTION_MAX_PLANES, SECTION_MAX_PLANE_SEGMENTS = 4096, 1 << 20
SECTION_POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("plane", "<u4"), ("va", "<u4"), ("vb", "<u4"), ("contour", "<u4"),
                                ("ends", "<u4")])
SECTION_SEGMENT_DTYPE = np.dtype([("p0", "<u4"), ("p1", "<u4"), ("tri", "<u4"), ("contour", "<u4")])
SECTION_CONTOUR_DTYPE = np.dtype([("plane", "<u4"), ("first_point", "<u4"), ("n_points", "<u4"), ("n_segments", "<u4"), ("n_ends", "<u4"),
                                  ("flags", "<u4"), ("length_q32", "<i8"), ("area_q28", "<i8"), ("reserved", "<u8")])
SECTION_PLANE_DTYPE = np.dtype([("first_segment", "<u4"), ("n_segments", "<u4"), ("first_point", "<u4"), ("n_points", "<u4"),
                                ("first_contour", "<u4"), ("n_contours", "<u4"), ("n_closed", "<u4"), ("n_branched", "<u4"),
                                ("length_q32", "<i8"), ("area_q28", "<i8"), ("reserved", "<u8", (2,))])
assert (SECTION_POINT_DTYPE.itemsize, SECTION_SEGMENT_DTYPE.itemsize, SECTION_CONTOUR_DTYPE.itemsize, SECTION_PLANE_DTYPE.itemsize) == (32, 16, 48, 64)


class SectionOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint64)]


class SectionSummary(_Record):
    _fields_ = [(k, C.c_uint64) for k in ("n_tris_valid", "n_tris_invalid", "n_tris_far", "n_segments", "n_points", "n_contours", "n_closed",
                                          "reserved")]


assert C.sizeof(SectionOpts) == 16 and C.sizeof(SectionSummary) == 64


def section_opts():
    """An hfpf_section_opts (it has no settings yet)."""
    return _sized(SectionOpts)


check_section_opts = _opts_checker("section")


# hfpf_topology_edge.kind, the loops' and the shells' flags and the topology records (include/hfpf.h)
TOPOLOGY_BOUNDARY, TOPOLOGY_NONMANIFOLD, TOPOLOGY_MISWOUND = 1, 2, 3
TOPOLOGY_LOOP_CLOSED, TOPOLOGY_LOOP_BRANCHED = 1, 2
TOPOLOGY_SHELL_OPEN, TOPOLOGY_SHELL_NONMANIFOLD, TOPOLOGY_SHELL_MISWOUND, TOPOLOGY_SHELL_WATERTIGHT = 1, 2, 4, 8
TOPOLOGY_NONE, TOPOLOGY_MAX_VERTS = 0xFFFFFFFF, 1 << 26
TOPOLOGY_EDGE_DTYPE = np.dtype([("p0", "<u4"), ("p1", "<u4"), ("tri", "<u4"), ("kind", "<u4"), ("uses", "<u4"), ("loop", "<u4"), ("shell", "<u4"),
                                ("reserved", "<u4")])
TOPOLOGY_LOOP_DTYPE = np.dtype([("first_vertex", "<u4"), ("n_verts", "<u4"), ("n_edges", "<u4"), ("n_ends", "<u4"), ("flags", "<u4"),
                                ("shell", "<u4"), ("length_q32", "<i8"), ("area_q28", "<i8", (3,)), ("reserved", "<u8")])
TOPOLOGY_SHELL_DTYPE = np.dtype([("first_vertex", "<u4"), ("n_verts", "<u4"), ("n_tris", "<u4"), ("flags", "<u4"), ("n_edges", "<u4"),
                                 ("n_boundary", "<u4"), ("n_nonmanifold", "<u4"), ("n_miswound", "<u4"), ("n_loops", "<u4"), ("reserved0", "<u4"),
                                 ("area_q32", "<i8"), ("volume_q40", "<i8"), ("reserved", "<u8")])
assert (TOPOLOGY_EDGE_DTYPE.itemsize, TOPOLOGY_LOOP_DTYPE.itemsize, TOPOLOGY_SHELL_DTYPE.itemsize) == (32, 64, 64)


class TopologyOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint64)]


class TopologySummary(_Record):
    _fields_ = [(k, C.c_uint64) for k in ("n_tris_valid", "n_tris_invalid", "n_tris_far", "n_verts_used", "n_edges", "n_interior", "n_boundary",
                                          "n_nonmanifold", "n_miswound", "n_loops", "n_closed_loops", "n_shells", "n_watertight")] + [
        ("reserved", C.c_uint64 * 3)]
    DICT_FIELDS = [k for k, _ in _fields_[:13]]


assert C.sizeof(TopologyOpts) == 16 and C.sizeof(TopologySummary) == 128


def topology_opts():
    """An hfpf_topology_opts (it has no settings yet)."""
    return _sized(TopologyOpts)


check_topology_opts = _opts_checker("topology")


# hfpf_plan_opts.flags, hfpf_view_score and hfpf_tri_plan (include/hfpf.h)
PLAN_TWO_SIDED, PLAN_MODEL_OCCLUDES = 1, 2
VIEW_SCORE_DTYPE = np.dtype([("rank", "<i4"), ("n_in_view", "<u4"), ("n_facing", "<u4"), ("n_visible", "<u4"), ("visible_q40", "<u8"),
                             ("gain_q40", "<u8"), ("gain_samples", "<u8")])
TRI_PLAN_DTYPE = np.dtype([("n_targets", "<u4"), ("n_reachable", "<u4"), ("n_planned", "<u4"), ("flags", "<u4")])
assert VIEW_SCORE_DTYPE.itemsize == 40 and TRI_PLAN_DTYPE.itemsize == 16


class PlanOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("cover", CoverOpts), ("view", RenderOpts),
                ("occluder_near", C.c_double), ("min_cos", C.c_double), ("tolerance", C.c_double), ("slope", C.c_double),
                ("min_gain_q40", C.c_uint64), ("max_views", C.c_uint32), ("reserved0", C.c_uint32), ("reserved", C.c_uint64)]


class PlanSummary(_Record):
    _fields_ = [("coverage", CoverageSummary), ("n_views", C.c_uint32), ("n_selected", C.c_uint32)] + [
        (k, C.c_uint64) for k in ("n_targets", "n_reachable", "n_planned", "target_q40", "reachable_q40", "planned_q40")]
    DICT_FIELDS = [k for k, _ in _fields_[1:]]

    def as_dict(self):
        """The fields (coverage as CoverageSummary.as_dict gives it)."""
        d = super().as_dict()
        d["coverage"] = self.coverage.as_dict()
        return d


assert C.sizeof(PlanOpts) == 208 and C.sizeof(PlanSummary) == 152


def plan_opts(K, width, height, cover=None, view=None, occluder_near=None, min_cos=0.0, tolerance=0.004, slope=0.0, min_gain_q40=0, max_views=8,
              two_sided=False, model_occludes=False, **kw):
    """An hfpf_plan_opts: the sensor (K = (fx, fy, cx, cy), width, height and the other keywords of render_opts(), or a ready `view`),
    what a target is (the keywords of cover_opts(), or a ready `cover`; the view's own min_count is view_min_count), the nearest distance at which a surface still blocks a ray
    (default: the view's z_near), the facing gate (min_cos < 0 = off), the depth test (tolerance + slope * zc, metres) and the
    greedy selection (max_views, min_gain_q40)."""
    ck = {k: kw.pop(k) for k in ("radius", "min_count", "max_distance", "spacing", "max_subdivision", "min_normal_dot", "abs_normal") if k in kw}
    if "view_min_count" in kw:  # min_count is the cover's, as in cover_opts()
        kw["min_count"] = kw.pop("view_min_count")
    o = _sized(PlanOpts)
    o.flags = (PLAN_TWO_SIDED if two_sided else 0) | (PLAN_MODEL_OCCLUDES if model_occludes else 0)
    o.cover = _or(cover, cover_opts, **ck)
    o.view = _or(view, render_opts, K, width, height, **kw)
    o.occluder_near = float(o.view.z_near if occluder_near is None else occluder_near)
    o.min_cos, o.tolerance, o.slope = float(min_cos), float(tolerance), float(slope)
    o.min_gain_q40, o.max_views = int(min_gain_q40), int(max_views)
    return o


check_plan_opts = _opts_checker("plan")


# hfpf_consistency_opts.flags, hfpf_row_consistency.flags and hfpf_row_consistency (include/hfpf.h)
CONSISTENCY_DROP = 1
CONS_SEEN, CONS_SUPPORTED, CONS_CONTRADICTED = 1, 2, 4
CONS_NONE = 0xFFFFFFFF  # first_through of a row no frame sees through
ROW_CONSISTENCY_DTYPE = np.dtype([(k, "<u4") for k in ("n_in_view", "n_tested", "n_support", "n_through", "n_occluded", "first_through",
                                                       "flags", "reserved")])
assert ROW_CONSISTENCY_DTYPE.itemsize == 32


class ConsistencyOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("window", C.c_int32), ("min_through", C.c_uint32),
                ("min_count", C.c_double), ("z_near", C.c_double), ("z_far", C.c_double), ("tolerance", C.c_double), ("slope", C.c_double),
                ("min_cos", C.c_double), ("through_ratio", C.c_double), ("reserved", C.c_uint64)]


class ConsistencySummary(_Record):
    _fields_ = [(k, C.c_uint64) for k in ("n_rows", "n_seen", "n_supported", "n_contradicted", "n_kept", "pairs_tested", "pairs_support",
                                          "pairs_through")]


assert C.sizeof(ConsistencyOpts) == 80 and C.sizeof(ConsistencySummary) == 64


def consistency_opts(window=0, min_through=1, min_count=0.0, z_range=(0.01, 100.0), tolerance=0.004, slope=0.0, min_cos=0.3,
                     through_ratio=1.0, drop=False):
    """An hfpf_consistency_opts: the pixel window's half-width, the THROUGH frames a contradiction needs and their ratio to the SUPPORT
    frames, the count gate, the depth range, tol = tolerance + slope * zc (metres), and the facing gate (below 0 = off)."""
    o = _sized(ConsistencyOpts)
    o.flags = CONSISTENCY_DROP if drop else 0
    o.window, o.min_through = int(window), int(min_through)
    o.min_count, o.z_near, o.z_far = float(min_count), float(z_range[0]), float(z_range[1])
    o.tolerance, o.slope, o.min_cos, o.through_ratio = float(tolerance), float(slope), float(min_cos), float(through_ratio)
    return o


check_consistency_opts = _opts_checker("consistency")


# hfpf_hide_opts.op, hfpf_hide_opts and hfpf_hide_result (include/hfpf.h)
HIDE, SHOW, HIDE_OTHERS = 1, 2, 3
HIDE_OPS = {"hide": HIDE, "show": SHOW, "hide_others": HIDE_OTHERS}


class HideOpts(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("struct_size", "op", "select_mask", "select_value", "flags", "reserved")]


class HideResult(_Record):
    DICT_FIELDS = ("n_selected", "n_matched", "n_changed", "n_hidden", "n_full")
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(k, C.c_uint64) for k in DICT_FIELDS]


assert C.sizeof(HideOpts) == 24 and C.sizeof(HideResult) == 48


def hide_opts(op="hide", select_mask=0, select_value=0):
    """An hfpf_hide_opts: the op ("hide", "show", "hide_others" or its number) and the selector's mask and value."""
    o = _sized(HideOpts)
    o.op = HIDE_OPS.get(op, op)
    o.select_mask, o.select_value = int(select_mask) & 0xFFFFFFFF, int(select_value) & 0xFFFFFFFF
    return o


check_hide_opts = _opts_checker("hide")


def _copy_out(outs, free, *free_args):
    """numpy copies of engine-owned host arrays, which free(*free_args) then releases (always, also when a copy cannot be
    allocated).  outs: (pointer, count or shape, dtype, wanted) each; an unwanted array comes back as None."""
    try:
        copies = tuple(np.empty(shape, dtype) if wanted else None for _, shape, dtype, wanted in outs)
        for a, (ptr, _, _, _) in zip(copies, outs):
            if a is not None and a.nbytes:
                C.memmove(a.ctypes.data, ptr.value, a.nbytes)
        return copies
    finally:
        free(*free_args)


def _mesh_out(v, nv, t, nt):
    """(vertices, triangles) copied out of the two host arrays of an hfpf_extract_mesh or hfpf_read_ply, which are freed."""
    return _copy_out([(v, nv.value, MESH_VERTEX_DTYPE, True), (t, (nt.value, 3), np.uint32, True)], lib().hfpf_free_mesh, v, t)


def read_ply(path):
    """hfpf_read_ply: (vertices of MESH_VERTEX_DTYPE, (n, 3) uint32 triangles) of a binary little-endian PLY (host code, no GPU
    needed); HfpfError with the reader's message otherwise."""
    v, nv, t, nt = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    rc = lib().hfpf_read_ply(os.fsencode(str(path)), C.byref(v), C.byref(nv), C.byref(t), C.byref(nt))
    if rc != 0:
        raise HfpfError(rc, (lib().hfpf_last_error(None) or b"").decode())
    return _mesh_out(v, nv, t, nt)


# hfpf_raycast_opts.flags, hfpf_ray_hit.flags, hfpf_ray and hfpf_ray_hit (include/hfpf.h)
RAYCAST_CULL_BACKFACES = 1
RAY_USED, RAY_HIT, RAY_BACKFACE, RAY_NEAR = 1, 2, 4, 8
RAY_DTYPE = np.dtype([("o", "<f4", (3,)), ("d", "<f4", (3,))])
RAY_HIT_DTYPE = np.dtype([("t", "<f4"), ("flags", "<u4"), ("p", "<f4", (3,)), ("n", "<f4", (3,)), ("row_voxel", "<i4", (3,)),
                          ("rgb", "<u4"), ("count", "<u4"), ("sample", "<u4"), ("reserved", "<u4", (2,))])
assert RAY_DTYPE.itemsize == 24 and RAY_HIT_DTYPE.itemsize == 64


class RaycastOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("radius", C.c_int32), ("reserved0", C.c_int32),
                ("min_count", C.c_double), ("max_distance", C.c_double), ("step", C.c_double), ("t_min", C.c_double),
                ("t_max", C.c_double), ("reserved", C.c_uint64)]


def raycast_opts(radius=2, min_count=0.0, max_distance=float("inf"), step=0.5, t_range=(0.0, 1.0), cull_backfaces=False):
    """An hfpf_raycast_opts: the query window of the samples (1..4), the count and distance gates, the sample spacing in voxels and
    the ray interval (metres along a general ray, z_near / z_far of a view)."""
    o = _sized(RaycastOpts)
    o.flags = RAYCAST_CULL_BACKFACES if cull_backfaces else 0
    o.radius = int(radius)
    o.min_count, o.max_distance, o.step = float(min_count), float(max_distance), float(step)
    o.t_min, o.t_max = float(t_range[0]), float(t_range[1])
    return o


check_raycast_opts = _opts_checker("raycast")


def _rays(rays):
    """(n, 6) float32 (origin, direction) or RAY_DTYPE records -> contiguous RAY_DTYPE."""
    rays = np.asarray(rays)
    if rays.dtype != RAY_DTYPE:
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6).view(RAY_DTYPE).reshape(-1)
    return np.ascontiguousarray(rays)


def write_ply(verts, tris, path):
    """hfpf_write_ply of MESH_VERTEX_DTYPE vertices and (n, 3) uint32 triangles (host code, no GPU needed)."""
    verts = np.ascontiguousarray(verts, MESH_VERTEX_DTYPE)
    tris = np.ascontiguousarray(tris, np.uint32).reshape(-1, 3)
    rc = lib().hfpf_write_ply(_p(verts) if len(verts) else None, len(verts), _p(tris) if len(tris) else None, len(tris), str(path).encode())
    if rc != 0:
        raise HfpfError(rc, "hfpf_write_ply(%s) failed" % path)


SNAPSHOT_HEADER_BYTES = 4096  # HFPF_SNAPSHOT_HEADER_BYTES: what snapshot_info needs of a blob or file


class SnapshotInfo(C.Structure):
    """struct hfpf_snapshot_info (include/hfpf.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("format_version", C.c_uint32), ("layout_tag", C.c_uint64), ("total_bytes", C.c_uint64),
                ("payload_bytes", C.c_uint64), ("payload_checksum", C.c_uint64), ("resolution", C.c_float), ("flags", C.c_uint32),
                ("bbox", C.c_double * 6), ("k", C.c_int32), ("K", C.c_int32), ("gate", C.c_int32), ("reserved0", C.c_int32),
                ("cylinder_radius", C.c_double), ("ball_radius", C.c_double), ("z_clip_min", C.c_double), ("z_clip_max", C.c_double),
                ("max_bricks", C.c_uint64), ("max_log_points", C.c_uint64), ("max_normals", C.c_uint64), ("max_frames", C.c_uint64),
                ("frames_integrated", C.c_uint64), ("clean_passes", C.c_uint64), ("next_frame_id", C.c_uint64),
                ("voxels_occupied", C.c_uint64), ("voxels_with_normal", C.c_uint64), ("reserved", C.c_uint64 * 4)]


def _snapshot_info_struct(info):
    """A SnapshotInfo from the dict snapshot_info() returns (or a SnapshotInfo as it is)."""
    if isinstance(info, SnapshotInfo):
        return info
    s = _sized(SnapshotInfo)
    for name, ctype in SnapshotInfo._fields_:
        if name in ("struct_size", "reserved", "reserved0") or name not in info:
            continue
        if name == "bbox":
            for i in range(6):
                s.bbox[i] = float(info["bbox"][i])
        else:
            setattr(s, name, info[name])
    return s


def snapshot_info(blob):
    """hfpf_snapshot_info: what the header of a snapshot says, as a dict (host code: no handle, no GPU).  blob: bytes-like, at
    least its first SNAPSHOT_HEADER_BYTES bytes."""
    raw = np.frombuffer(blob, dtype=np.uint8) if blob is not None else None
    s = _sized(SnapshotInfo)
    rc =lib().hfpf_snapshot_info(_p(raw) if raw is not None and raw.size else None, raw.size if raw is not None else 0, C.byref(s))
    if rc != 0:
        raise HfpfError(rc, "not a snapshot of this format (hfpf_snapshot_info)")
    out = {n: getattr(s, n) for n, _ in SnapshotInfo._fields_ if n not in ("struct_size", "reserved", "reserved0")}
    out["bbox"] = tuple(s.bbox[:])
    return out


def config_from_snapshot(info):
    """hfpf_config_from_snapshot: the Config a handle needs to take the snapshot `info` describes (capacities = the needed ones,
    device and scheduling hints at their defaults).  OccupancyGrid.from_config(cfg) creates it."""
    c = Config()
    s = _snapshot_info_struct(info)
    rc = lib().hfpf_config_from_snapshot(C.byref(s), C.byref(c))
    if rc != 0:
        raise HfpfError(rc, "hfpf_config_from_snapshot")
    return c


class _SnapshotBuffer:
    """Owner of one hfpf_snapshot result (engine-allocated host memory); exposes it to numpy without copying."""

    def __init__(self, ptr, n):
        self._ptr, self._n = ptr, n

    @property
    def __array_interface__(self):
        return {"shape": (self._n,), "typestr": "|u1", "data": (self._ptr, False), "version": 3}

    def __del__(self):
        try:
            lib().hfpf_free_snapshot(C.c_void_p(self._ptr))
        except Exception:
            pass


EPOCH_REC_DTYPE = np.dtype([("key", "<u8"), ("first_frame", "<u4"), ("vx", "<f4"), ("vy", "<f4"), ("vz", "<f4"), ("pad", "<u4", (2,))])
assert EPOCH_REC_DTYPE.itemsize == 32


def build(force=False):
    """hipcc cross-compiles gfx950 without a GPU; see csrc/Makefile."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-C", CSRC_DIR, "-s"])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HfpfError(-4, "libhfpf.so not built (%s); run __graft_entry__.build() -- there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32
    for name in ("hfpf_default_config", "hfpf_free_rows", "hfpf_free_mesh", "hfpf_free_components", "hfpf_free_deviation", "hfpf_free_coverage",
                 "hfpf_free_plan", "hfpf_free_section", "hfpf_free_topology", "hfpf_free_consistency", "hfpf_free_snapshot"):  # the void functions
        getattr(L, name).restype = None
    L.hfpf_default_config.argtypes = [C.POINTER(Config)]
    L.hfpf_abi_version.restype = C.c_int
    L.hfpf_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.hfpf_destroy.argtypes = [vp]
    L.hfpf_last_error.argtypes = [vp]
    L.hfpf_last_error.restype = C.c_char_p
    L.hfpf_get_dims.argtypes = [vp, C.POINTER(i32), C.POINTER(C.c_double)]
    L.hfpf_integrate.argtypes = [vp, vp, u32, u32, u32, u32, u32, u32, vp]
    L.hfpf_integrate_device.argtypes = [vp, vp, u32, u64, u32, u32, u32, u32, u32, u32, vp, vp]
    L.hfpf_integrate_pinned.argtypes = [vp, vp, u32, u32, u32, u32, u32, u32, vp]
    L.hfpf_host_alloc.argtypes = [vp, u64, C.POINTER(vp)]
    L.hfpf_host_free.argtypes = [vp, vp]
    L.hfpf_is_dirty.argtypes = [vp]
    L.hfpf_clean.argtypes = [vp]
    L.hfpf_extract.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    L.hfpf_extract_filtered.argtypes = [vp, C.POINTER(ExtractOpts), C.POINTER(vp), C.POINTER(u64)]
    L.hfpf_free_rows.argtypes = [vp]
    L.hfpf_write_pcd.argtypes = [vp, u64, C.c_char_p]
    L.hfpf_write_meta_csv.argtypes = [vp, u64, C.c_char_p]
    L.hfpf_write_pcd_xyzrgb.argtypes = [vp, u64, C.c_char_p, u32, i32, i32]
    L.hfpf_write_pcd_binary.argtypes = [vp, u64, C.c_char_p]
    L.hfpf_clear.argtypes = [vp]
    L.hfpf_sync.argtypes = [vp]
    L.hfpf_get_counters.argtypes = [vp, C.POINTER(Counters)]
    L.hfpf_get_occupied.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.hfpf_device_alloc.argtypes = [vp, u64, C.POINTER(vp)]
    L.hfpf_device_free.argtypes = [vp, vp]
    L.hfpf_device_upload.argtypes = [vp, vp, vp, u64]
    L.hfpf_kernel_timing.argtypes = [vp, C.c_int]
    L.hfpf_get_kernel_time.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(u64)]
    L.hfpf_probe_points.argtypes = [vp, vp, vp, u64, vp, vp, vp]
    L.hfpf_probe_normals.argtypes = [vp, u64, vp, vp, vp, vp, vp]
    L.hfpf_probe_project.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp]
    L.hfpf_probe_trig.argtypes = [vp, u64, vp, vp, vp, vp, vp]
    L.hfpf_dist_unique_id.argtypes = [vp]
    L.hfpf_dist_init.argtypes = [vp, C.c_int, C.c_int, vp]
    L.hfpf_dist_disable.argtypes = [vp]
    L.hfpf_dist_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.hfpf_epoch_export.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    L.hfpf_epoch_import.argtypes = [vp, vp, u64]
    L.hfpf_stats_export.argtypes = [vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(u64)]
    L.hfpf_extract_with_stats.argtypes = [vp, vp, vp, C.POINTER(vp), C.POINTER(u64)]
    L.hfpf_device_download.argtypes = [vp, vp, vp, u64]
    L.hfpf_device_copy.argtypes = [vp, vp, vp, u64]
    L.hfpf_epoch_import_gathered.argtypes = [vp, vp, u64, i32, i32, vp]
    L.hfpf_integrate_depth.argtypes = [vp, C.POINTER(DepthImage), vp, vp, vp]
    L.hfpf_integrate_depth_pinned.argtypes = [vp, C.POINTER(DepthImage), vp, vp, vp]
    L.hfpf_integrate_depth_device.argtypes = [vp, C.POINTER(DepthImage), vp, u64, vp, u64, u32, vp, vp]
    L.hfpf_probe_depth.argtypes = [vp, C.POINTER(DepthImage), vp, vp, vp, vp]
    L.hfpf_render.argtypes = [vp, C.POINTER(RenderOpts), vp, C.POINTER(RenderPlanes)]
    L.hfpf_render_device.argtypes = [vp, C.POINTER(RenderOpts), u32, vp, C.POINTER(RenderPlanes)]
    L.hfpf_track_depth.argtypes = [vp, C.POINTER(TrackOpts), C.POINTER(DepthImage), vp, vp, C.POINTER(TrackResult)]
    L.hfpf_track_depth_device.argtypes = [vp, C.POINTER(TrackOpts), C.POINTER(DepthImage), vp, vp, C.POINTER(TrackResult)]
    L.hfpf_track.argtypes = [vp, C.POINTER(TrackOpts), vp, u32, u32, u32, u32, u32, vp, C.POINTER(TrackResult)]
    L.hfpf_query.argtypes = [vp, C.POINTER(QueryOpts), vp, u32, u32, u32, u32, u32, vp, vp, vp]
    L.hfpf_query_device.argtypes = [vp, C.POINTER(QueryOpts), vp, u32, u32, u32, u32, u32, vp, vp, vp]
    L.hfpf_query_depth.argtypes = [vp, C.POINTER(QueryOpts), C.POINTER(DepthImage), vp, vp, vp, vp]
    L.hfpf_extract_mesh.argtypes = [vp, C.POINTER(MeshOpts), C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(u64)]
    L.hfpf_extract_mesh_device.argtypes = [vp, C.POINTER(MeshOpts), C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(u64)]
    L.hfpf_free_mesh.argtypes = [vp, vp]
    L.hfpf_write_ply.argtypes = [vp, u64, vp, u64, C.c_char_p]
    L.hfpf_check_mesh_opts.argtypes = [C.POINTER(MeshOpts)]
    L.hfpf_check_component_opts.argtypes = [C.POINTER(ComponentOpts)]
    for fn in (L.hfpf_extract_components, L.hfpf_extract_components_device):
        fn.argtypes = [vp, C.POINTER(ComponentOpts), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(u64)]
    L.hfpf_free_components.argtypes = [vp, vp, vp]
    L.hfpf_check_deviation_opts.argtypes = [C.POINTER(DeviationOpts)]
    for fn in (L.hfpf_compare_mesh, L.hfpf_compare_mesh_device):
        fn.argtypes = [vp, C.POINTER(DeviationOpts), vp, u64, u32, vp, u64, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64),
                       C.POINTER(DeviationSummary)]
    L.hfpf_check_align_opts.argtypes = [C.POINTER(AlignOpts)]
    for fn in (L.hfpf_align_mesh, L.hfpf_align_mesh_device):
        fn.argtypes = [vp, C.POINTER(AlignOpts), vp, u64, u32, vp, u64, vp, C.POINTER(AlignResult)]
    L.hfpf_check_cover_opts.argtypes = [C.POINTER(CoverOpts)]
    for fn in (L.hfpf_cover_mesh, L.hfpf_cover_mesh_device):
        fn.argtypes = [vp, C.POINTER(CoverOpts), vp, u64, u32, vp, u64, vp, C.POINTER(vp), C.POINTER(CoverageSummary)]
    L.hfpf_free_coverage.argtypes = [vp]
    L.hfpf_check_plan_opts.argtypes = [C.POINTER(PlanOpts)]
    for fn in (L.hfpf_plan_views, L.hfpf_plan_views_device):
        fn.argtypes = [vp, C.POINTER(PlanOpts), vp, u64, u32, vp, u64, vp, vp, u32, vp, C.POINTER(vp), C.POINTER(PlanSummary)]
    L.hfpf_free_plan.argtypes = [vp]
    L.hfpf_check_section_opts.argtypes = [C.POINTER(SectionOpts)]
    for fn in (L.hfpf_section_mesh, L.hfpf_section_mesh_device):
        fn.argtypes = [vp, C.POINTER(SectionOpts), vp, u64, u32, vp, u64, vp, vp, u32, C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(u64),
                       C.POINTER(vp), C.POINTER(u64), vp, C.POINTER(SectionSummary)]
    L.hfpf_free_section.argtypes = [vp, vp, vp]
    L.hfpf_check_topology_opts.argtypes = [C.POINTER(TopologyOpts)]
    for fn in (L.hfpf_mesh_topology, L.hfpf_mesh_topology_device):
        fn.argtypes = [vp, C.POINTER(TopologyOpts), vp, u64, u32, vp, u64, vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(u64),
                       C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(TopologySummary)]
    L.hfpf_free_topology.argtypes = [vp, vp, vp, vp]
    L.hfpf_free_deviation.argtypes = [vp, vp]
    L.hfpf_check_consistency_opts.argtypes = [C.POINTER(ConsistencyOpts)]
    for fn in (L.hfpf_depth_consistency, L.hfpf_depth_consistency_device):
        fn.argtypes = [vp, C.POINTER(ConsistencyOpts), C.POINTER(DepthImage), vp, u64, u32, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64),
                       C.POINTER(ConsistencySummary)]
    L.hfpf_free_consistency.argtypes = [vp, vp]
    L.hfpf_check_hide_opts.argtypes = [C.POINTER(HideOpts)]
    for fn in (L.hfpf_hide_voxels, L.hfpf_hide_voxels_device):
        fn.argtypes = [vp, C.POINTER(HideOpts), vp, u64, u32, vp, u32, C.POINTER(HideResult)]
    L.hfpf_hide_box.argtypes = [vp, u32, vp, vp, C.POINTER(HideResult)]
    L.hfpf_show_all.argtypes = [vp]
    L.hfpf_get_hidden.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.hfpf_read_ply.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(u64)]
    dbl = C.c_double
    L.hfpf_check_raycast_opts.argtypes = [C.POINTER(RaycastOpts)]
    L.hfpf_raycast.argtypes = [vp, C.POINTER(RaycastOpts), vp, u64, vp, vp]
    L.hfpf_raycast_device.argtypes = [vp, C.POINTER(RaycastOpts), vp, u64, vp, vp]
    L.hfpf_raycast_view.argtypes = [vp, C.POINTER(RaycastOpts), u32, u32, dbl, dbl, dbl, dbl, vp, vp]
    L.hfpf_raycast_view_device.argtypes = [vp, C.POINTER(RaycastOpts), u32, u32, dbl, dbl, dbl, dbl, u32, vp, vp]
    L.hfpf_snapshot.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    L.hfpf_free_snapshot.argtypes = [vp]
    L.hfpf_restore.argtypes = [vp, vp, u64]
    L.hfpf_save.argtypes = [vp, C.c_char_p]
    L.hfpf_load.argtypes = [vp, C.c_char_p]
    L.hfpf_snapshot_info.argtypes = [vp, u64, C.POINTER(SnapshotInfo)]
    L.hfpf_config_from_snapshot.argtypes = [C.POINTER(SnapshotInfo), C.POINTER(Config)]
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _pose12(pose, identity=False):
    """The twelve contiguous doubles of one 3x4 [R|t]; identity=True: no pose stands for the identity."""
    if pose is None and identity:
        pose = np.eye(4)[:3]
    return np.ascontiguousarray(pose, dtype=np.float64).reshape(12)


def _poses(poses, n=-1, flat=False):
    """The contiguous doubles of a batch of 3x4 poses: (n, 12), or flat as the consistency calls take them."""
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    return poses.reshape(-1) if flat else poses.reshape(n, 12)


def _cloud_args(cloud, layout, n_points, device=False):
    """(cloud, n_points, point_step, off_x, off_y, off_z) of a cloud of records.  No layout = packed (x, y, z) float32 triples.  A
    host cloud is made contiguous (and float32 without a layout), and n_points defaults to the records it holds; with device=True
    the cloud is a device pointer, passed on as it is."""
    if not device:
        cloud = np.ascontiguousarray(cloud) if layout else np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 3)
    layout = layout or dict(point_step=12, off_x=0, off_y=4, off_z=8)
    step = layout["point_step"]
    if n_points is None:
        n_points = cloud.nbytes // step
    return cloud, n_points, step, layout["off_x"], layout["off_y"], layout["off_z"]


def _mesh_args(verts, tris, device, n_verts, vertex_stride, n_tris):
    """The five mesh arguments of the C ABI, (vertices, n_verts, vertex_stride, triangles, n_tris), and the arrays that have to
    outlive the call.  device=True: verts and tris are device pointers and the three numbers are required.  Otherwise verts are
    MESH_VERTEX_DTYPE records (stride 32) or an (n, 3) float32 array (stride 12), tris (n, 3) uint32, the three numbers override
    what the arrays give, and an array of no bytes is passed as NULL."""
    if device:
        return (C.c_void_p(verts), int(n_verts), int(vertex_stride), C.c_void_p(tris), int(n_tris)), ()
    verts = np.ascontiguousarray(verts)
    if verts.dtype != MESH_VERTEX_DTYPE:
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, np.uint32).reshape(-1, 3)
    stride = int(vertex_stride) if vertex_stride is not None else verts.dtype.itemsize * (1 if verts.dtype == MESH_VERTEX_DTYPE else 3)
    nv = int(n_verts) if n_verts is not None else len(verts)
    nt = int(n_tris) if n_tris is not None else len(tris)
    return (_p(verts) if verts.nbytes else None, nv, stride, _p(tris) if tris.nbytes else None, nt), (verts, tris)


def default_config():
    c = Config()
    lib().hfpf_default_config(C.byref(c))
    return c


class _RowBuffer:
    """Owner of one hfpf_extract result (engine-allocated); exposes it to numpy without copying."""

    def __init__(self, ptr, n):
        self._ptr, self._n = ptr, n

    @property
    def __array_interface__(self):
        return {"shape": (self._n,), "typestr": "|V%d" % ROW_DTYPE.itemsize, "descr": ROW_DTYPE.descr, "data": (self._ptr, False), "version": 3}

    def __del__(self):
        try:
            lib().hfpf_free_rows(C.c_void_p(self._ptr))
        except Exception:
            pass


class OccupancyGrid:
    """Device-resident occupancy grid.  Keyword defaults are the reference's constants."""

    def __init__(self, resolution=None, bbox=None, k=None, K=None, gate=None, cylinder_radius=None, ball_radius=None,
                 z_clip=None, device=0, max_bricks=0, max_log_points=0, max_normals=0, max_frames=0, fuse_color=False, pcl_shifted_cov=False, binned_update=None, frame_width=0, max_call_points=0):
        L = lib()
        c = default_config()
        if resolution is not None:
            c.resolution = resolution
        if bbox is not None:
            if len(bbox) != 6:
                raise HfpfError(-1, "bounding_box needs 6 values (xmin,xmax,ymin,ymax,zmin,zmax)")
            for i in range(6):
                c.bbox[i] = float(bbox[i])
        for name, val in (("k", k), ("K", K), ("gate", gate), ("cylinder_radius", cylinder_radius),
                          ("ball_radius", ball_radius)):
            if val is not None:
                setattr(c, name, val)
        if z_clip is not None:
            c.z_clip_min, c.z_clip_max = z_clip
        c.device = device
        if binned_update is None:
            binned_update = os.environ.get("HFPF_BINNED", "1") != "0"  # HFPF_BINNED=0: A/B against the direct form
        c.flags = ((FLAG_FUSE_COLOR if fuse_color else 0) | (FLAG_PCL_SHIFTED_COV if pcl_shifted_cov else 0) |
                   (0 if binned_update else FLAG_DIRECT_UPDATE))
        c.max_bricks, c.max_log_points, c.max_normals, c.max_frames = max_bricks, max_log_points, max_normals, max_frames
        c.frame_width = int(frame_width)  # scheduling hint only (16x16-pixel tiles); results do not depend on it
        c.max_call_points = int(max_call_points)  # 0 = per-call bins grown on demand
        self._create(c)

    def _create(self, c):
        self.cfg = c
        self._transport = None
        self._h = C.c_void_p()
        rc = lib().hfpf_create(C.byref(c), C.byref(self._h))
        if rc != 0:
            msg = lib().hfpf_last_error(None).decode()
            self._h = None
            raise HfpfError(rc, msg)

    @classmethod
    def from_config(cls, cfg):
        """A grid from a ready Config (config_from_snapshot, or default_config with fields changed)."""
        g = cls.__new__(cls)
        g._create(cfg)
        return g

    # -- plumbing --
    def _chk(self, rc):
        if rc < 0:
            raise HfpfError(rc, lib().hfpf_last_error(self._h).decode())
        return rc

    def _device_results(self, n, outs, call):
        """Where a device form leaves its results.  outs: (the caller's device pointer or 0, dtype, wanted) per result;
        call(*pointers) runs the C call.  With the caller's first pointer the results stay in the caller's buffers and None is
        returned; without it they go through scratch device buffers of n records and come back as a tuple of numpy arrays (None
        for an unwanted one)."""
        if outs[0][0]:
            call(*(ptr for ptr, _, _ in outs))
            return None
        bufs = []
        try:
            for _, dtype, wanted in outs:
                bufs.append(self.device_alloc(max(1, n) * dtype.itemsize) if wanted else 0)
            call(*bufs)
            return tuple(self.device_download(b, n * dtype.itemsize).view(dtype) if b else None for b, (_, dtype, _) in zip(bufs, outs))
        finally:
            for b in bufs:
                if b:
                    self.device_free(b)

    def close(self):
        if getattr(self, "_h", None):
            lib().hfpf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def dims(self):
        d = (C.c_int32 * 3)()
        r = C.c_double()
        self._chk(lib().hfpf_get_dims(self._h, d, C.byref(r)))
        return (d[0], d[1], d[2]), r.value

    # -- the reference surface --
    def integrate(self, buf, pose, n_points=None, point_step=16, off_x=0, off_y=4, off_z=8, off_rgb=12):
        """addPoints + capture stage for one host frame (PointCloud2-style records)."""
        buf = np.ascontiguousarray(buf)
        pose = _pose12(pose)
        if n_points is None:
            n_points = buf.nbytes // point_step
        self._chk(lib().hfpf_integrate(self._h, _p(buf), n_points, point_step, off_x, off_y, off_z, off_rgb, _p(pose)))

    def host_alloc(self, nbytes):
        """Page-locked host memory as a uint8 numpy view (free with host_free(view))."""
        p = C.c_void_p()
        self._chk(lib().hfpf_host_alloc(self._h, nbytes, C.byref(p)))
        return np.frombuffer((C.c_uint8 * nbytes).from_address(p.value), dtype=np.uint8)

    def host_free(self, view):
        self._chk(lib().hfpf_host_free(self._h, C.c_void_p(view.ctypes.data)))

    def integrate_pinned(self, buf, pose, n_points=None, point_step=16, off_x=0, off_y=4, off_z=8, off_rgb=12):
        """One frame straight from page-locked memory (a view from host_alloc): asynchronous, no bounce copy."""
        pose = _pose12(pose)
        if n_points is None:
            n_points = buf.nbytes // point_step
        self._chk(lib().hfpf_integrate_pinned(self._h, C.c_void_p(buf.ctypes.data), n_points, point_step, off_x, off_y, off_z, off_rgb, _p(pose)))

    def integrate_device(self, dev_ptr, n_frames, frame_stride, n_points, poses, frame_ids=None, point_step=16, off_x=0,
                         off_y=4, off_z=8, off_rgb=12):
        poses = _poses(poses, n_frames)
        ids = None
        if frame_ids is not None:
            ids = np.ascontiguousarray(frame_ids, dtype=np.uint32)
        self._chk(lib().hfpf_integrate_device(self._h, C.c_void_p(dev_ptr), n_frames, frame_stride, n_points, point_step,
                                              off_x, off_y, off_z, off_rgb, _p(poses), _p(ids) if ids is not None else None))

    def integrate_depth(self, depth, pose, K, color=None, color_format=None, depth_scale=0.001):
        """One registered depth (+ colour) frame from numpy images in pageable memory (hfpf_integrate_depth).
        K = (fx, fy, cx, cy); depth uint16 (counts of depth_scale metres) or float32 (metres)."""
        d = _image_desc(depth, K, color, color_format, depth_scale)
        pose = _pose12(pose)
        self._chk(lib().hfpf_integrate_depth(self._h, C.byref(d), C.c_void_p(depth.ctypes.data),
                                             C.c_void_p(color.ctypes.data) if color is not None else None, _p(pose)))

    def integrate_depth_pinned(self, depth, pose, K, color=None, color_format=None, depth_scale=0.001):
        """The same for images that are views of page-locked memory (host_alloc); they must stay untouched until the next sync."""
        d = _image_desc(depth, K, color, color_format, depth_scale)
        pose = _pose12(pose)
        self._chk(lib().hfpf_integrate_depth_pinned(self._h, C.byref(d), C.c_void_p(depth.ctypes.data),
                                                    C.c_void_p(color.ctypes.data) if color is not None else None, _p(pose)))

    def integrate_depth_device(self, desc, dev_depth, depth_frame_stride, n_frames, poses, dev_color=0, color_frame_stride=0,
                               frame_ids=None):
        """n_frames depth frames resident in HBM (hfpf_integrate_depth_device); desc from depth_desc()."""
        poses = _poses(poses, n_frames)
        ids = np.ascontiguousarray(frame_ids, dtype=np.uint32) if frame_ids is not None else None
        self._chk(lib().hfpf_integrate_depth_device(self._h, C.byref(desc), C.c_void_p(dev_depth), depth_frame_stride,
                                                    C.c_void_p(dev_color) if dev_color else None, color_frame_stride, n_frames,
                                                    _p(poses), _p(ids) if ids is not None else None))

    @property
    def state_changed(self):
        return bool(self._chk(lib().hfpf_is_dirty(self._h)))

    def clean(self):
        """updateThicknessVectors.  With a host-staged transport attached (see hfpf_dist.py) the epoch exchange
        runs first; with RCCL (dist_init_rccl) the engine does it internally.  Collective across ranks."""
        if self._transport is not None:
            self._transport.exchange(self)
        self._chk(lib().hfpf_clean(self._h))

    def _rows_out(self, rows, n):
        """Zero-copy: a numpy view over the engine-owned row buffer; hfpf_free_rows runs when the view is collected."""
        if not n.value:
            return np.zeros(0, dtype=ROW_DTYPE)
        return np.asarray(_RowBuffer(rows.value, n.value))

    def extract(self):
        if self._transport is not None:
            return self._transport.merged_extract(self)
        rows = C.c_void_p()
        n = C.c_uint64()
        self._chk(lib().hfpf_extract(self._h, C.byref(rows), C.byref(n)))
        return self._rows_out(rows, n)

    def extract_filtered(self, min_count=0.0, classify_threshold=-1, paint_white=False):
        """downloadHQ(threshold) / downloadClassified / download of the reference (grid.hpp:491-601): the same ordered
        extract with the count filter and the colour coding done on the device."""
        o = ExtractOpts(C.sizeof(ExtractOpts), int(classify_threshold), float(min_count), 1 if paint_white else 0, 0)
        rows = C.c_void_p()
        n = C.c_uint64()
        self._chk(lib().hfpf_extract_filtered(self._h, C.byref(o), C.byref(rows), C.byref(n)))
        return self._rows_out(rows, n)

    # -- looking at the model from a camera --
    def render(self, pose, K, width, height, planes=("depth", "normal", "rgb", "count", "voxel"), opts=None, **kw):
        """One view of the fused model (hfpf_render): pose = camera -> fusion frame 3x4, K = (fx, fy, cx, cy).  Keywords as
        render_opts (z_range, min_count, splat_radius, max_splat_radius, cull_backfaces, world_normals), or a ready `opts`.
        Returns {plane: HxW (depth, rgb, count) or HxWx3 (normal, voxel) array} for the requested planes."""
        o = _or(opts, render_opts, K, width, height, **kw)
        pose = _pose12(pose)
        out, pl = {}, RenderPlanes()
        for name, dt, ch in RENDER_PLANES:
            if name in planes:
                out[name] = np.empty((o.height, o.width, ch) if ch > 1 else (o.height, o.width), dtype=dt)
                setattr(pl, name, out[name].ctypes.data)
        unknown = set(planes) - set(out)
        if unknown:
            raise ValueError("unknown render planes %s" % sorted(unknown))
        self._chk(lib().hfpf_render(self._h, C.byref(o), _p(pose), C.byref(pl)))
        return out

    def render_device(self, poses, K, width, height, dev_planes, opts=None, **kw):
        """len(poses) views into device planes (hfpf_render_device): dev_planes = {plane: device pointer}; view v of a plane
        starts v * width * height elements (x 3 for normal and voxel) behind its pointer."""
        o = _or(opts, render_opts, K, width, height, **kw)
        poses = _poses(poses)
        pl = RenderPlanes()
        for name, ptr in dev_planes.items():
            if name not in RenderPlanes.__dict__:
                raise ValueError("unknown render plane %r" % name)
            setattr(pl, name, ptr)
        self._chk(lib().hfpf_render_device(self._h, C.byref(o), poses.shape[0], _p(poses), C.byref(pl)))

    # -- correcting a frame's pose against the model --
    def track_depth(self, depth, pose, K, depth_scale=0.001, opts=None, **kw):
        """Refine the camera -> fusion pose of one depth image in pageable memory (hfpf_track_depth).  The model view defaults to the
        image's own intrinsics and size with back faces culled; keywords as track_opts.  Returns (3x4 pose, result dict)."""
        d = _image_desc(depth, K, None, None, depth_scale)
        o = _or(opts, track_opts, K, depth.shape[1], depth.shape[0], **kw)
        pose = _pose12(pose)
        r = track_result()
        self._chk(lib().hfpf_track_depth(self._h, C.byref(o), C.byref(d), C.c_void_p(depth.ctypes.data), _p(pose), C.byref(r)))
        return _track_out(r)

    def track_depth_device(self, desc, dev_depth, pose, opts=None, **kw):
        """The same for a depth image resident in HBM (hfpf_track_depth_device); desc from depth_desc()."""
        o = _or(opts, track_opts, (desc.fx, desc.fy, desc.cx, desc.cy), desc.width, desc.height, **kw)
        pose = _pose12(pose)
        r = track_result()
        self._chk(lib().hfpf_track_depth_device(self._h, C.byref(o), C.byref(desc), C.c_void_p(dev_depth), _p(pose), C.byref(r)))
        return _track_out(r)

    def track(self, cloud, layout, pose, view_K, width, height, n_points=None, opts=None, **kw):
        """Refine the pose of one cloud of records in pageable memory (hfpf_track); layout = dict(point_step, off_x, off_y, off_z)
        (extra keys such as off_rgb are ignored); the model view is (view_K, width, height)."""
        cloud, *layout = _cloud_args(cloud, layout, n_points)
        o = _or(opts, track_opts, view_K, width, height, **kw)
        pose = _pose12(pose)
        r = track_result()
        self._chk(lib().hfpf_track(self._h, C.byref(o), _p(cloud), *layout, _p(pose), C.byref(r)))
        return _track_out(r)

    # -- querying the model at given points --
    def query(self, cloud, pose, layout=None, n_points=None, opts=None, radius=1, min_count=0.0, max_distance=float("inf"), zclip=False,
              rows=True):
        """Nearest row within the voxel window of each point of a cloud in pageable memory (hfpf_query).  cloud: an (N, 3) float32
        array, or records with layout = dict(point_step, off_x, off_y, off_z) (extra keys are ignored).  Returns (hits, rows):
        numpy arrays of QUERY_HIT_DTYPE and ROW_DTYPE; rows is None with rows=False."""
        cloud, n_points, *layout = _cloud_args(cloud, layout, n_points)
        o = _or(opts, query_opts, radius, min_count, max_distance, zclip)
        pose = _pose12(pose)
        hits = np.empty(n_points, QUERY_HIT_DTYPE)
        out = np.empty(n_points, ROW_DTYPE) if rows else None
        self._chk(lib().hfpf_query(self._h, C.byref(o), _p(cloud), n_points, *layout, _p(pose), _p(hits), _p(out) if rows else None))
        return hits, out

    def query_device(self, dev_cloud, n_points, pose, layout=None, dev_hits=0, dev_rows=0, rows=True, opts=None, radius=1, min_count=0.0,
                     max_distance=float("inf"), zclip=False):
        """The same for a cloud resident in HBM, read in place (hfpf_query_device); layout defaults to packed (x, y, z) f32 triples.
        With dev_hits (and dev_rows, or 0 for none) the results stay in those device buffers and None is returned; otherwise they go
        to scratch device buffers and come back as (hits, rows) numpy arrays as query() returns them."""
        dev_cloud, n_points, *layout = _cloud_args(dev_cloud, layout, n_points, device=True)
        o = _or(opts, query_opts, radius, min_count, max_distance, zclip)
        pose = _pose12(pose)

        def call(hits, out):
            self._chk(lib().hfpf_query_device(self._h, C.byref(o), C.c_void_p(dev_cloud), n_points, *layout, _p(pose), C.c_void_p(hits),
                                              C.c_void_p(out) if out else None))
        return self._device_results(n_points, [(dev_hits, QUERY_HIT_DTYPE, True), (dev_rows, ROW_DTYPE, rows)], call)

    # -- a surface of the model --
    def extract_mesh(self, opts=None, radius=2, min_count=0.0, max_distance=float("inf")):
        """The triangle mesh of the fused model (hfpf_extract_mesh): (vertices of MESH_VERTEX_DTYPE, (n, 3) uint32 triangles), copied
        out of the engine's host arrays."""
        o = _or(opts, mesh_opts, radius, min_count, max_distance)
        v, nv, t, nt = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        self._chk(lib().hfpf_extract_mesh(self._h, C.byref(o), C.byref(v), C.byref(nv), C.byref(t), C.byref(nt)))
        return _mesh_out(v, nv, t, nt)

    def extract_mesh_device(self, opts=None, radius=2, min_count=0.0, max_distance=float("inf")):
        """The same mesh in HBM (hfpf_extract_mesh_device): (vertex pointer, n_verts, triangle pointer, n_tris); free both pointers with
        device_free (they are 0 for an empty mesh)."""
        o = _or(opts, mesh_opts, radius, min_count, max_distance)
        v, nv, t, nt = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        self._chk(lib().hfpf_extract_mesh_device(self._h, C.byref(o), C.byref(v), C.byref(nv), C.byref(t), C.byref(nt)))
        return v.value or 0, nv.value, t.value or 0, nt.value

    # -- connected components, and the model without its specks --
    def extract_components(self, opts=None, rows=True, device=False, **kw):
        """The rows of the kept components, their labels and the component records (hfpf_extract_components): (rows of ROW_DTYPE or
        None with rows=False, uint32 labels, comps of COMPONENT_DTYPE), copied out of the engine's host arrays.  Keywords as
        component_opts().  device=True runs hfpf_extract_components_device instead and returns (rows pointer, labels pointer, n_rows,
        comps pointer, n_comps) in HBM; free the pointers with device_free (they are 0 when nothing is kept)."""
        o = _or(opts, component_opts, **kw)
        r, l, nr, c, nc = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        fn = lib().hfpf_extract_components_device if device else lib().hfpf_extract_components
        self._chk(fn(self._h, C.byref(o), C.byref(r) if rows else None, C.byref(l), C.byref(nr), C.byref(c), C.byref(nc)))
        if device:
            return r.value or 0, l.value or 0, nr.value, c.value or 0, nc.value
        return _copy_out([(r, nr.value, ROW_DTYPE, rows), (l, nr.value, np.uint32, True), (c, nc.value, COMPONENT_DTYPE, True)],
                         lib().hfpf_free_components, r, l, c)

    # -- deviation from a triangle mesh --
    def compare_mesh(self, verts, tris, pose=None, device=False, opts=None, rows=False, n_verts=None, vertex_stride=None, n_tris=None, **kw):
        """How far the model's rows are from a triangle mesh (hfpf_compare_mesh): (dev of DEVIATION_DTYPE, summary dict), or (rows of
        ROW_DTYPE, dev, summary) with rows=True.  verts: MESH_VERTEX_DTYPE vertices (stride 32) or an (n, 3) float32 array (stride 12;
        vertex_stride overrides); tris: (n, 3) uint32; pose: 3x4 [R|t] mesh frame -> fusion frame (identity by default).  Keywords as
        deviation_opts().  device=True runs hfpf_compare_mesh_device: verts and tris are device pointers (n_verts, vertex_stride and
        n_tris are then required) and the result is (rows pointer or 0, dev pointer, n_rows, summary); free the pointers with
        device_free (they are 0 without rows)."""
        o = _or(opts, deviation_opts, **kw)
        pose = _pose12(pose, identity=True)
        mesh, keep = _mesh_args(verts, tris, device, n_verts, vertex_stride, n_tris)
        r, d, nr, s = C.c_void_p(), C.c_void_p(), C.c_uint64(), DeviationSummary()
        fn = lib().hfpf_compare_mesh_device if device else lib().hfpf_compare_mesh
        self._chk(fn(self._h, C.byref(o), *mesh, _p(pose), C.byref(r) if rows else None, C.byref(d), C.byref(nr), C.byref(s)))
        if device:
            return r.value or 0, d.value or 0, nr.value, s.as_dict()
        out_rows, dev = _copy_out([(r, nr.value, ROW_DTYPE, rows), (d, nr.value, DEVIATION_DTYPE, True)], lib().hfpf_free_deviation, r, d)
        return (out_rows, dev, s.as_dict()) if rows else (dev, s.as_dict())

    # -- best-fitting a triangle mesh to the model --
    def align_mesh(self, verts, tris, pose=None, device=False, opts=None, n_verts=None, vertex_stride=None, n_tris=None, **kw):
        """Refine the mesh frame -> fusion frame pose of a triangle mesh against the model's rows (hfpf_align_mesh): a dict of
        iterations, flags, rows_sampled, inliers, rms, information (6x6) and pose (3x4, to hand to compare_mesh).  verts, tris, pose
        and the device form's arguments as compare_mesh(); keywords as align_opts().  The capture range is max_distance."""
        o = _or(opts, align_opts, **kw)
        pose = _pose12(pose, identity=True)
        mesh, keep = _mesh_args(verts, tris, device, n_verts, vertex_stride, n_tris)
        r = align_result()
        fn = lib().hfpf_align_mesh_device if device else lib().hfpf_align_mesh
        self._chk(fn(self._h, C.byref(o), *mesh, _p(pose), C.byref(r)))
        return _refine_out(r, "rows_sampled")

    # -- coverage of a triangle mesh by the model --
    def cover_mesh(self, verts, tris, pose=None, device=False, opts=None, n_verts=None, vertex_stride=None, n_tris=None, **kw):
        """Which parts of a triangle mesh the model has rows near (hfpf_cover_mesh): (records of TRI_COVERAGE_DTYPE, one per triangle;
        summary dict with the derived floats area and covered_area in m^2).  verts, tris, pose and the device form's arguments as
        compare_mesh(); keywords as cover_opts().  device=True runs hfpf_cover_mesh_device and returns (records pointer, summary);
        free the pointer with device_free (it is 0 without triangles)."""
        o = _or(opts, cover_opts, **kw)
        pose = _pose12(pose, identity=True)
        mesh, keep = _mesh_args(verts, tris, device, n_verts, vertex_stride, n_tris)
        c, s = C.c_void_p(), CoverageSummary()
        fn = lib().hfpf_cover_mesh_device if device else lib().hfpf_cover_mesh
        self._chk(fn(self._h, C.byref(o), *mesh, _p(pose), C.byref(c), C.byref(s)))
        if device:
            return c.value or 0, s.as_dict()
        cov, = _copy_out([(c, mesh[4] if c.value else 0, TRI_COVERAGE_DTYPE, True)], lib().hfpf_free_coverage, c)  # mesh[4]: n_tris
        return cov, s.as_dict()

    # -- planar sections of a triangle mesh --
    def section_mesh(self, verts, tris, pose=None, planes=(), device=False, opts=None, n_verts=None, vertex_stride=None, n_tris=None):
        """Cut a triangle mesh with planes (hfpf_section_mesh): (points of SECTION_POINT_DTYPE, segments of SECTION_SEGMENT_DTYPE,
        contours of SECTION_CONTOUR_DTYPE, one record of SECTION_PLANE_DTYPE per plane, summary dict).  planes: (n, 4) float64 rows
        (n.x, n.y, n.z, d) in the fusion frame; verts, tris, pose and the device form's arguments as compare_mesh().  device=True runs
        hfpf_section_mesh_device and returns the three arrays as (pointer, count) pairs in HBM: free the pointers with device_free
        (they are 0 without segments).  section_mesh_device() is that form by name."""
        o = _or(opts, section_opts)
        pose = _pose12(pose, identity=True)
        planes = np.ascontiguousarray(planes, np.float64).reshape(-1, 4)
        recs = np.zeros(len(planes), SECTION_PLANE_DTYPE)
        pp, rp = (_p(planes), _p(recs)) if len(planes) else (None, None)
        mesh, keep = _mesh_args(verts, tris, device, n_verts, vertex_stride, n_tris)
        p, s, c, npt, ns, nc, summ = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64(), SectionSummary()
        fn = lib().hfpf_section_mesh_device if device else lib().hfpf_section_mesh
        self._chk(fn(self._h, C.byref(o), *mesh, _p(pose), pp, len(planes), C.byref(p), C.byref(npt), C.byref(s), C.byref(ns), C.byref(c),
                     C.byref(nc), rp, C.byref(summ)))
        if device:
            return (p.value or 0, npt.value), (s.value or 0, ns.value), (c.value or 0, nc.value), recs, summ.as_dict()
        points, segments, contours = _copy_out([(p, npt.value, SECTION_POINT_DTYPE, True), (s, ns.value, SECTION_SEGMENT_DTYPE, True),
                                                (c, nc.value, SECTION_CONTOUR_DTYPE, True)], lib().hfpf_free_section, p, s, c)
        return points, segments, contours, recs, summ.as_dict()

    def section_mesh_device(self, dev_verts, n_verts, vertex_stride, dev_tris, n_tris, pose=None, planes=(), opts=None):
        """hfpf_section_mesh_device on a mesh in HBM (as extract_mesh_device leaves it): section_mesh(device=True)."""
        return self.section_mesh(dev_verts, dev_tris, pose, planes, device=True, opts=opts, n_verts=n_verts, vertex_stride=vertex_stride, n_tris=n_tris)

    # -- open edges of a triangle mesh --
    def mesh_topology(self, verts, tris, pose=None, device=False, opts=None, tri_shell=True, n_verts=None, vertex_stride=None, n_tris=None):
        """Boundary loops, shells and watertightness of a triangle mesh (hfpf_mesh_topology): (edges of TOPOLOGY_EDGE_DTYPE, one per
        edge that is not interior; loops of TOPOLOGY_LOOP_DTYPE; shells of TOPOLOGY_SHELL_DTYPE; uint32 tri_shell, one per triangle, or
        None with tri_shell=False; summary dict).  verts, tris, pose and the device form's arguments as compare_mesh().  device=True
        runs hfpf_mesh_topology_device and returns the three record arrays as (pointer, count) pairs in HBM and tri_shell as a pointer
        (0 when not asked for): free the pointers with device_free (an empty array's is 0).  mesh_topology_device() is that form by
        name."""
        o = _or(opts, topology_opts)
        pose = _pose12(pose, identity=True)
        mesh, keep = _mesh_args(verts, tris, device, n_verts, vertex_stride, n_tris)
        e, l, s, t, ne, nl, ns, summ = (C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64(),
                                        TopologySummary())
        fn = lib().hfpf_mesh_topology_device if device else lib().hfpf_mesh_topology
        self._chk(fn(self._h, C.byref(o), *mesh, _p(pose), C.byref(e), C.byref(ne), C.byref(l), C.byref(nl), C.byref(s), C.byref(ns),
                     C.byref(t) if tri_shell else None, C.byref(summ)))
        if device:
            return (e.value or 0, ne.value), (l.value or 0, nl.value), (s.value or 0, ns.value), t.value or 0, summ.as_dict()
        edges, loops, shells, per_tri = _copy_out([(e, ne.value, TOPOLOGY_EDGE_DTYPE, True), (l, nl.value, TOPOLOGY_LOOP_DTYPE, True),
                                                   (s, ns.value, TOPOLOGY_SHELL_DTYPE, True), (t, mesh[4] if t.value else 0, np.uint32, tri_shell)],
                                                  lib().hfpf_free_topology, e, l, s, t)  # mesh[4]: n_tris
        return edges, loops, shells, per_tri, summ.as_dict()

    def mesh_topology_device(self, dev_verts, n_verts, vertex_stride, dev_tris, n_tris, pose=None, opts=None, tri_shell=True):
        """hfpf_mesh_topology_device on a mesh in HBM (as extract_mesh_device leaves it): mesh_topology(device=True)."""
        return self.mesh_topology(dev_verts, dev_tris, pose, device=True, opts=opts, tri_shell=tri_shell, n_verts=n_verts, vertex_stride=vertex_stride,
                                  n_tris=n_tris)

    # -- planning the next views against a reference mesh --
    def plan_views(self, verts, tris, poses, pose=None, device=False, opts=None, tri_plan=True, n_verts=None, vertex_stride=None, n_tris=None, **kw):
        """Score candidate camera poses by the reference surface they would add (hfpf_plan_views): (scores of VIEW_SCORE_DTYPE, one per
        view; records of TRI_PLAN_DTYPE, one per triangle, or None with tri_plan=False; summary dict).  poses: n 3x4 [R|t], camera ->
        fusion frame; verts, tris, pose and the device form's arguments as compare_mesh(); keywords as plan_opts().  device=True runs
        hfpf_plan_views_device and returns the records as a device pointer (0 without triangles or with tri_plan=False): free it with
        device_free."""
        o = _or(opts, plan_opts, **kw)
        pose = _pose12(pose, identity=True)
        poses = _poses(poses)
        n_views = len(poses)
        room = np.zeros(max(n_views, 1), VIEW_SCORE_DTYPE)  # never NULL, also without views
        mesh, keep = _mesh_args(verts, tris, device, n_verts, vertex_stride, n_tris)
        t, s = C.c_void_p(), PlanSummary()
        fn = lib().hfpf_plan_views_device if device else lib().hfpf_plan_views
        self._chk(fn(self._h, C.byref(o), *mesh, _p(pose), _p(poses) if n_views else None, n_views, _p(room), C.byref(t) if tri_plan else None,
                     C.byref(s)))
        if device:
            return room[:n_views], t.value or 0, s.as_dict()
        rec, = _copy_out([(t, mesh[4] if t.value else 0, TRI_PLAN_DTYPE, tri_plan)], lib().hfpf_free_plan, t)  # mesh[4]: n_tris
        return room[:n_views], rec, s.as_dict()

    # -- rows that depth frames see through --
    def depth_consistency(self, frames, poses, K, depth_scale=0.001, opts=None, rows=True, desc=None, depth_frame_stride=None, n_frames=None,
                          **kw):
        """What depth frames in pageable memory say about every row (hfpf_depth_consistency): (rows of ROW_DTYPE or None with
        rows=False, cons of ROW_CONSISTENCY_DTYPE, summary dict).  frames: an (n, H, W) uint16 or float32 array (rows and frames may be
        padded: a view of a larger array); poses: n 3x4 [R|t], camera -> fusion frame.  Keywords as consistency_opts().  desc,
        depth_frame_stride and n_frames override what the array's shape and strides give (frames is then any buffer)."""
        o = _or(opts, consistency_opts, **kw)
        frames = np.asarray(frames)
        if desc is None:
            if frames.ndim != 3:
                raise ValueError("frames must be an (n, H, W) array")
            d = _image_desc(frames[0] if len(frames) else np.zeros(frames.shape[1:], frames.dtype), K, None, None, depth_scale)
            n = len(frames)
            stride = frames.strides[0] if n else d.depth_step * d.height
        else:
            d, n, stride = desc, int(n_frames), int(depth_frame_stride)
        n = int(n_frames) if n_frames is not None else n
        stride = int(depth_frame_stride) if depth_frame_stride is not None else stride
        poses = _poses(poses, flat=True)
        r, c, nr, s = C.c_void_p(), C.c_void_p(), C.c_uint64(), ConsistencySummary()
        self._chk(lib().hfpf_depth_consistency(self._h, C.byref(o), C.byref(d), C.c_void_p(frames.ctypes.data) if frames.size else None, stride, n,
                                               _p(poses) if poses.size else None, C.byref(r) if rows else None, C.byref(c), C.byref(nr), C.byref(s)))
        out, cons = _copy_out([(r, nr.value, ROW_DTYPE, rows), (c, nr.value, ROW_CONSISTENCY_DTYPE, True)], lib().hfpf_free_consistency, r, c)
        return out, cons, s.as_dict()

    def depth_consistency_device(self, desc, dev_depth, depth_frame_stride, n_frames, poses, opts=None, rows=True, **kw):
        """The same for frames resident in HBM (hfpf_depth_consistency_device): (rows pointer or 0, cons pointer, n_rows, summary
        dict); free the pointers with device_free (they are 0 without rows)."""
        o = _or(opts, consistency_opts, **kw)
        poses = _poses(poses, flat=True)
        r, c, nr, s = C.c_void_p(), C.c_void_p(), C.c_uint64(), ConsistencySummary()
        self._chk(lib().hfpf_depth_consistency_device(self._h, C.byref(o), C.byref(desc), C.c_void_p(dev_depth), int(depth_frame_stride), int(n_frames),
                                                      _p(poses) if poses.size else None, C.byref(r) if rows else None, C.byref(c), C.byref(nr),
                                                      C.byref(s)))
        return r.value or 0, c.value or 0, nr.value, s.as_dict()

    # -- casting rays against the model --
    def raycast(self, rays, pose, opts=None, **kw):
        """First surface crossing of each ray (hfpf_raycast).  rays: (n, 6) float32 (origin, direction) in the camera frame or RAY_DTYPE
        records in pageable memory; pose = camera -> fusion frame 3x4.  Keywords as raycast_opts().  Returns RAY_HIT_DTYPE hits."""
        o = _or(opts, raycast_opts, **kw)
        rays = _rays(rays)
        pose = _pose12(pose)
        hits = np.empty(len(rays), RAY_HIT_DTYPE)
        self._chk(lib().hfpf_raycast(self._h, C.byref(o), _p(rays) if len(rays) else None, len(rays), _p(pose), _p(hits)))
        return hits

    def raycast_device(self, dev_rays, n_rays, pose, dev_hits=0, opts=None, **kw):
        """The same for rays resident in HBM (hfpf_raycast_device).  With dev_hits the hits stay in that device buffer and None is
        returned; otherwise they go to a scratch device buffer and come back as raycast() returns them."""
        o = _or(opts, raycast_opts, **kw)
        pose = _pose12(pose)
        got = self._device_results(n_rays, [(dev_hits, RAY_HIT_DTYPE, True)], lambda hits: self._chk(
            lib().hfpf_raycast_device(self._h, C.byref(o), C.c_void_p(dev_rays), n_rays, _p(pose), C.c_void_p(hits))))
        return got and got[0]

    def raycast_view(self, pose, K, width, height, opts=None, **kw):
        """The view rays of one pinhole view (hfpf_raycast_view): K = (fx, fy, cx, cy), t_range = (z_near, z_far); hit i = pixel
        (i % width, i // width), its t the camera-frame depth.  Returns (height, width) RAY_HIT_DTYPE hits."""
        o = _or(opts, raycast_opts, **kw)
        pose = _pose12(pose)
        hits = np.empty((int(height), int(width)), RAY_HIT_DTYPE)
        self._chk(lib().hfpf_raycast_view(self._h, C.byref(o), int(width), int(height), float(K[0]), float(K[1]), float(K[2]), float(K[3]),
                                          _p(pose), _p(hits) if hits.size else None))
        return hits

    def raycast_views_device(self, poses, K, width, height, dev_hits=0, opts=None, **kw):
        """A batch of views into HBM (hfpf_raycast_view_device): poses (n, 3, 4); view v's hits start v * width * height behind
        dev_hits.  Without dev_hits they go to a scratch device buffer and come back as (n, height, width) hits."""
        o = _or(opts, raycast_opts, **kw)
        poses = _poses(poses)
        n = len(poses) * int(width) * int(height)
        got = self._device_results(n, [(dev_hits, RAY_HIT_DTYPE, True)], lambda hits: self._chk(lib().hfpf_raycast_view_device(
            self._h, C.byref(o), int(width), int(height), float(K[0]), float(K[1]), float(K[2]), float(K[3]), len(poses),
            _p(poses) if len(poses) else None, C.c_void_p(hits))))
        return got and got[0].reshape(len(poses), int(height), int(width))

    def query_depth(self, depth, pose, K, depth_scale=0.001, opts=None, radius=1, min_count=0.0, max_distance=float("inf"), zclip=False,
                    rows=True):
        """Query every pixel of one depth image in pageable memory (hfpf_query_depth); hit / row i = pixel (i % W, i // W)."""
        d = _image_desc(depth, K, None, None, depth_scale)
        o = _or(opts, query_opts, radius, min_count, max_distance, zclip)
        pose = _pose12(pose)
        n = d.width * d.height
        hits = np.empty(n, QUERY_HIT_DTYPE)
        out = np.empty(n, ROW_DTYPE) if rows else None
        self._chk(lib().hfpf_query_depth(self._h, C.byref(o), C.byref(d), C.c_void_p(depth.ctypes.data), _p(pose), _p(hits),
                                         _p(out) if rows else None))
        return hits, out

    # -- multi-GPU --
    def dist_init_rccl(self, rank, world, unique_id):
        """unique_id: the 128 bytes rank 0 got from dist_unique_id(), broadcast by the launcher."""
        buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
        self._chk(lib().hfpf_dist_init(self._h, rank, world, buf))

    def dist_world(self):
        """Rank count the engine's RCCL communicator reports (1 without a communicator)."""
        r, w = C.c_int32(), C.c_int32()
        self._chk(lib().hfpf_dist_info(self._h, C.byref(r), C.byref(w)))
        return w.value

    def dist_disable(self):
        self._chk(lib().hfpf_dist_disable(self._h))

    def attach_transport(self, transport):
        self._transport = transport

    def epoch_export(self):
        """-> (device pointer, n_records) of the 16-byte records of the cells occupied and the frames integrated since the last exchange."""
        p = C.c_void_p()
        n = C.c_uint64()
        self._chk(lib().hfpf_epoch_export(self._h, C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def epoch_import(self, dev_ptr, n_records):
        self._chk(lib().hfpf_epoch_import(self._h, C.c_void_p(dev_ptr), n_records))

    def epoch_import_gathered(self, dev_buffer, slice_stride_bytes, world, my_rank, counts):
        """Import every other rank's slice of a padded all-gather buffer (the layout ncclAllGather leaves behind)."""
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        self._chk(lib().hfpf_epoch_import_gathered(self._h, C.c_void_p(dev_buffer), slice_stride_bytes, world, my_rank, _p(c)))

    def device_copy(self, dev_dst, dev_src, nbytes):
        self._chk(lib().hfpf_device_copy(self._h, C.c_void_p(dev_dst), C.c_void_p(dev_src), nbytes))

    def stats_export(self):
        """-> (dev ptr, n_words, colour dev ptr or 0, n_colour_words) of this handle's partial int64 sums."""
        p, pc = C.c_void_p(), C.c_void_p()
        n, nc = C.c_uint64(), C.c_uint64()
        self._chk(lib().hfpf_stats_export(self._h, C.byref(p), C.byref(n), C.byref(pc), C.byref(nc)))
        return p.value or 0, n.value, pc.value or 0, nc.value

    def extract_with_stats(self, dev_words, dev_cwords=0):
        rows = C.c_void_p()
        n = C.c_uint64()
        self._chk(lib().hfpf_extract_with_stats(self._h, C.c_void_p(dev_words), C.c_void_p(dev_cwords) if dev_cwords else None,
                                                C.byref(rows), C.byref(n)))
        return self._rows_out(rows, n)

    def device_download(self, dev_ptr, nbytes, dtype=np.uint8):
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        self._chk(lib().hfpf_device_download(self._h, _p(out), C.c_void_p(dev_ptr), out.nbytes))
        return out

    def download_data(self, cloud_location, metadata):
        """downloadData(cloud_location, metadata): writes test_cloud.pcd and meta.csv; returns the rows."""
        rows = self.extract()
        write_pcd(rows, cloud_location)
        write_meta_csv(rows, metadata)
        return rows

    def clear(self):
        self._chk(lib().hfpf_clear(self._h))

    # -- hiding rows from every read-out --
    def hide_voxels(self, voxels, op="hide", select=None, select_mask=0, select_value=0, device=False, n=None, voxel_stride=None,
                    select_stride=None, opts=None):
        """hfpf_hide_voxels: op on the voxels of a list; returns the counts as a dict.  voxels: an (n, 3) int32 array (stride 12), a
        ROW_DTYPE array (stride 64), or any array whose rows begin with three int32, `voxel_stride` bytes apart.  select: an array of
        one uint32 word per entry, `select_stride` bytes apart (default: its item size); entry i is selected iff (word & select_mask)
        == select_value.  device=True (hfpf_hide_voxels_device): voxels and select are device pointers, and n, voxel_stride (and
        select_stride with a selector) are required."""
        o = _or(opts, hide_opts, op, select_mask, select_value)
        res = _sized(HideResult)
        if device:
            self._chk(lib().hfpf_hide_voxels_device(self._h, C.byref(o), C.c_void_p(voxels), int(n), int(voxel_stride), C.c_void_p(select) if select else None,
                                                    int(select_stride or 0), C.byref(res)))
            return res.as_dict()
        voxels = np.asarray(voxels)
        if voxels.dtype.names is None and voxel_stride is None:
            voxels = np.ascontiguousarray(voxels, dtype=np.int32).reshape(-1, 3)
        n = len(voxels) if n is None else int(n)
        vs = int(voxel_stride) if voxel_stride is not None else (voxels.strides[0] if len(voxels) > 1 else max(12, voxels.dtype.itemsize))
        ss = 0
        if select is not None:
            ss = int(select_stride) if select_stride is not None else (select.strides[0] if len(select) else select.dtype.itemsize)
        self._chk(lib().hfpf_hide_voxels(self._h, C.byref(o), C.c_void_p(voxels.ctypes.data) if n else None, n, vs,
                                         C.c_void_p(select.ctypes.data) if select is not None else None, ss, C.byref(res)))
        return res.as_dict()

    def hide_box(self, lo, hi, op="hide"):
        """hfpf_hide_box: op on the voxels lo..hi (inclusive indices; the box may reach outside the grid); returns the counts."""
        lo3, hi3 = np.ascontiguousarray(lo, dtype=np.int32).reshape(3), np.ascontiguousarray(hi, dtype=np.int32).reshape(3)
        res = _sized(HideResult)
        self._chk(lib().hfpf_hide_box(self._h, HIDE_OPS.get(op, op), _p(lo3), _p(hi3), C.byref(res)))
        return res.as_dict()

    def show_all(self):
        """hfpf_show_all: nothing is hidden any more."""
        self._chk(lib().hfpf_show_all(self._h))

    def hidden(self):
        """hfpf_get_hidden: the hidden voxels, (n, 3) int32 in ascending (x, y, z) order."""
        n = C.c_uint64()
        self._chk(lib().hfpf_get_hidden(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 3), dtype=np.int32)
        if n.value:
            self._chk(lib().hfpf_get_hidden(self._h, _p(out), n.value, C.byref(n)))
        return out

    # -- keeping a session --
    def snapshot(self):
        """hfpf_snapshot: the handle's state as a uint8 numpy array over the engine's host buffer (bytes-like: bytes(a), a.tobytes(),
        memoryview(a), file.write(a) all work); freed when the array is collected."""
        p, n = C.c_void_p(), C.c_uint64()
        self._chk(lib().hfpf_snapshot(self._h, C.byref(p), C.byref(n)))
        return np.asarray(_SnapshotBuffer(p.value, n.value))

    def restore(self, blob):
        """hfpf_restore: clear, then put the state of `blob` (bytes-like) in place."""
        raw = np.frombuffer(blob, dtype=np.uint8)
        self._chk(lib().hfpf_restore(self._h, _p(raw) if raw.size else None, raw.size))

    def save(self, path):
        """hfpf_save: the bytes of snapshot(), written to a file."""
        self._chk(lib().hfpf_save(self._h, os.fsencode(path)))

    def load(self, path):
        """hfpf_load: restore() from a file written by save()."""
        self._chk(lib().hfpf_load(self._h, os.fsencode(path)))

    # -- diagnostics / harness --
    def sync(self):
        self._chk(lib().hfpf_sync(self._h))

    def counters(self):
        c = Counters()
        self._chk(lib().hfpf_get_counters(self._h, C.byref(c)))
        return {n: getattr(c, n) for n, _ in Counters._fields_}

    def occupied(self):
        n = C.c_uint64()
        self._chk(lib().hfpf_get_occupied(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 3), dtype=np.int32)
        if n.value:
            self._chk(lib().hfpf_get_occupied(self._h, _p(out), n.value, C.byref(n)))
        return out

    def device_alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(lib().hfpf_device_alloc(self._h, nbytes, C.byref(p)))
        return p.value

    def device_free(self, ptr):
        self._chk(lib().hfpf_device_free(self._h, C.c_void_p(ptr)))

    def device_upload(self, dev_ptr, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(lib().hfpf_device_upload(self._h, C.c_void_p(dev_ptr), _p(arr), arr.nbytes))

    def kernel_timing(self, enable=True):
        """True / 1: integrate calls and clean passes; 2: also each kernel of an integrate call (kernel_time ids 2..4)."""
        self._chk(lib().hfpf_kernel_timing(self._h, int(enable)))

    def kernel_time(self, kernel_id=0):
        ms = C.c_double()
        n = C.c_uint64()
        self._chk(lib().hfpf_get_kernel_time(self._h, kernel_id, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # -- leaf probes (tests) --
    def probe_points(self, pose, xyz):
        pose = _pose12(pose)
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        n = xyz.shape[0]
        q = np.zeros((n, 3), np.float32)
        idx = np.zeros((n, 3), np.int32)
        flags = np.zeros(n, np.uint8)
        self._chk(lib().hfpf_probe_points(self._h, _p(pose), _p(xyz), n, _p(q), _p(idx), _p(flags)))
        return q, idx, flags

    def probe_normals(self, cells, occ, vps):
        cells = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 3)
        n = cells.shape[0]
        occ = np.ascontiguousarray(occ, dtype=np.uint8).reshape(n, 125)
        vps = np.ascontiguousarray(vps, dtype=np.float32).reshape(n, 3)
        normals = np.zeros((n, 3), np.float32)
        totals = np.zeros(n, np.int32)
        self._chk(lib().hfpf_probe_normals(self._h, n, _p(cells), _p(occ), _p(vps), _p(normals), _p(totals)))
        return normals, totals

    def probe_project(self, pts, centres, normals):
        pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
        n = pts.shape[0]
        centres = np.ascontiguousarray(centres, dtype=np.float32).reshape(n, 3)
        normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(n, 3)
        proj = np.zeros((n, 3), np.float32)
        dist = np.zeros(n, np.float64)
        member = np.zeros(n, np.uint8)
        self._chk(lib().hfpf_probe_project(self._h, n, _p(pts), _p(centres), _p(normals), _p(proj), _p(dist), _p(member)))
        # bit 0: the reference's form (f32 sqrt widened, compared with the radius); bit 1: the kernels' form (squared
        # distance against the precomputed largest passing value) -- kept for the test that the two always agree
        self.last_member_kernel_form = (member & 2) != 0
        self.last_hoisted_division_same = (member & 4) != 0
        return proj, dist, (member & 1) != 0

    def probe_depth(self, depth, K, color=None, color_format=None, depth_scale=0.001):
        """The kernels' depth-pixel loads + back-projection on one image: (H*W x 3 f32 xyz, H*W u32 rgb)."""
        d = _image_desc(depth, K, color, color_format, depth_scale)
        n = d.width * d.height
        xyz = np.zeros((n, 3), np.float32)
        rgb = np.zeros(n, np.uint32)
        self._chk(lib().hfpf_probe_depth(self._h, C.byref(d), C.c_void_p(depth.ctypes.data),
                                         C.c_void_p(color.ctypes.data) if color is not None else None, _p(xyz), _p(rgb)))
        return xyz, rgb

    def probe_trig(self, y, x):
        y = np.ascontiguousarray(y, dtype=np.float32)
        x = np.ascontiguousarray(x, dtype=np.float32)
        a = np.zeros_like(x)
        c = np.zeros_like(x)
        s = np.zeros_like(x)
        self._chk(lib().hfpf_probe_trig(self._h, x.size, _p(y), _p(x), _p(a), _p(c), _p(s)))
        return a, c, s


def dist_unique_id():
    buf = (C.c_char * 128)()
    rc = lib().hfpf_dist_unique_id(buf)
    if rc != 0:
        raise HfpfError(rc, lib().hfpf_last_error(None).decode())
    return bytes(buf)


def write_pcd(rows, path):
    rows = np.ascontiguousarray(rows, dtype=ROW_DTYPE)
    rc = lib().hfpf_write_pcd(_p(rows), rows.size, os.fsencode(path))
    if rc != 0:
        raise HfpfError(rc, "write_pcd(%s)" % path)


def write_meta_csv(rows, path):
    rows = np.ascontiguousarray(rows, dtype=ROW_DTYPE)
    rc = lib().hfpf_write_meta_csv(_p(rows), rows.size, os.fsencode(path))
    if rc != 0:
        raise HfpfError(rc, "write_meta_csv(%s)" % path)


def write_pcd_xyzrgb(rows, path, min_count=0, classify_threshold=-1, white=True):
    """download / downloadHQ(threshold) / downloadClassified of the reference (grid.hpp:491-575)."""
    rows = np.ascontiguousarray(rows, dtype=ROW_DTYPE)
    rc = lib().hfpf_write_pcd_xyzrgb(_p(rows), rows.size, os.fsencode(path), min_count, classify_threshold, 1 if white else 0)
    if rc != 0:
        raise HfpfError(rc, "write_pcd_xyzrgb(%s)" % path)


def write_pcd_binary(rows, path):
    rows = np.ascontiguousarray(rows, dtype=ROW_DTYPE)
    rc = lib().hfpf_write_pcd_binary(_p(rows), rows.size, os.fsencode(path))
    if rc != 0:
        raise HfpfError(rc, "write_pcd_binary(%s)" % path)
