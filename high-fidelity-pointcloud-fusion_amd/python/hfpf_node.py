"""ctypes binding of the ROS-free node shell (host/libhfpf_node.so, include/hfpf_node.h): the harness that stands in
for roscpp/tf2 so the start/stop/reset/process state machine of pointcloud_fusion_and_filter can be driven in tests."""
import ctypes as C
import os

import numpy as np

import hfpf

_LIB_PATH = os.path.join(hfpf.PKG_DIR, "host", "libhfpf_node.so")
_lib = None

PUBLISH_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p)
TF_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_char), C.c_uint32)

EXPORTS = ["hfpf_node_default_params", "hfpf_node_create", "hfpf_node_destroy", "hfpf_node_last_error", "hfpf_node_on_point_cloud",
           "hfpf_node_start", "hfpf_node_stop", "hfpf_node_reset", "hfpf_node_process", "hfpf_node_clean_now", "hfpf_node_grid",
           "hfpf_node_get_stats", "hfpf_node_set_publisher", "hfpf_node_on_depth_image",
           "hfpf_node_set_mesh_output", "hfpf_node_save_session", "hfpf_node_load_session", "hfpf_node_set_component_filter",
           "hfpf_node_set_reference_mesh", "hfpf_node_set_reference_alignment", "hfpf_node_set_reference_coverage",
           "hfpf_node_set_view_candidates", "hfpf_node_set_section_planes", "hfpf_node_set_mesh_topology",
           "hfpf_node_set_depth_consistency", "hfpf_node_set_hide_filtered", "hfpf_node_hide_box"]


class Params(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("fusion_frame", C.c_char_p), ("directory_name", C.c_char_p),
                ("bounding_box", C.POINTER(C.c_double)), ("bounding_box_len", C.c_uint32), ("engine", hfpf.Config),
                ("clean_period_s", C.c_double), ("final_clean_on_process", C.c_int32), ("write_variants", C.c_int32)]


class CloudMsg(C.Structure):
    _fields_ = [("data", C.c_void_p), ("height", C.c_uint32), ("width", C.c_uint32), ("point_step", C.c_uint32),
                ("row_step", C.c_uint32), ("off_x", C.c_uint32), ("off_y", C.c_uint32), ("off_z", C.c_uint32),
                ("off_rgb", C.c_uint32), ("frame_id", C.c_char_p)]


class DepthMsg(C.Structure):
    _fields_ = [("depth", C.c_void_p), ("color", C.c_void_p), ("image", hfpf.DepthImage), ("frame_id", C.c_char_p)]


class TriggerResponse(C.Structure):
    _fields_ = [("success", C.c_int32), ("message", C.c_char * 256)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("received", "integrated", "dropped_not_started", "dropped_tf", "clean_passes", "process_calls")] + \
               [("started", C.c_int32), ("cloud_subscription_started", C.c_int32)]


def lib():
    global _lib
    if _lib is None:
        hfpf.lib()
        L = C.CDLL(_LIB_PATH)
        L.hfpf_node_default_params.argtypes = [C.POINTER(Params)]
        L.hfpf_node_default_params.restype = None
        L.hfpf_node_create.argtypes = [C.POINTER(Params), TF_FN, C.c_void_p, C.POINTER(C.c_void_p)]
        L.hfpf_node_destroy.argtypes = [C.c_void_p]
        L.hfpf_node_last_error.argtypes = [C.c_void_p]
        L.hfpf_node_last_error.restype = C.c_char_p
        L.hfpf_node_on_point_cloud.argtypes = [C.c_void_p, C.POINTER(CloudMsg)]
        L.hfpf_node_on_depth_image.argtypes = [C.c_void_p, C.POINTER(DepthMsg)]
        for f in ("start", "stop", "reset", "process"):
            getattr(L, "hfpf_node_" + f).argtypes = [C.c_void_p, C.POINTER(TriggerResponse)]
        L.hfpf_node_clean_now.argtypes = [C.c_void_p]
        L.hfpf_node_grid.argtypes = [C.c_void_p]
        L.hfpf_node_grid.restype = C.c_void_p
        L.hfpf_node_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
        L.hfpf_node_set_publisher.argtypes = [C.c_void_p, PUBLISH_FN, C.c_void_p]
        L.hfpf_node_set_mesh_output.argtypes = [C.c_void_p, C.POINTER(hfpf.MeshOpts)]
        L.hfpf_node_set_section_planes.argtypes = [C.c_void_p, C.POINTER(hfpf.SectionOpts), C.c_void_p, C.c_uint32]
        L.hfpf_node_set_mesh_topology.argtypes = [C.c_void_p, C.POINTER(hfpf.TopologyOpts)]
        L.hfpf_node_set_component_filter.argtypes = [C.c_void_p, C.POINTER(hfpf.ComponentOpts)]
        L.hfpf_node_set_reference_mesh.argtypes = [C.c_void_p, C.POINTER(hfpf.DeviationOpts), C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                                   C.c_uint64, C.c_void_p]
        L.hfpf_node_set_reference_alignment.argtypes = [C.c_void_p, C.POINTER(hfpf.AlignOpts)]
        L.hfpf_node_set_reference_coverage.argtypes = [C.c_void_p, C.POINTER(hfpf.CoverOpts)]
        L.hfpf_node_set_view_candidates.argtypes = [C.c_void_p, C.POINTER(hfpf.PlanOpts), C.c_void_p, C.c_uint32]
        L.hfpf_node_set_depth_consistency.argtypes = [C.c_void_p, C.POINTER(hfpf.ConsistencyOpts), C.c_uint32]
        L.hfpf_node_set_hide_filtered.argtypes = [C.c_void_p, C.c_int]
        L.hfpf_node_hide_box.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(hfpf.HideResult)]
        L.hfpf_node_save_session.argtypes = [C.c_void_p, C.c_char_p]
        L.hfpf_node_load_session.argtypes = [C.c_void_p, C.c_char_p]
        _lib = L
    return _lib


class FusionNode:
    """pointcloud_fusion_and_filter without ROS: params in, Trigger services and the cloud callback as methods."""

    def __init__(self, bounding_box, directory_name="./", fusion_frame="fusion_frame", tf_lookup=None, clean_period_s=0.0,
                 final_clean_on_process=False, resolution=None, write_variants=False, publisher=None, **caps):
        L = lib()
        p = Params()
        L.hfpf_node_default_params(C.byref(p))
        self._keep = [fusion_frame.encode(), os.fsencode(directory_name), (C.c_double * len(bounding_box))(*bounding_box)]
        p.fusion_frame, p.directory_name = self._keep[0], self._keep[1]
        p.bounding_box = C.cast(self._keep[2], C.POINTER(C.c_double))
        p.bounding_box_len = len(bounding_box)
        if resolution is not None:
            p.engine.resolution = resolution
        for k, v in caps.items():
            setattr(p.engine, k, v)
        p.clean_period_s = clean_period_s
        p.final_clean_on_process = 1 if final_clean_on_process else 0
        p.write_variants = 1 if write_variants else 0
        self._tf_py = tf_lookup
        self._pub_py = publisher

        def _tf(user, target, source, pose, err, cap):
            if self._tf_py is None:
                return 0
            try:
                T = np.ascontiguousarray(self._tf_py(target.decode(), source.decode()), dtype=np.float64).reshape(12)
            except Exception as e:  # stands for tf2::TransformException
                msg = str(e).encode()[:cap - 1]
                C.memmove(err, msg, len(msg))
                return 1
            for i in range(12):
                pose[i] = T[i]
            return 0
        self._tf_c = TF_FN(_tf)
        self._h = C.c_void_p()
        rc = L.hfpf_node_create(C.byref(p), self._tf_c, None, C.byref(self._h))
        if rc != 0:
            self._h = None
            raise hfpf.HfpfError(rc, L.hfpf_node_last_error(None).decode())

        def _pub(user, rows, n_rows, frame_id):  # the rows are only valid during the call: copy
            arr = np.frombuffer((C.c_char * (n_rows * hfpf.ROW_DTYPE.itemsize)).from_address(rows), dtype=hfpf.ROW_DTYPE).copy() if n_rows else \
                np.zeros(0, dtype=hfpf.ROW_DTYPE)
            self._pub_py(arr, frame_id.decode())
        self._pub_c = PUBLISH_FN(_pub)
        if publisher is not None:
            L.hfpf_node_set_publisher(self._h, self._pub_c, None)

    def close(self):
        if getattr(self, "_h", None):
            lib().hfpf_node_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _srv(self, name):
        r = TriggerResponse()
        rc = getattr(lib(), "hfpf_node_" + name)(self._h, C.byref(r))
        return rc, bool(r.success), r.message.decode()

    def start(self):
        return self._srv("start")

    def stop(self):
        return self._srv("stop")

    def reset(self):
        return self._srv("reset")

    def process(self):
        return self._srv("process")

    def publish(self, buf, height, width, point_step=16, offsets=(0, 4, 8, 12), frame_id="camera"):
        """A PointCloud2 arriving on ~input_point_cloud.  Returns 1 integrated / 0 dropped."""
        buf = np.ascontiguousarray(buf)
        m = CloudMsg(buf.ctypes.data, height, width, point_step, width * point_step, offsets[0], offsets[1], offsets[2], offsets[3],
                     frame_id.encode())
        rc = lib().hfpf_node_on_point_cloud(self._h, C.byref(m))
        if rc < 0:
            raise hfpf.HfpfError(rc, lib().hfpf_node_last_error(self._h).decode())
        return rc

    def publish_depth(self, depth, K, color=None, color_format=None, depth_scale=0.001, frame_id="camera"):
        """A synchronised depth Image (+ colour Image) with its CameraInfo K = (fx, fy, cx, cy).  Returns 1 / 0 as publish."""
        d = hfpf._image_desc(depth, K, color, color_format, depth_scale)
        m = DepthMsg(depth.ctypes.data, color.ctypes.data if color is not None else None, d, frame_id.encode())
        rc = lib().hfpf_node_on_depth_image(self._h, C.byref(m))
        if rc < 0:
            raise hfpf.HfpfError(rc, lib().hfpf_node_last_error(self._h).decode())
        return rc

    def clean_now(self):
        rc = lib().hfpf_node_clean_now(self._h)
        if rc < 0:
            raise hfpf.HfpfError(rc, lib().hfpf_node_last_error(self._h).decode())
        return rc

    def set_mesh_output(self, opts=None, **kw):
        """~process also writes <directory_name>/mesh.ply with these hfpf.mesh_opts (or its keywords); set_mesh_output(None) with no
        keywords turns it off."""
        o = opts if opts is not None else (hfpf.mesh_opts(**kw) if kw else None)
        rc = lib().hfpf_node_set_mesh_output(self._h, C.byref(o) if o is not None else None)
        if rc < 0:
            raise hfpf.HfpfError(rc, lib().hfpf_node_last_error(self._h).decode())

    def set_mesh_topology(self, on=True, opts=None):
        """~process also writes mesh_edges.csv, mesh_loops.csv, mesh_shells.csv and mesh_topology_summary.csv: hfpf_mesh_topology_device
        of the mesh it writes to mesh.ply; it needs set_mesh_output.  set_mesh_topology(False) turns it off."""
        o = (opts if opts is not None else hfpf.topology_opts()) if on else None
        rc = lib().hfpf_node_set_mesh_topology(self._h, C.byref(o) if o is not None else None)
        if rc < 0:
            raise hfpf.HfpfError(rc, lib().hfpf_node_last_error(self._h).decode())

    def set_section_planes(self, planes=None, opts=None, n_planes=None):
        """~process also writes sections.csv and section_summary.csv: hfpf_section_mesh of the mesh it writes to mesh.ply with these
        planes ((n, 4) float64 rows n.x, n.y, n.z, d in the fusion frame); it needs set_mesh_output.  set_section_planes(None) turns it
        off.  n_planes overrides the count handed over (for the 4096-plane limit)."""
        if planes is None:
            rc = lib().hfpf_node_set_section_planes(self._h, None, None, 0)
        else:
            o = opts if opts is not None else hfpf.section_opts()
            planes = np.ascontiguousarray(planes, np.float64).reshape(-1, 4)
            rc = lib().hfpf_node_set_section_planes(self._h, C.byref(o), planes.ctypes.data if planes.size else None,
                                                    len(planes) if n_planes is None else int(n_planes))
        if rc < 0:
            raise hfpf.HfpfError(rc, lib().hfpf_node_last_error(self._h).decode())

    def set_component_filter(self, opts=None, **kw):
        """~process saves only the rows of the components hfpf_extract_components keeps with these hfpf.component_opts (or its
        keywords); set_component_filter(None) with no keywords turns it off."""
        o = opts if opts is not None else (hfpf.component_opts(**kw) if kw else None)
        rc = lib().hfpf_node_set_component_filter(self._h, C.byref(o) if o is not None else None)
        if rc < 0:
            raise hfpf.HfpfError(rc, lib().hfpf_node_last_error(self._h).decode())

    def set_reference_mesh(self, verts=None, tris=None, pose=None, opts=None, **kw):
        """~process also writes deviation.csv and deviation_summary.csv: the saved cloud against this mesh (hfpf.MESH_VERTEX_DTYPE or
        (n, 3) float32 vertices, (n, 3) uint32 triangles, a 3x4 pose mesh frame -> fusion frame, identity by default; options as
        hfpf.deviation_opts).  set_reference_mesh() with no mesh turns it off."""
        if verts is None:
            rc = lib().hfpf_node_set_reference_mesh(self._h, None, None, 0, 12, None, 0, None)
        else:
            o = opts if opts is not None else hfpf.deviation_opts(**kw)
            verts = np.ascontiguousarray(verts)
            if verts.dtype != hfpf.MESH_VERTEX_DTYPE:
                verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
            stride = 32 if verts.dtype == hfpf.MESH_VERTEX_DTYPE else 12
            tris = np.ascontiguousarray(tris, np.uint32).reshape(-1, 3)
            pose = np.ascontiguousarray(np.eye(4)[:3] if pose is None else pose, np.float64).reshape(12)
            rc = lib().hfpf_node_set_reference_mesh(self._h, C.byref(o), verts.ctypes.data_as(C.c_void_p), len(verts), stride,
                                                    tris.ctypes.data_as(C.c_void_p), len(tris), pose.ctypes.data_as(C.c_void_p))
        if rc < 0:
            raise hfpf.HfpfError(rc, lib().hfpf_node_last_error(self._h).decode())

    def set_reference_alignment(self, opts=None, **kw):
        """~process best-fits the reference mesh from its pose (hfpf_align_mesh with these hfpf.align_opts, or its keywords) before it
        compares, and also writes alignment.csv; set_reference_alignment(None) with no keywords turns it off."""
        o = opts if opts is not None else (hfpf.align_opts(**kw) if kw else None)
        rc = lib().hfpf_node_set_reference_alignment(self._h, C.byref(o) if o is not None else None)
        if rc < 0:
            raise hfpf.HfpfError(rc, lib().hfpf_node_last_error(self._h).decode())

    def set_view_candidates(self, poses=None, opts=None, **kw):
        """~process also writes view_plan.csv and view_plan_summary.csv: hfpf_plan_views of the reference mesh for these candidate
        poses (n 3x4 [R|t], camera -> fusion frame) with these hfpf.plan_opts, or its keywords, at the pose the deviation files use;
        set_view_candidates(None) turns it off."""
        o = None if poses is None else (opts if opts is not None else hfpf.plan_opts(**kw))
        p = np.ascontiguousarray(poses if poses is not None else np.zeros((0, 12)), np.float64).reshape(-1, 12)
        rc = lib().hfpf_node_set_view_candidates(self._h, C.byref(o) if o is not None else None, p.ctypes.data if len(p) else None, len(p))
        if rc < 0:
            raise hfpf.HfpfError(rc, lib().hfpf_node_last_error(self._h).decode())

    def set_reference_coverage(self, opts=None, **kw):
        """~process also writes coverage.csv and coverage_summary.csv: hfpf_cover_mesh of the reference mesh (these hfpf.cover_opts, or
        its keywords) at the pose the deviation files use; set_reference_coverage(None) with no keywords turns it off."""
        o = opts if opts is not None else (hfpf.cover_opts(**kw) if kw else None)
        rc = lib().hfpf_node_set_reference_coverage(self._h, C.byref(o) if o is not None else None)
        if rc < 0:
            raise hfpf.HfpfError(rc, lib().hfpf_node_last_error(self._h).decode())

    def set_depth_consistency(self, opts=None, keep_frames=64, **kw):
        """~process also writes consistency.csv and consistency_summary.csv: hfpf_depth_consistency (these hfpf.consistency_opts, or
        its keywords) of the last keep_frames depth images the node integrated; set_depth_consistency(None) with no keywords turns it
        off."""
        o = opts if opts is not None else (hfpf.consistency_opts(**kw) if kw else None)
        rc = lib().hfpf_node_set_depth_consistency(self._h, C.byref(o) if o is not None else None, int(keep_frames))
        if rc < 0:
            raise hfpf.HfpfError(rc, lib().hfpf_node_last_error(self._h).decode())

    def set_hide_filtered(self, on=True):
        """With a component filter set, ~process hides the rows the filter drops (hfpf_hide_voxels_device), so that mesh.ply, the
        variants and the reports leave them out as test_cloud.pcd does; off by default."""
        rc = lib().hfpf_node_set_hide_filtered(self._h, 1 if on else 0)
        if rc < 0:
            raise hfpf.HfpfError(rc, lib().hfpf_node_last_error(self._h).decode())

    def hide_box(self, box_m, op="hide"):
        """hfpf_node_hide_box: op ("hide", "show", "hide_others") on a box in fusion-frame metres (xmin, xmax, ymin, ymax, zmin, zmax);
        returns the counts of hfpf_hide_box."""
        box = np.ascontiguousarray(box_m, np.float64).reshape(6)
        res = hfpf.HideResult()
        res.struct_size = C.sizeof(hfpf.HideResult)
        rc = lib().hfpf_node_hide_box(self._h, hfpf.HIDE_OPS.get(op, op), box.ctypes.data_as(C.c_void_p), C.byref(res))
        if rc < 0:
            raise hfpf.HfpfError(rc, lib().hfpf_node_last_error(self._h).decode())
        return res.as_dict()

    def save_session(self, path):
        """The grid's session to a file (hfpf_save); legal while capture and the clean thread run."""
        rc = lib().hfpf_node_save_session(self._h, os.fsencode(path))
        if rc < 0:
            raise hfpf.HfpfError(rc, lib().hfpf_node_last_error(self._h).decode())

    def load_session(self, path):
        """Replace the grid's session by a saved one (hfpf_load); the node stays started or stopped as it was."""
        rc = lib().hfpf_node_load_session(self._h, os.fsencode(path))
        if rc < 0:
            raise hfpf.HfpfError(rc, lib().hfpf_node_last_error(self._h).decode())

    def stats(self):
        s = Stats()
        lib().hfpf_node_get_stats(self._h, C.byref(s))
        return {n: getattr(s, n) for n, _ in Stats._fields_}
