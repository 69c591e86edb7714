/* include/hfpf_node.h -- ROS-free shell of the reference node `pointcloud_fusion_and_filter`.
 *
 * Reproduces the control surface of class PointcloudFusion
 * (pointcloud_fusion/pointcloud_fusion/src/pointcloud_fusion_and_filter.cpp:99-169,327-440, "node.cpp") on top of
 * libhfpf.so: the four std_srvs/Trigger services, the PointCloud2 subscriber callback with its tf lookup, the
 * periodic clean thread and the two output files.  ROS itself is absent from this image, so the shell takes plain
 * structs; host/ros_shell.cpp (built only where catkin/roscpp exist) maps the ROS types onto it 1:1.
 */
#ifndef HFPF_NODE_H
#define HFPF_NODE_H
#include "hfpf.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct hfpf_node hfpf_node;

typedef struct hfpf_node_params {
    uint32_t struct_size;
    const char* fusion_frame;        /* private param `fusion_frame`, default "fusion_frame" (node.cpp:447) */
    const char* directory_name;      /* private param `directory_name`, default "./" (node.cpp:449) */
    const double* bounding_box;      /* private param `bounding_box` (node.cpp:451): xmin,xmax,ymin,ymax,zmin,zmax */
    uint32_t bounding_box_len;       /* must be 6; the reference indexes box[0..5] unchecked (node.cpp:162) */
    hfpf_config engine;              /* every other engine knob; bbox is overwritten from bounding_box */
    double clean_period_s;           /* 5.0 = sleep(5) of cleanGrid (node.cpp:323); <= 0: no thread, use hfpf_node_clean_now */
    int32_t final_clean_on_process;  /* 0 = reference behaviour (process does not clean first, node.cpp:377-398) */
    int32_t write_variants;          /* 1 = also write the files of the reference's `#if 0` block (node.cpp:399-437):
                                        test_cloud_{50,100,150,200,250,300}.pcd (downloadHQ), test_cloud_classified.pcd,
                                        test_cloud_normals.pcd; each a device-side filtered extract.  0 = reference behaviour */
} hfpf_node_params;

/* sensor_msgs/PointCloud2 as the decoder uses it (node.cpp:182-216): fields[0..3] = x,y,z,rgb. */
typedef struct hfpf_cloud_msg {
    const void* data;
    uint32_t height, width, point_step, row_step;
    uint32_t off_x, off_y, off_z, off_rgb; /* fields[0..3].offset */
    const char* frame_id;                  /* header.frame_id */
} hfpf_cloud_msg;

/* A registered depth image (+ colour image) of an RGB-D camera: two sensor_msgs/Image of one stamp and the depth camera's
 * CameraInfo (approximate-time synchronised by the caller).  `image` carries width, height, both encodings as HFPF_DEPTH_* /
 * HFPF_COLOR_*, both row steps and K (include/hfpf.h, hfpf_depth_image). */
typedef struct hfpf_depth_msg {
    const void* depth;      /* depth Image data */
    const void* color;      /* colour Image data, or NULL with image.color_format = HFPF_COLOR_NONE */
    hfpf_depth_image image;
    const char* frame_id;   /* header.frame_id of the depth image */
} hfpf_depth_msg;

/* std_srvs/TriggerResponse */
typedef struct hfpf_trigger_response {
    int32_t success;
    char message[256];
} hfpf_trigger_response;

/* tf_buffer_.lookupTransform(target, source, ros::Time(0)) (node.cpp:336): return 0 and fill the row-major 3x4
 * pose target<-source, or non-zero for a tf2::TransformException (text in err). */
typedef int (*hfpf_tf_lookup_fn)(void* user, const char* target_frame, const char* source_frame, double pose_3x4[12],
                                 char* err, uint32_t err_cap);

void hfpf_node_default_params(hfpf_node_params* p);
/* PointcloudFusion::PointcloudFusion (node.cpp:146-169): builds the grid, starts the clean thread. */
int hfpf_node_create(const hfpf_node_params* p, hfpf_tf_lookup_fn tf, void* tf_user, hfpf_node** out);
int hfpf_node_destroy(hfpf_node* n);
const char* hfpf_node_last_error(const hfpf_node* n);

/* onReceivedPointCloud (node.cpp:327-349) + the two capture threads (node.cpp:218-299).
 * Returns 1 = integrated, 0 = dropped (not started, or tf failure: warn + drop, node.cpp:340-344), < 0 = error.
 * Only the first row is consumed: n = row_step / point_step (node.cpp:185,190). */
int hfpf_node_on_point_cloud(hfpf_node* n, const hfpf_cloud_msg* msg);

/* The same callback for a depth frame: the start/stop gating, frame bookkeeping and tf lookup of hfpf_node_on_point_cloud by
 * msg->frame_id, then hfpf_integrate_depth.  Same return values. */
int hfpf_node_on_depth_image(hfpf_node* n, const hfpf_depth_msg* msg);

/* ~start ~stop ~reset ~process (node.cpp:154-157, 351-440). start/stop/reset set success=true like the reference;
 * process writes <directory_name>/test_cloud.pcd and /meta.csv (node.cpp:395-396), clears the grid (node.cpp:438)
 * and -- documented deviation -- reports success=true with a message (the reference never sets the response). */
int hfpf_node_start(hfpf_node* n, hfpf_trigger_response* res);
int hfpf_node_stop(hfpf_node* n, hfpf_trigger_response* res);
int hfpf_node_reset(hfpf_node* n, hfpf_trigger_response* res);
int hfpf_node_process(hfpf_node* n, hfpf_trigger_response* res);

/* The latent publisher of the reference: it advertises `~pcl_fusion_node/processed_cloud_normals` (sensor_msgs/PointCloud2,
 * node.cpp:138,158) and never publishes.  Here ~process hands the extracted PointXYZRGBNormal rows (the cloud it is about to
 * save, in the fusion frame) to whoever registered; the ROS adapter (host/ros_shell.cpp) publishes them on that topic.
 * The rows are only valid during the call. */
typedef void (*hfpf_publish_fn)(void* user, const hfpf_row* rows, uint64_t n_rows, const char* frame_id);
int hfpf_node_set_publisher(hfpf_node* n, hfpf_publish_fn fn, void* user);

/* EXTENSION: with mesh output set, ~process also writes <directory_name>/mesh.ply: hfpf_extract_mesh of the model it saves, with
 * these options, through hfpf_write_ply (before the grid is cleared).  NULL turns it off again, the default.  Invalid options are
 * refused with HFPF_ERR_BAD_ARG and leave the setting as it was.  (hfpf_node_params keeps its size: it is part of the ABI.) */
int hfpf_node_set_mesh_output(hfpf_node* n, const hfpf_mesh_opts* opts);

/* EXTENSION: profiles of the saved mesh.  With section planes set and mesh output set, ~process also cuts the mesh it writes to
 * mesh.ply (hfpf_section_mesh of include/hfpf.h: that mesh, identity pose, these planes) and writes, beside it, sections.csv (header
 * plane,contour,tri,x0,y0,z0,x1,y1,z1, then one line per segment in (plane, triangle) order: its plane, contour and triangle and the
 * x, y, z of its two points p0 and p1, floats as %.9g) and section_summary.csv (header plane,first_segment,n_segments,first_point,
 * n_points,first_contour,n_contours,n_closed,n_branched,length_q32,area_q28, then one line per plane with its hfpf_section_plane).
 * planes holds n_planes * 4 f64 (n.x, n.y, n.z, d) in the fusion frame; the node keeps a copy.  With section planes set and mesh
 * output NOT set, ~process returns HFPF_ERR_STATE with success=false before it writes anything, and keeps the grid: set the mesh
 * output (or drop the planes) and call it again.  NULL opts turns it off again, the default: neither file is then written.  Invalid
 * options (hfpf_check_section_opts), more than 4096 planes, NULL planes with n_planes > 0 and a plane with a non-finite value or a
 * normal of no finite length > 0 are refused with HFPF_ERR_BAD_ARG and leave the setting as it was. */
int hfpf_node_set_section_planes(hfpf_node* n, const hfpf_section_opts* opts, const double* planes, uint32_t n_planes);

/* EXTENSION: open edges of the saved mesh.  With mesh topology set and mesh output set, ~process also runs hfpf_mesh_topology_device
 * (include/hfpf.h) on the mesh it writes to mesh.ply, read in HBM where hfpf_extract_mesh_device leaves it with the same options,
 * identity pose, and writes beside it: mesh_edges.csv (header p0,p1,tri,kind,uses,loop,shell, then one line per edge that is not
 * interior, in the call's order), mesh_loops.csv (header loop,first_vertex,n_verts,n_edges,n_ends,flags,shell,length_q32,area_q28_x,
 * area_q28_y,area_q28_z), mesh_shells.csv (header shell,first_vertex,n_verts,n_tris,flags,n_edges,n_boundary,n_nonmanifold,n_miswound,
 * n_loops,area_q32,volume_q40) and mesh_topology_summary.csv (header n_tris_valid,n_tris_invalid,n_tris_far,n_verts_used,n_edges,
 * n_interior,n_boundary,n_nonmanifold,n_miswound,n_loops,n_closed_loops,n_shells,n_watertight, then one line); every value is an
 * integer.  With mesh topology set and mesh output NOT set, ~process returns HFPF_ERR_STATE with success=false before it writes
 * anything, and keeps the grid, exactly as with section planes.  NULL opts turns it off again, the default: none of the four files
 * is then written.  Invalid options (hfpf_check_topology_opts) are refused with HFPF_ERR_BAD_ARG and leave the setting as it was. */
int hfpf_node_set_mesh_topology(hfpf_node* n, const hfpf_topology_opts* opts);

/* EXTENSION: with a component filter set, ~process saves the model without its specks: test_cloud.pcd and meta.csv (and the
 * published cloud) hold the rows hfpf_extract_components keeps with these options instead of every row.  mesh.ply and the
 * write_variants files are not filtered, unless hidden with hfpf_hide_voxels (hfpf_node_set_hide_filtered below does that for the
 * rows this filter drops).  NULL turns it off again, the default: the files are then byte-identical to those of a node
 * that never called this.  Invalid options (hfpf_check_component_opts) are refused with HFPF_ERR_BAD_ARG and leave the setting as it
 * was. */
int hfpf_node_set_component_filter(hfpf_node* n, const hfpf_component_opts* opts);

/* EXTENSION: make every file leave out what the component filter drops.  With this on (default off) and a component filter set,
 * ~process first runs the filter in HBM (hfpf_extract_components_device) and hides the rows it drops (hfpf_hide_voxels_device of
 * include/hfpf.h: HFPF_HIDE_OTHERS on the kept rows, stride 64, read in place), then goes on as a node without a component filter.
 * test_cloud.pcd and meta.csv are then byte-identical to those of the filter alone; mesh.ply, the write_variants files,
 * deviation*.csv, coverage*.csv, alignment.csv and consistency*.csv are those of the direct calls on a handle with the same rows hidden
 * (their own min_count options apply again: the filter's no longer replaces them).  ~process clears the grid at its end as before,
 * which empties the hidden set.  With it off, or without a component filter, every file is byte-identical to that of a node that
 * never called this. */
int hfpf_node_set_hide_filtered(hfpf_node* n, int on);

/* EXTENSION: the operator's "erase this" (HFPF_HIDE), "bring it back" (HFPF_SHOW) or "crop to this" (HFPF_HIDE_OTHERS) during a scan:
 * hfpf_hide_box of include/hfpf.h on the node's grid for a box in fusion-frame metres, box_m = xmin,xmax,ymin,ymax,zmin,zmax.  Each
 * bound becomes an inclusive voxel index with the voxel = floor((p - bbox_min) / res) of the query contract (saturated to the int32
 * range; a NaN bound is refused with HFPF_ERR_BAD_ARG).  It runs under the grid's own lock, like save and load: a frame or a clean
 * pass lands wholly before or wholly after it.  Rows that appear later are visible; ~process (its hfpf_clear) empties the set, ~reset does not touch the grid.
 * res may be NULL.  Errors as hfpf_hide_box. */
int hfpf_node_hide_box(hfpf_node* n, uint32_t op, const double box_m[6], hfpf_hide_result* res);

/* EXTENSION: with a reference mesh set, ~process also measures the saved cloud against it (hfpf_compare_mesh of include/hfpf.h) and
 * writes, beside test_cloud.pcd, deviation.csv (header ix,iy,iz,signed_distance,distance,tri,flags, then one line per row of the saved
 * cloud, floats as %.9g) and deviation_summary.csv (one header line, one value line: n_rows, n_found, n_negative, n_tris_valid,
 * n_tris_invalid, max_abs, sum_abs_q30, sum_sq_q30).  The mesh (arguments as hfpf_compare_mesh's, host memory) and the pose are
 * copied.  With a component filter set the lines are those of the kept rows: the compare runs on the full row set with the filter's
 * min_count (opts->min_count is then ignored), the kept rows' records are selected and the row part of the summary is rebuilt from
 * them.  NULL opts turns it off again, the default.  Invalid arguments are refused with HFPF_ERR_BAD_ARG and leave the setting as it
 * was; max_distance against the grid's resolution is checked by ~process, which then fails as hfpf_compare_mesh does. */
int hfpf_node_set_reference_mesh(hfpf_node* n, const hfpf_deviation_opts* opts, const void* verts, uint64_t n_verts, uint32_t vertex_stride,
                                 const uint32_t* tris, uint64_t n_tris, const double* pose_3x4);

/* EXTENSION: best-fit, then compare.  With alignment options set and a reference mesh set, ~process first refines the reference
 * mesh's pose against the model (hfpf_align_mesh of include/hfpf.h, started from the pose given to hfpf_node_set_reference_mesh; with a
 * component filter set, opts->compare.min_count is replaced by the filter's, as the compare's is) and writes deviation.csv and
 * deviation_summary.csv at the refined pose.  It also writes alignment.csv: the header
 * iterations,flags,rows_sampled,inliers,rms,p0,...,p11 and one value line, rms and the 12 pose values (row-major [R|t]) as %.17g, so
 * that the pose reads back bit for bit.  The stored pose of the reference mesh is not changed: every ~process starts from it again.
 * Without a reference mesh the setting has no effect.  NULL turns it off again, the default: the files are then those of a node that
 * never called this, and no alignment.csv is written.  Invalid options (hfpf_check_align_opts) are refused with HFPF_ERR_BAD_ARG and
 * leave the setting as it was. */
int hfpf_node_set_reference_alignment(hfpf_node* n, const hfpf_align_opts* opts);

/* EXTENSION: which parts of the reference mesh were scanned.  With coverage options set and a reference mesh set, ~process also runs
 * hfpf_cover_mesh of include/hfpf.h on that mesh, at the pose the deviation files are written at (the refined pose when alignment is
 * on; with a component filter set, opts->min_count is replaced by the filter's, as the compare's is), and writes coverage.csv (header
 * tri,n_samples,n_in_bbox,n_covered,flags,area,max_distance,sum_dist_q30, then one line per triangle of the mesh, floats as %.9g) and
 * coverage_summary.csv (one header line, one value line: n_tris_valid, n_tris_invalid, n_tris_huge, n_samples, n_in_bbox, n_covered,
 * sum_dist_q30, area_q40_lo, area_q40_hi, covered_q40_lo, covered_q40_hi, max_distance).  Without a reference mesh the setting has no
 * effect.  NULL turns it off again, the default: neither file is then written.  Invalid options (hfpf_check_cover_opts) are refused
 * with HFPF_ERR_BAD_ARG and leave the setting as it was. */
int hfpf_node_set_reference_coverage(hfpf_node* n, const hfpf_cover_opts* opts);

/* EXTENSION: from where to scan what is still missing.  With candidate views set and a reference mesh set, ~process also runs
 * hfpf_plan_views of include/hfpf.h on that mesh, at the pose the deviation files are written at (the refined pose when alignment is
 * on; with a component filter set, opts->cover.min_count is replaced by the filter's, as the coverage's is), and writes view_plan.csv
 * (header view,rank,n_in_view,n_facing,n_visible,visible_q40,gain_q40,gain_samples, then one line per candidate view) and
 * view_plan_summary.csv (one header line, one value line: n_views, n_selected, n_targets, n_reachable, n_planned, target_q40,
 * reachable_q40, planned_q40, and of the embedded coverage summary n_samples, n_in_bbox, n_covered).  poses holds n_views * 12 f64,
 * row-major [R|t], camera -> fusion frame; the node keeps a copy.  Without a reference mesh the setting has no effect.  A NULL opts
 * turns it off again, the default: neither file is then written.  Invalid options (hfpf_check_plan_opts), more than 4096 views and
 * NULL or non-finite poses are refused with HFPF_ERR_BAD_ARG and leave the setting as it was. */
int hfpf_node_set_view_candidates(hfpf_node* n, const hfpf_plan_opts* opts, const double* poses, uint32_t n_views);

/* EXTENSION: what the last depth images say about every saved row.  With consistency options set the node keeps host copies of the
 * last keep_frames (1..4096) depth images hfpf_node_on_depth_image integrated, with their poses; an image whose hfpf_depth_image
 * differs from the ring's empties the ring first.  ~process then also runs hfpf_depth_consistency of include/hfpf.h on those images
 * (frame index = position in the ring, oldest first; no frames: all-zero records) and writes, beside test_cloud.pcd, consistency.csv
 * (header ix,iy,iz,n_in_view,n_tested,n_support,n_through,n_occluded,first_through,flags, then one line per row of the saved cloud)
 * and consistency_summary.csv (one header line, one value line: n_rows, n_seen, n_supported, n_contradicted, n_kept, pairs_tested,
 * pairs_support, pairs_through).  It is a report: HFPF_CONSISTENCY_DROP in opts->flags is ignored, and the saved cloud and the mesh
 * are not filtered by it.  With a component filter set the lines are those of the kept rows: the call runs on the full row set with
 * the filter's min_count (opts->min_count is then ignored), the kept rows' records are selected and the summary is rebuilt from
 * them.  ~reset, hfpf_node_load_session and a ~process that saved its cloud empty the ring.  Clouds (hfpf_node_on_point_cloud) are
 * not kept.  NULL opts turns it off again, the default, and drops the ring: the files are then byte-identical to those of a node
 * that never called this.  Invalid options (hfpf_check_consistency_opts) or a keep_frames outside 1..4096 are refused with
 * HFPF_ERR_BAD_ARG and leave the setting as it was. */
int hfpf_node_set_depth_consistency(hfpf_node* n, const hfpf_consistency_opts* opts, uint32_t keep_frames);

/* EXTENSION: keep the grid's session in a file and take it up again (hfpf_save / hfpf_load of include/hfpf.h on the node's grid, with
 * their errors).  Both run under the grid's own lock, so they are legal while the cloud callback and the clean thread run: a frame
 * or a clean pass lands wholly before or wholly after them.  Loading replaces the fused data only: the node stays started or stopped
 * as it was, its counters go on, and the node's grid must match the file as hfpf_restore says (same grid configuration and
 * max_log_points, pools that hold the session). */
int hfpf_node_save_session(hfpf_node* n, const char* path);
int hfpf_node_load_session(hfpf_node* n, const char* path);

/* One iteration of cleanGrid (node.cpp:301-325): clean iff state_changed.  Returns 1 if a pass ran. */
int hfpf_node_clean_now(hfpf_node* n);
hfpf_handle* hfpf_node_grid(hfpf_node* n);

typedef struct hfpf_node_stats {
    uint64_t received, integrated, dropped_not_started, dropped_tf, clean_passes, process_calls;
    int32_t started, cloud_subscription_started;
} hfpf_node_stats;
int hfpf_node_get_stats(hfpf_node* n, hfpf_node_stats* out);

#ifdef __cplusplus
}
#endif
#endif
