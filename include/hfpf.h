/* include/hfpf.h -- C ABI of the MI355X-native occupancy-grid point-cloud fusion engine (libhfpf.so).
 *
 * This is the drop-in boundary for the reference's `class OccupancyGrid`
 * (pointcloud_fusion/pointcloud_fusion/include/utilities/OccupancyGrid.hpp:99-136, "grid.hpp" below),
 * which the reference node owns by value as `PointcloudFusion::grid_`
 * (pointcloud_fusion/pointcloud_fusion/src/pointcloud_fusion_and_filter.cpp:132, "node.cpp" below).
 * The reference has no FFI layer of its own; each entry point cites the member function / call site
 * it replaces.  Plain pointers and sizes only; no C++ or torch types cross this boundary; nothing
 * throws across it.  All functions return an hfpf_status (0 = ok, negative = error) unless noted,
 * and may be called from any thread (the handle serialises mutating calls internally; the reference
 * serialises with grid_mtx_, node.cpp:142,291,305).
 *
 * The engine has no CPU fallback: every entry point that computes runs HIP kernels on the
 * configured device and fails with HFPF_ERR_HIP when no device is usable.
 */
#ifndef HFPF_H
#define HFPF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HFPF_ABI_VERSION 6

/* hfpf_config.flags */
#define HFPF_FLAG_FUSE_COLOR 1u /* EXTENSION: also average the member points' RGB per voxel (reference: never, grid.hpp:471-479) */
#define HFPF_FLAG_DIRECT_UPDATE 4u /* dependant updates with one memory-side atomic per (point, dependant) pair.  Default (flag
                                      clear) is the two-pass form: points are binned per 8x8x8 brick, one workgroup per brick
                                      accumulates its statistic records in LDS and flushes each once per launch.  Same results
                                      either way (the sums are integers); the binned form is ~1.5x faster on the bench. */
#define HFPF_FLAG_PCL_SHIFTED_COV 2u /* plane fit with pcl::computeMeanAndCovarianceMatrix as PCL >= 1.11 computes it (moments of
                                        p - first point).  Default (0) is the single-pass form of PCL <= 1.10; the two differ
                                        visibly in f32 ~1 m from the origin (call site grid.hpp:302) */

typedef struct hfpf_handle hfpf_handle;

typedef enum hfpf_status {
    HFPF_OK = 0,
    HFPF_ERR_BAD_CONFIG = -1, /* bbox max<=min, resolution<=0, k!=2, K out of range ... */
    HFPF_ERR_BAD_ARG = -2,
    HFPF_ERR_CAPACITY = -3, /* a device pool (bricks, point log, normals, registrations) overflowed */
    HFPF_ERR_HIP = -4,      /* HIP runtime error; see hfpf_last_error */
    HFPF_ERR_STATE = -5,
    HFPF_ERR_IO = -6,
    HFPF_ERR_DIST = -7 /* RCCL / rank bootstrap error */
} hfpf_status;

/* Replaces setResolution/setDimensions/setK/construct (grid.hpp:614,604,138,621; called once from
 * the node ctor, node.cpp:161-164) plus the compile-time constants of the capture stage.
 * Defaults (hfpf_default_config) are the reference's values. */
typedef struct hfpf_config {
    uint32_t struct_size;     /* = sizeof(hfpf_config) */
    float resolution;         /* voxel edge, metres, AS FLOAT: the reference stores a float into a double
                                 member (grid.hpp:614-619), so 0.005f -> 0.004999999888241291. node.cpp:91 */
    double bbox[6];           /* xmin,xmax,ymin,ymax,zmin,zmax; launch param `bounding_box` (node.cpp:451,162) */
    int32_t k;                /* occupancy stencil half-width; must be 2 (grid.hpp:334 hard-codes 125 probes) */
    int32_t K;                /* line half-length in voxel steps (template arg, node.cpp:311,317) = 3 */
    int32_t gate;             /* a voxel gets a normal when occupied neighbours > gate (grid.hpp:352) = 20.  The count includes the
                                 voxel itself and only cells of the 5 x 5 x 5 stencil inside the grid.  Any value is accepted.  Below 2
                                 the gate also passes voxels with one or two such cells: no plane fits fewer than three points
                                 (grid.hpp:301), and their rows keep a zero normal (see hfpf_row).  At 2 to 4 every stencil that passes
                                 can still be collinear, and a collinear stencil gives a NaN normal */
    double cylinder_radius;   /* kCylinderRadius, grid.hpp:36 = 0.001 */
    double ball_radius;       /* kBballRadius, grid.hpp:35 = 0.015 */
    double z_clip_min;        /* kZmin, node.cpp:92 = 0.28 (camera frame, strict) */
    double z_clip_max;        /* kZmax, node.cpp:93 = 0.6 */
    int32_t device;           /* HIP device ordinal */
    uint32_t flags;           /* HFPF_FLAG_*; 0 = the reference's behaviour */
    /* Device pool capacities; 0 = engine default.  The reference grows without bound (README:12). */
    uint64_t max_bricks;      /* 8x8x8-voxel bricks that may be touched */
    uint64_t max_log_points;  /* points buffered while their voxel has no normal (grid.hpp:211,230) */
    uint64_t max_normals;     /* voxels that may receive a normal */
    uint64_t max_frames;      /* frame ids (viewpoint table) */
    /* Scheduling hint, no reference counterpart: pixels per image row when every frame is a row-major organised image
       (sensor_msgs/PointCloud2 width of an organised cloud, or the sensor's width for clouds republished as height=1);
       0 = unknown.  The integrate kernel then walks a frame in 16x16-pixel patches instead of 256-point runs, which
       touches about half as many voxel-table lines per point.  Used only when width and rows are multiples of 16 and
       n_points is a multiple of width; results never depend on it. */
    uint32_t frame_width;
    uint32_t reserved0;       /* 0 */
    /* Largest n_points * n_frames one hfpf_integrate_device call will carry; sizes the per-call brick bins at create like
       the other pools.  0 = grown on demand (the first call of a new size then pays for the allocation). */
    uint64_t max_call_points;
} hfpf_config;

/* One emitted voxel = one line of test_cloud.pcd + one line of meta.csv (grid.hpp:466-480). 64 bytes.
 *
 * THE NORMAL is the reference's plane fit of the occupied stencil cells' centres (single-pass f32 covariance, pcl::eigen33), turned
 * towards the viewpoint of the voxel's first frame.  It is a unit vector but for two cases, which are the reference's arithmetic and
 * are reproduced, not repaired:
 *   NaN in all three components: the cross products of the eigen-solve are all exactly zero and the normal is 0/0.  That happens
 *     when the covariance has rank one (every collinear stencil, at any gate that lets one pass) and when the f32 covariance of a flat
 *     stencil cancels far from the origin (a surface along the grid at 100 m and more, where the coordinates' squares eat the f32
 *     mantissa; HFPF_FLAG_PCL_SHIFTED_COV takes the moments about the first point and has none of these).  Neighbours of such a
 *     voxel may carry normals that are rounding noise: unit vectors, deterministic, unrelated to the surface.
 *   zero in all three components: fewer than three stencil cells were valid and occupied, so there was no fit (gate below 2 only).
 * Either row has count == 0, x = y = z = 0 and zero statistics: no point lies within a cylinder about a NaN or zero-length line,
 * and the voxel registers in no other cell (NaN) or in its own cell alone (zero).  Sign and payload of the NaN are unspecified;
 * compare by isnan.  Every read-out that takes rows by count >= max(1, min_count) (render, track, query and what is built on it:
 * mesh, raycast, cover) never sees such a row; extract, extract_filtered and components at min_count 0, compare_mesh, depth_consistency,
 * hide and snapshot carry it.  A NaN normal fails every gate on a normal (components' min_normal_dot, depth_consistency's min_cos: a NaN
 * compares false); a zero normal has the dot product 0 with everything. */
typedef struct hfpf_row {
    int32_t ix, iy, iz;  /* voxel index triplet */
    uint32_t count;      /* points in cylinder (VoxelInfo::count) */
    float x, y, z;       /* cylinder-filtered mean of projected points (VoxelInfo::centroid); (0,0,0) when count==0 */
    float nx, ny, nz;    /* VoxelInfo::normal: a unit vector, or NaN NaN NaN, or 0 0 0 (above); the latter two only with count == 0 */
    float sdx, sdy, sdz; /* VoxelInfo::sd (population variance per axis, as the reference's Welford recurrence) */
    float mean_dist;     /* VoxelInfo::mean_dist */
    float sd_dist;       /* VoxelInfo::sd_dist */
    uint32_t rgb;        /* 0 (the reference never writes rgb); with HFPF_FLAG_FUSE_COLOR: mean colour of the cylinder members, 0x00RRGGBB */
} hfpf_row;

typedef struct hfpf_counters {
    uint64_t points_presented;  /* input points seen by integrate (before any clip) */
    uint64_t points_zclip_pass; /* survived the camera-frame z-clip */
    uint64_t points_in_bbox;    /* survived the bbox clip (= voxel touches) */
    uint64_t points_buffered;   /* appended to the point log */
    uint64_t dep_pairs_tested;  /* (point, dependant) cylinder tests in integrate */
    uint64_t dep_pairs_member;  /* ... that were inside the cylinder */
    uint64_t voxels_occupied;
    uint64_t voxels_with_normal;
    uint64_t bricks_allocated;
    uint64_t registrations;     /* dependant registrations on occupied cells (grid.hpp:417) */
    uint64_t dep_entries;       /* entries in the current dependant table */
    uint64_t frames_integrated;
    uint64_t clean_passes;
    uint64_t device_bytes;      /* HBM allocated by this handle */
    uint64_t replay_members;    /* buffered points found inside a cylinder when replayed by a clean pass (grid.hpp:418-440) */
    uint64_t points_direct;     /* of points_buffered: appended one by one through the overflow list (no bin region or a full one), outside the bricks' runs */
    uint64_t table_misses;      /* work items of the dependant update that found no slot in the LDS record table (updated HBM directly) */
    uint64_t update_extra_rounds; /* (ABI 5) sort rounds beyond the first that bricks of the dependant update / streaming replay took (a brick with more parked points than one LDS round holds) */
} hfpf_counters;

void hfpf_default_config(hfpf_config* cfg);
int hfpf_abi_version(void);

/* OccupancyGrid(), setResolution, setDimensions, setK, construct  (grid.hpp:111,614,604,138,621).
 * SIZE LIMITS (HFPF_ERR_BAD_CONFIG, before anything is allocated): with dim[a] = (int)((max[a] - min[a]) / (double)resolution),
 *   (max[a] - min[a]) / (double)resolution < 2097151 on every axis: at most 2,097,150 cells, so that a cell index 0..dim fits a
 *     21-bit key field (an all-ones field is kept as the sentinel);
 *   the brick directory, one 32-bit word per 8 x 8 x 8 cells of the dim + 1 storage cells an axis, has at most 4.0e9 entries
 *     ((dim[0] + 8) / 8 * ((dim[1] + 8) / 8) * ((dim[2] + 8) / 8), integer divisions): its linear index is 32-bit.
 * Both limits are reached by tests/test_gpu_deep.py: the hot path and every read-out run at 2,097,150 cells an axis and at
 * 1579^3 = 3.94e9 directory entries (16 GB of device memory for the directory alone). */
int hfpf_create(const hfpf_config* cfg, hfpf_handle** out);
/* The reference never destroys its grid (no destructor; leaks). */
int hfpf_destroy(hfpf_handle* h);
/* Thread-local-free: the last error text of this handle (or of create when h == NULL). */
const char* hfpf_last_error(const hfpf_handle* h);
/* xdim,ydim,zdim as construct() truncates them (grid.hpp:623-625) and the resolution as a double. */
int hfpf_get_dims(const hfpf_handle* h, int32_t dims[3], double* resolution);

/* Integrate one frame given as PointCloud2-style records in HOST memory.
 * Replaces, in one call: pointCloud2ToPclXYZRGBOMP (node.cpp:182-216), the z-clip (node.cpp:251-255),
 * pcl::transformPointCloud (node.cpp:289), the viewpoint (node.cpp:290) and
 * OccupancyGrid::addPoints<N> (grid.hpp:185-280; call sites node.cpp:293,295).
 *   base        first record; n_points records of point_step bytes.  The caller applies the
 *               reference's first-row rule, i.e. n_points = row_step / point_step (node.cpp:185,190).
 *   off_*       byte offsets of the f32 fields x,y,z,rgb inside a record (fields[0..3].offset).
 *   pose_3x4    fusion_frame <- camera, row-major 3x4 f64 (the Affine3d of node.cpp:338).
 * The buffer is copied before the call returns.  Frame ids count up from 0 per handle.
 * The frame's kernels are launched at once when the engine's stream is idle; while it is busy with earlier frames the frame
 * waits (already uploading) and is launched together with the frames behind it, at most HFPF_HOST_BATCH (default 4) per launch.
 * Any other call on the handle launches what is waiting first; an error of a deferred launch is returned by that call.
 * Deferred errors: HFPF_OK means "accepted".  A pool that overflows on the device while the frame's kernels run (HFPF_ERR_CAPACITY)
 * is noticed at the handle's next counter read-back -- hfpf_clean, hfpf_extract, hfpf_sync, hfpf_get_counters -- and returned by
 * that call; the handle then refuses work (HFPF_ERR_STATE) until hfpf_clear.  Frames accepted after the failure and not yet
 * launched are dropped, and the call that finds them waiting says so with HFPF_ERR_STATE. */
int hfpf_integrate(hfpf_handle* h, const void* base, uint32_t n_points, uint32_t point_step, uint32_t off_x,
                   uint32_t off_y, uint32_t off_z, uint32_t off_rgb, const double pose_3x4[12]);

/* The same for a frame in PAGE-LOCKED host memory (hfpf_host_alloc below, or hipHostRegister by the caller): no bounce copy; the
 * upload runs on the engine's copy stream and overlaps the kernels of earlier frames, the call returns at once.  The buffer must
 * stay untouched until the next hfpf_sync / hfpf_clean / hfpf_extract of this handle (all of which wait for queued work).
 * hfpf_integrate itself uploads the same way after copying the caller's buffer into pinned staging. */
int hfpf_integrate_pinned(hfpf_handle* h, const void* pinned_base, uint32_t n_points, uint32_t point_step, uint32_t off_x,
                          uint32_t off_y, uint32_t off_z, uint32_t off_rgb, const double pose_3x4[12]);
int hfpf_host_alloc(hfpf_handle* h, uint64_t bytes, void** host_ptr); /* page-locked host memory */
int hfpf_host_free(hfpf_handle* h, void* host_ptr);

/* Same path for frames already resident in HBM: n_frames frames, frame f at dev_base + f*frame_stride,
 * poses = n_frames*12 f64 in HOST memory, frame_ids = n_frames ids in HOST memory or NULL (auto).
 * One launch covers the whole batch; asynchronous on the engine's stream. */
int hfpf_integrate_device(hfpf_handle* h, const void* dev_base, uint32_t n_frames, uint64_t frame_stride,
                          uint32_t n_points, uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z,
                          uint32_t off_rgb, const double* poses, const uint32_t* frame_ids);

/* ---- registered depth + colour images (the sensor's own output instead of a PointCloud2) ----------------------------------
 * A depth frame is DEFINED as the organised cloud this f32 arithmetic makes of it (modelled on depth_image_proc's convertDepth /
 * point_cloud_xyzrgb); that cloud is then fused exactly as hfpf_integrate fuses a cloud, so rows and counters are byte-identical
 * to those of the equivalent packed cloud (x, y, z, rgb; 16 bytes) through hfpf_integrate.  Per frame, on the host:
 * cxf = (float)cx, cyf = (float)cy, and
 *   HFPF_DEPTH_U16 (16UC1): unit = depth_scale (metres per count), sx = (float)((double)unit / fx), sy = (float)((double)unit / fy);
 *                           pixel (u, v) with count d is valid iff d != 0;
 *                           x = (((float)u - cxf) * (float)d) * sx, y = (((float)v - cyf) * (float)d) * sy, z = (float)d * unit
 *   HFPF_DEPTH_F32 (32FC1, metres): sx = (float)(1.0 / fx), sy = (float)(1.0 / fy); valid iff isfinite(d);
 *                           x = (((float)u - cxf) * d) * sx, y likewise, z = d
 * Every operation f32, left to right, never contracted.  An invalid pixel becomes x = y = z = NaN: it counts in points_presented
 * and fails the z-clip, as a NaN record of a cloud does.  Colour (same width x height as the depth image) becomes
 * rgb = r << 16 | g << 8 | b, alpha dropped (what the reference's decode makes of an rgb field, node.cpp:170-216); HFPF_COLOR_NONE
 * gives rgb = 0.  Points are in row-major order, i = v * width + u; viewpoint and frame ids behave as for a cloud.  Lens
 * distortion is not modelled.  hfpf_config.frame_width is ignored: a depth frame carries its own width (16x16-pixel tiles when
 * width and height are multiples of 16). */
#define HFPF_DEPTH_U16 1 /* sensor_msgs/Image "16UC1" / "mono16": uint16 counts of depth_scale metres, 0 = no reading */
#define HFPF_DEPTH_F32 2 /* "32FC1": f32 metres, non-finite = no reading */
#define HFPF_COLOR_NONE 0
#define HFPF_COLOR_RGB8 1  /* "rgb8" */
#define HFPF_COLOR_BGR8 2  /* "bgr8" */
#define HFPF_COLOR_RGBA8 3 /* "rgba8" */
#define HFPF_COLOR_BGRA8 4 /* "bgra8" */

/* One frame's (or a batch's) image geometry, formats and pinhole intrinsics (sensor_msgs/CameraInfo K: fx = K[0], fy = K[4],
 * cx = K[2], cy = K[5]).  Rejected with HFPF_ERR_BAD_ARG (the handle stays usable): struct_size != sizeof, reserved != 0,
 * width * height = 0 or above 2^31, an unknown format, depth_step below width * sample size or not a multiple of the sample
 * size (2 / 4 bytes), color_step below width * bytes per pixel (3 / 4) or, for the 4-byte formats, not a multiple of 4,
 * fx / fy not finite and positive, cx / cy not finite, depth_scale not finite and positive (U16 only; F32 ignores it),
 * a NULL depth image, a colour image with HFPF_COLOR_NONE or none with another format.  An image occupies
 * (height - 1) * step + width * bytes per pixel bytes; nothing behind that is read. */
typedef struct hfpf_depth_image {
    uint32_t struct_size;  /* = sizeof(hfpf_depth_image) */
    uint32_t width, height;
    uint32_t depth_format; /* HFPF_DEPTH_* */
    uint32_t depth_step;   /* bytes per depth image row (sensor_msgs/Image step) */
    float depth_scale;     /* metres per count of HFPF_DEPTH_U16 (0.001f for most sensors) */
    double fx, fy, cx, cy;
    uint32_t color_format; /* HFPF_COLOR_* */
    uint32_t color_step;   /* bytes per colour image row (ignored with HFPF_COLOR_NONE) */
    uint64_t reserved;     /* 0 */
} hfpf_depth_image;

/* hfpf_integrate for one depth frame (+ its registered colour image, or NULL with HFPF_COLOR_NONE) in pageable HOST memory:
 * both images are copied into the pinned staging before the call returns; the upload, batching (HFPF_HOST_BATCH), deferred
 * errors and the refusal of work after a failure are those of hfpf_integrate.  A depth frame takes ~5 bytes per pixel over
 * the link instead of the 16-32 of a cloud.  Cloud and depth frames may be interleaved freely on one handle; a batch of waiting
 * frames holds frames of one kind, size, format and intrinsics only. */
int hfpf_integrate_depth(hfpf_handle* h, const hfpf_depth_image* desc, const void* depth, const void* color, const double pose_3x4[12]);
/* ... from PAGE-LOCKED host memory; both buffers must stay untouched as hfpf_integrate_pinned says. */
int hfpf_integrate_depth_pinned(hfpf_handle* h, const hfpf_depth_image* desc, const void* depth, const void* color, const double pose_3x4[12]);
/* ... for n_frames depth frames resident in HBM: frame f's depth image at dev_depth + f * depth_frame_stride, its colour image at
 * dev_color + f * color_frame_stride (dev_color NULL with HFPF_COLOR_NONE).  Device pointers and strides must be multiples of the
 * sample size (depth 2 / 4, colour 4 for the 4-byte formats).  poses and frame_ids as hfpf_integrate_device (frame_ids NULL =
 * auto; global ids for the multi-GPU schedule).  One launch covers the batch; asynchronous on the engine's stream. */
int hfpf_integrate_depth_device(hfpf_handle* h, const hfpf_depth_image* desc, const void* dev_depth, uint64_t depth_frame_stride,
                                const void* dev_color, uint64_t color_frame_stride, uint32_t n_frames, const double* poses,
                                const uint32_t* frame_ids);

/* OccupancyGrid::state_changed (grid.hpp:110; read at node.cpp:306). Returns 0/1, or a negative status. */
int hfpf_is_dirty(hfpf_handle* h);
/* OccupancyGrid::updateThicknessVectors<N,K> (grid.hpp:311-454; call sites node.cpp:311,317).
 * The result is that of the reference walking its candidates in canonical ascending (x,y,z) order: "the last registrant wins" on
 * an unoccupied cell (grid.hpp:443-449) goes to the candidate with the largest (x,y,z) key of the pass.  The records themselves
 * are numbered in Z-order of their cells inside a pass (neighbouring records = neighbouring cells); DESIGN.md section 3.
 * Deferred errors: a SMALL pass (fewer than 2^21 / (2K+1) candidate cells) is enqueued to its end and HFPF_OK returned without
 * waiting for it; a pool that overflows inside such a pass (HFPF_ERR_CAPACITY: normal records, registrations, dependant table)
 * is returned by the next call that reads the counters back (this one included, on its next invocation), and the handle then
 * refuses work until hfpf_clear.  Integrate calls enqueued in between run on the tables as the failed pass left them; their
 * results are discarded with the handle's state at hfpf_clear.  HFPF_CLEAN_NOWAIT=0 makes every pass wait and report itself.
 * A pass that directly follows an integrate call of four or more frames starts from counters published before that call's
 * update kernel has finished (its front half runs beside it; HFPF_CLEAN_OVERLAP=0 switches that off): an error that kernel
 * raises is deferred in the same way. */
int hfpf_clean(hfpf_handle* h);

/* OccupancyGrid::downloadData (grid.hpp:456-488; call site node.cpp:398) split in two: the ordered
 * extract (rows in lexicographic x,y,z order, engine-owned buffer) and the two file writers. */
int hfpf_extract(hfpf_handle* h, hfpf_row** rows, uint64_t* n_rows);
void hfpf_free_rows(hfpf_row* rows);
/* The alternate extractors the reference keeps behind `#if 0` (node.cpp:399-437) as options of the same device-side scan:
 *   downloadHQ(cloud, threshold)   grid.hpp:546-575   min_count = threshold (rows with count < threshold are dropped ON THE
 *                                                      DEVICE, before the sort's compaction: they never reach the host), paint_white = 1
 *   downloadClassified(cloud)      grid.hpp:512-544   classify_threshold = kGoodPointsThreshold = 100 (grid.hpp:34): count > 100
 *                                                      -> red (g = b = 0), else white
 *   download(XYZRGB / XYZRGBNormal) grid.hpp:491-510,577-601  all defaults (rgb stays 0 as a default-constructed PCL point)
 * Row order is the same lexicographic (x,y,z) order.  opts == NULL is hfpf_extract. */
typedef struct hfpf_extract_opts {
    uint32_t struct_size;       /* = sizeof(hfpf_extract_opts) */
    int32_t classify_threshold; /* < 0: off */
    double min_count;           /* 0: keep all */
    int32_t paint_white;        /* 1: rgb = 0x00FFFFFF */
    int32_t reserved0;
} hfpf_extract_opts;
int hfpf_extract_filtered(hfpf_handle* h, const hfpf_extract_opts* opts, hfpf_row** rows, uint64_t* n_rows);
/* ---- rendering the fused model from a camera (the inverse of depth integration; no reference counterpart) -------------------
 * A render draws exactly the rows hfpf_extract would return at that point of the call sequence (host frames still waiting for
 * their launch are launched first, as extract does), splatted into a pinhole image.  pose_3x4 follows the integrate convention:
 * row-major [R|t], camera -> fusion frame.  All arithmetic is f64, left to right, never contracted.  For a row with f32 (x, y, z)
 * and normal (nx, ny, nz), T = pose_3x4:
 *   dx = (double)x - T[3], dy = (double)y - T[7], dz = (double)z - T[11]
 *   xc = (T[0]*dx + T[4]*dy) + T[8]*dz,  yc = (T[1]*dx + T[5]*dy) + T[9]*dz,  zc = (T[2]*dx + T[6]*dy) + T[10]*dz
 *   the row is drawn iff count >= max(1, min_count) (the compare of hfpf_extract_opts), z_near < zc < z_far and, with
 *   HFPF_RENDER_CULL_BACKFACES, ((nx*dx + ny*dy) + nz*dz) < 0 (nx.. widened to double)
 *   u = (xc / zc) * fx + cx,  v = (yc / zc) * fy + cy;  skipped unless |u| < 2^30 and |v| < 2^30
 *   pu = floor(u + 0.5), pv = floor(v + 0.5)   (the pixel whose centre back-projects onto the row: the inverse of a depth frame)
 *   r = splat_radius, or for -1: min(max_splat_radius, floor(((0.5 * res) * max(fx, fy)) / zc)), res = hfpf_get_dims' resolution
 *   candidates: every pixel (pu + i, pv + j), |i|, |j| <= r, inside [0, width) x [0, height);  depth32 = (float)zc
 * Each pixel takes the candidate with the smallest depth32; ties go to the lexicographically smallest (ix, iy, iz), so the image
 * does not depend on scheduling.  From the winner: depth = depth32; rgb, count and voxel = the row's own values; normal = the
 * row's normal in the camera frame ((T[0]*nx + T[4]*ny) + T[8]*nz, (T[1]*nx + T[5]*ny) + T[9]*nz, (T[2]*nx + T[6]*ny) + T[10]*nz,
 * each rounded to f32) or, with HFPF_RENDER_WORLD_NORMALS, as stored.  Empty pixels: depth and normal NaN (0x7FC00000), rgb and
 * count 0, voxel -1.
 * A render changes nothing on the handle: tables, counters and later results are those without it, except that device_bytes
 * counts the scratch it keeps (8 bytes per pixel per view of a chunk of at most 256 MB, plus the row set and, for hfpf_render,
 * its planes).  Rejected with HFPF_ERR_BAD_ARG (the handle stays usable): struct_size != sizeof, unknown flags, reserved != 0,
 * width * height = 0 or above 2^31, fx / fy not finite and positive, cx / cy not finite, not 0 < z_near < z_far with both
 * finite, min_count NaN, splat_radius outside -1..15, max_splat_radius outside 0..15, a NULL pose array, every plane NULL.
 * A handle with an RCCL communicator returns HFPF_ERR_STATE (a distributed render is not provided); a failed handle returns
 * HFPF_ERR_STATE as extract does.  Both calls return when the planes are complete. */
#define HFPF_RENDER_CULL_BACKFACES 1u /* skip rows whose normal faces away from the camera */
#define HFPF_RENDER_WORLD_NORMALS 2u  /* normal plane in the fusion frame (default: camera frame) */

typedef struct hfpf_render_opts {
    uint32_t struct_size;   /* = sizeof(hfpf_render_opts) */
    uint32_t width, height; /* image size; width * height in 1..2^31 */
    uint32_t flags;         /* HFPF_RENDER_* */
    double fx, fy, cx, cy;  /* pinhole intrinsics, as hfpf_depth_image */
    double z_near, z_far;   /* a row is drawn iff z_near < zc < z_far */
    double min_count;       /* rows with count < max(1, min_count) are not drawn */
    int32_t splat_radius;   /* >= 0: fixed half-width in pixels (0 = one pixel); -1: auto per row (above) */
    int32_t max_splat_radius; /* cap of the auto radius, 0..15 */
    uint64_t reserved;      /* 0 */
} hfpf_render_opts;

typedef struct hfpf_render_planes { /* every plane optional (NULL = not produced); at least one non-NULL */
    float* depth;    /* width * height: camera-frame z in metres */
    float* normal;   /* width * height * 3 */
    uint32_t* rgb;   /* width * height: the row's rgb (0x00RRGGBB) */
    uint32_t* count; /* width * height: the row's count */
    int32_t* voxel;  /* width * height * 3: the row's ix, iy, iz */
} hfpf_render_planes;

/* One view into pageable HOST planes. */
int hfpf_render(hfpf_handle* h, const hfpf_render_opts* o, const double pose_3x4[12], const hfpf_render_planes* host_out);
/* n_views views (poses = n_views * 12 f64 in HOST memory) into DEVICE planes: view v's plane starts v * width * height elements
 * (times 3 for normal and voxel) behind the plane's base.  The row set is built once for all views.  n_views = 0 does nothing. */
int hfpf_render_device(hfpf_handle* h, const hfpf_render_opts* o, uint32_t n_views, const double* poses, const hfpf_render_planes* dev_out);

/* ---- refining a frame's pose against the fused model (frame-to-model point-to-plane ICP; no reference counterpart) -----------
 * A track takes one frame (a depth image or a cloud) and a pose guess T0 (row-major [R|t], camera -> fusion frame, the integrate
 * convention) and returns a refined pose in the same convention; the caller then integrates the frame at that pose.  Let
 * c = (T0[3], T0[7], T0[11]), the input camera centre.  All host and device arithmetic is f64 unless stated, one rounding per
 * operation, left to right, never contracted.
 * Model view: the z-buffer hfpf_render would build with opts.view at T0 -- the same row set (host frames still waiting are
 *   launched first), splat and tie rule; no plane is produced.  Its word bits(depth32) << 32 | j names row j of that row set.
 * Sampling: depth pixel (u, v) iff u % stride == 0 and v % stride == 0, back-projected by the f32 arithmetic of the depth-frame
 *   contract above; cloud point i iff i % stride == 0, its f32 x, y, z.  A sampled point p is USED iff x, y, z are finite and
 *   z_clip_min < z < z_clip_max (the handle's z-clip, as integrate applies it).  At most 2^26 points may be sampled.
 * Per iteration k = 1, 2, ... with estimate T = T_{k-1}, for every used point p:
 *   pw = (((T[0]*px + T[1]*py) + T[2]*pz) + T[3], ((T[4]*px + ...) + T[7], ((T[8]*px + ...) + T[11])   (p widened, not rounded)
 *   a = pw - c; projected into the view with the splat's arithmetic at T0 (dx, dy, dz = a): kept iff z_near < zc < z_far,
 *   |u|, |v| < 2^30, (pu, pv) = (floor(u + 0.5), floor(v + 0.5)) inside the image and its word not empty (no culling test).
 *   q = (double)row j's x, y, z;  n = (double)row j's nx, ny, nz;  d = pw - q
 *   kept iff (d.x*d.x + d.y*d.y) + d.z*d.z <= max_distance * max_distance, (n.x*n.x + n.y*n.y) + n.z*n.z <= 2 and
 *   max(|a.x|, |a.y|, |a.z|) < 32 (metres: the headroom rule below)
 *   r = (n.x*d.x + n.y*d.y) + n.z*d.z
 *   J = (a.y*n.z - a.z*n.y, a.z*n.x - a.x*n.z, a.x*n.y - a.y*n.x, n.x, n.y, n.z)      (twist order omega, tau)
 *   each kept point (an INLIER) adds (int64) rint(v * s) for v = J_i*J_j (i <= j; s = 2^24), J_i*r (s = 2^28) and r*r (s = 2^32)
 *   into exact int64 sums, so the sums do not depend on scheduling.  Headroom: |J_i| < 64, |r| < 2, and 2^26 points keep every
 *   sum below 2^62.
 * On the host: A = J^T J (sums / 2^24, symmetric), b = J^T r (sums / 2^28), rr = sum / 2^32, all from the int64 sums.
 *   inliers < min_inliers: HFPF_TRACK_TOO_FEW, stop.
 *   Cholesky of M = A + damping*I (damping added to the diagonal), j = 0..5:  s = M[j][j] - L[j][0]^2 - ... - L[j][j-1]^2 (each
 *   subtracted in turn); s > 0 or HFPF_TRACK_DEGENERATE and stop; L[j][j] = sqrt(s); for i = j+1..5: L[i][j] = (M[i][j] -
 *   L[i][0]*L[j][0] - ... - L[i][j-1]*L[j][j-1]) / L[j][j].  Then y_i = (-b_i - L[i][0]*y_0 - ... - L[i][i-1]*y_{i-1}) / L[i][i]
 *   for i = 0..5 and xi_i = (y_i - L[i+1][i]*xi_{i+1} - ... - L[5][i]*xi_5) / L[i][i] for i = 5..0.
 *   xi = (omega, tau); w = 0.5*omega; f = 2 / (1 + ((w.x*w.x + w.y*w.y) + w.z*w.z)); W = [w]x = {{0, -w.z, w.y}, {w.z, 0, -w.x},
 *   {-w.y, w.x, 0}}; R(omega)[i][j] = I[i][j] + f * (W[i][j] + ((W[i][0]*W[0][j] + W[i][1]*W[1][j]) + W[i][2]*W[2][j])) (Cayley).
 *   R_k[i][j] = (Rw[i][0]*R[0][j] + Rw[i][1]*R[1][j]) + Rw[i][2]*R[2][j];  t_k[i] = (c[i] + ((Rw[i][0]*e0 + Rw[i][1]*e1) +
 *   Rw[i][2]*e2)) + tau[i], e = t - c.
 *   HFPF_TRACK_CONVERGED and stop when (omega.x^2 + omega.y^2) + omega.z^2 < eps_rotation^2 and likewise tau against
 *   eps_translation (the update is applied first); otherwise stop after max_iterations.
 * The result: pose = the last estimate (T0 when the first system was TOO_FEW or DEGENERATE), iterations = systems evaluated;
 * inliers, rms = sqrt(rr / inliers) (0 without inliers) and information = A describe the last system evaluated.  points_used
 * counts the used points (the same in every iteration).  HFPF_OK is returned whenever the arguments are valid, also for
 * TOO_FEW, DEGENERATE, an empty handle and a handle before its first clean pass.  A track changes nothing on the handle except
 * device_bytes (its scratch: a host frame's copy, the view's z-buffer, 240 bytes of sums).  Rejected with HFPF_ERR_BAD_ARG (the
 * handle stays usable, the result is not written): struct_size != sizeof (options or result), reserved != 0, max_iterations
 * outside 1..64, stride outside 1..16, min_inliers < 6, not 0 < max_distance <= 1, damping not finite and >= 0, eps_rotation or
 * eps_translation not finite and >= 0, an invalid view (the checks of hfpf_render_opts), a NULL or non-finite pose, a NULL
 * result, more than 2^26 sampled points; for depth images every check of hfpf_depth_image (colour fields included; no colour
 * image is read) and, on the device, an image not aligned to its sample size; for clouds a NULL buffer, n_points = 0, offsets or
 * point_step not multiples of 4, an offset + 4 beyond point_step.  A handle with an RCCL communicator returns HFPF_ERR_STATE,
 * as render does.  Every call returns when the result is complete. */
#define HFPF_TRACK_CONVERGED 1u  /* the last update was below both eps */
#define HFPF_TRACK_DEGENERATE 2u /* a pivot of the damped system was <= 0; pose = the last good estimate */
#define HFPF_TRACK_TOO_FEW 4u    /* fewer than min_inliers inliers; pose = the last good estimate */

typedef struct hfpf_track_opts {
    uint32_t struct_size;    /* = sizeof(hfpf_track_opts) */
    uint32_t max_iterations; /* 1..64 */
    uint32_t stride;         /* 1..16: the sampling above */
    uint32_t min_inliers;    /* >= 6 */
    hfpf_render_opts view;   /* the model view, rendered once at the input pose (HFPF_RENDER_WORLD_NORMALS has no effect) */
    double max_distance;     /* association gate in metres, 0 < max_distance <= 1 */
    double damping;          /* >= 0, added to the diagonal of the 6x6 system */
    double eps_rotation;     /* radians */
    double eps_translation;  /* metres */
    uint64_t reserved;       /* 0 */
} hfpf_track_opts;

typedef struct hfpf_track_result {
    uint32_t struct_size;    /* = sizeof(hfpf_track_result), set by the caller */
    uint32_t iterations;
    uint32_t flags;          /* HFPF_TRACK_* */
    uint32_t reserved;
    uint64_t points_used;    /* sampled points that are finite and pass the z-clip */
    uint64_t inliers;        /* of the last system evaluated */
    double rms;              /* sqrt(rr / inliers) of that system */
    double information[36];  /* its undamped J^T J, row-major, twist order (omega, tau) about the input camera centre */
    double pose[12];         /* refined pose, row-major [R|t], camera -> fusion frame */
} hfpf_track_result;

/* A depth image in pageable HOST memory (copied once per call through pinned staging). */
int hfpf_track_depth(hfpf_handle* h, const hfpf_track_opts* o, const hfpf_depth_image* desc, const void* depth, const double pose_3x4[12],
                     hfpf_track_result* result);
/* A depth image in DEVICE memory, read in place. */
int hfpf_track_depth_device(hfpf_handle* h, const hfpf_track_opts* o, const hfpf_depth_image* desc, const void* dev_depth,
                            const double pose_3x4[12], hfpf_track_result* result);
/* A cloud of n_points records of point_step bytes in pageable HOST memory, f32 x, y, z at the given byte offsets (as integrate). */
int hfpf_track(hfpf_handle* h, const hfpf_track_opts* o, const void* base, uint32_t n_points, uint32_t point_step, uint32_t off_x,
               uint32_t off_y, uint32_t off_z, const double pose_3x4[12], hfpf_track_result* result);

/* ---- querying the fused model at given points (nearest row within a voxel window; no reference counterpart) ----------------
 * A query takes points (a cloud or a depth image) and a pose T (row-major [R|t], camera -> fusion frame, the integrate
 * convention) and answers per point: its voxel, whether that voxel is occupied or holds a row, and the nearest row within a
 * window of voxels around it.  Everything is restatable from hfpf_extract's rows and hfpf_get_occupied's list.  Per point i:
 * Input: cloud record i's f32 x, y, z; depth pixel i = (i % width, i / width) back-projected by the f32 arithmetic of the
 *   depth-frame contract above (invalid pixels are NaN).  The point is USED iff x, y, z are finite and, with HFPF_QUERY_ZCLIP,
 *   z_clip_min < z < z_clip_max (the handle's z-clip, as integrate applies it).  An unused point gets flags = 0,
 *   voxel = INT_MIN on each axis, p = NaN and the "not found" values below.
 * Fusion frame: p = (float)(((T[0]*x + T[1]*y) + T[2]*z) + T[3]), likewise rows 1 and 2 (f64, x widened; the rounding of
 *   integrate).  voxel[a] = (int)floor(((double)p[a] - bbox_min[a]) / res) with res = hfpf_get_dims' resolution, INT_MIN when
 *   that is NaN or outside the int range: the voxel integrate puts the same point in.  IN_BBOX iff
 *   bbox_min[a] < (double)p[a] < bbox_max[a] on every axis.  OCCUPIED (IN_BBOX points only) iff hfpf_get_occupied lists voxel.
 * Candidates (USED and IN_BBOX points only): the rows hfpf_extract would return at this point of the call sequence (host frames
 *   still waiting are launched first) with count >= max(1, min_count) (the compare of hfpf_extract_opts) and
 *   max(|ix - voxel[0]|, |iy - voxel[1]|, |iz - voxel[2]|) <= radius.  HAS_ROW iff the row of voxel itself is a candidate.
 * Distance, f64, left to right, never contracted: d = ((double)p[0] - (double)row.x, ... y, ... z),
 *   d2 = (d.x*d.x + d.y*d.y) + d.z*d.z; a candidate is kept iff d2 <= max_distance * max_distance.
 * Winner: the kept candidate with the smallest d2; ties go to the lexicographically smallest (ix, iy, iz) (the smallest extract
 *   row index), so results do not depend on scheduling.  With a winner: FOUND, row_voxel = its (ix, iy, iz), row_count = its
 *   count, distance = (float)sqrt(d2), signed_distance = (float)(((double)nx*d.x + (double)ny*d.y) + (double)nz*d.z) (> 0 on the
 *   side the normal faces, i.e. the sensor side), and rows[i] = its hfpf_row, byte-identical to hfpf_extract's (no colour coding).
 *   Without one: row_voxel = -1, row_count = 0, distance = signed_distance = NaN (0x7FC00000), rows[i] = {ix = iy = iz = -1, every
 *   other field 0}.  reserved words are 0.
 * A query changes nothing on the handle except device_bytes (its scratch: for host forms the input and up to 2^20 points of
 * output per chunk; chunks do not change a byte of the result).  Rejected with HFPF_ERR_BAD_ARG (the handle stays usable, nothing
 * is written): struct_size != sizeof, unknown flags, reserved0 or reserved != 0, radius outside 0..4, min_count NaN, not
 * max_distance > 0 (+inf allowed), a NULL or non-finite pose, NULL hits; for clouds a NULL buffer, offsets or point_step not
 * multiples of 4, an offset + 4 beyond point_step, and on the device a buffer not 4-byte or hits / rows not 16-byte aligned; for depth
 * images every check of hfpf_depth_image (colour fields included; no colour image is read).  n_points = 0 returns HFPF_OK after
 * these checks (buffer and hits may then be NULL) and writes nothing.  A handle with an RCCL communicator returns HFPF_ERR_STATE
 * (a distributed query is not provided); a failed handle returns HFPF_ERR_STATE as extract does.  Every call returns when its
 * outputs are complete. */
#define HFPF_QUERY_ZCLIP 1u      /* opts.flags: apply the handle's camera-frame z-clip to the input point, as integrate does */

typedef struct hfpf_query_opts {
    uint32_t struct_size;        /* = sizeof(hfpf_query_opts) */
    uint32_t flags;              /* HFPF_QUERY_* */
    int32_t radius;              /* 0..4: Chebyshev half-width, in voxels, of the cube searched around the point's voxel */
    int32_t reserved0;           /* 0 */
    double min_count;            /* rows with count < max(1, min_count) are not candidates */
    double max_distance;         /* > 0, +inf allowed: candidates farther than this are ignored */
    uint64_t reserved;           /* 0 */
} hfpf_query_opts;

#define HFPF_QHIT_USED 1u        /* x, y, z finite (and inside the z-clip with HFPF_QUERY_ZCLIP) */
#define HFPF_QHIT_IN_BBOX 2u     /* the transformed point passes integrate's bounding-box test */
#define HFPF_QHIT_OCCUPIED 4u    /* its voxel is occupied (as hfpf_get_occupied lists it) */
#define HFPF_QHIT_HAS_ROW 8u     /* its voxel itself holds a candidate row (whatever max_distance says) */
#define HFPF_QHIT_FOUND 16u      /* a nearest row was found; row_voxel / distance / signed_distance / rows[i] describe it */

typedef struct hfpf_query_hit {  /* 64 bytes */
    int32_t voxel[3];            /* the point's voxel as integrate indexes it (INT_MIN when not USED) */
    uint32_t flags;              /* HFPF_QHIT_* */
    int32_t row_voxel[3];        /* the nearest row's (ix, iy, iz); -1 when not FOUND */
    uint32_t row_count;          /* its count; 0 when not FOUND */
    float p[3];                  /* the point in the fusion frame, f32 as integrate rounds it (NaN when not USED) */
    float distance;              /* |p - row|; NaN when not FOUND */
    float signed_distance;       /* row normal . (p - row); NaN when not FOUND */
    uint32_t reserved[3];        /* 0 */
} hfpf_query_hit;

#ifdef __cplusplus
static_assert(sizeof(hfpf_query_opts) == 40, "hfpf_query_opts is 40 bytes");
static_assert(sizeof(hfpf_query_hit) == 64, "hfpf_query_hit is 64 bytes");
#else
_Static_assert(sizeof(hfpf_query_opts) == 40, "hfpf_query_opts is 40 bytes");
_Static_assert(sizeof(hfpf_query_hit) == 64, "hfpf_query_hit is 64 bytes");
#endif

/* A cloud of n_points records of point_step bytes in pageable HOST memory (layout as hfpf_integrate / hfpf_track); hits[i] and
 * rows[i] (rows optional: NULL = not produced) describe record i. */
int hfpf_query(hfpf_handle* h, const hfpf_query_opts* o, const void* base, uint32_t n_points, uint32_t point_step, uint32_t off_x,
               uint32_t off_y, uint32_t off_z, const double pose_3x4[12], hfpf_query_hit* hits, hfpf_row* rows);
/* The same cloud in DEVICE memory, read in place; dev_hits / dev_rows are DEVICE pointers. */
int hfpf_query_device(hfpf_handle* h, const hfpf_query_opts* o, const void* dev_base, uint32_t n_points, uint32_t point_step,
                      uint32_t off_x, uint32_t off_y, uint32_t off_z, const double pose_3x4[12], hfpf_query_hit* dev_hits,
                      hfpf_row* dev_rows);
/* A depth image (no colour is read) in pageable HOST memory; hit / row i = pixel (i % width, i / width). */
int hfpf_query_depth(hfpf_handle* h, const hfpf_query_opts* o, const hfpf_depth_image* desc, const void* depth,
                     const double pose_3x4[12], hfpf_query_hit* hits, hfpf_row* rows);

/* ---- a triangle mesh of the fused model (point-set surface; no reference counterpart) ----------------------------------------
 * The zero set of "signed distance to the tangent plane of the nearest row" (hfpf_query's signed_distance), sampled on the voxel
 * corner lattice and polygonised by Kuhn tetrahedra (Hoppe et al. 1992).  Everything is restatable from hfpf_extract's rows and
 * hfpf_get_occupied's list (tests/mesh_ref.py):
 * Rows: the candidates hfpf_query would use at this point of the call sequence (host frames still waiting are launched first):
 *   count >= max(1, min_count), centroid = the extracted row's x, y, z.
 * Lattice point (i, j, k), 0 <= i <= dim_x (likewise j, k), sits at c[a] = (float)(bbox_min[a] + (double)i_a * res), one f64
 *   multiply and add, one rounding.  Its sample is the hfpf_query hit of the f32 point c under the identity pose with the given
 *   radius, min_count and max_distance (no z-clip).  The sample is DEFINED iff that hit is FOUND; its value s is the hit's
 *   signed_distance, its row the hit's row.  Lattice points on the bounding box's faces are never IN_BBOX (query's bbox test is
 *   strict), so they are never defined and cubes touching the box stay open.
 * Cubes: cube (ix, iy, iz) spans lattice points (ix..ix+1, iy..iy+1, iz..iz+1).  The candidate cubes are the valid cells (0..dim-1)
 *   within Chebyshev distance 1 of a candidate row's cell.  A cube is MESHED iff all 8 corner samples are defined.  (With radius >= 2
 *   the row that makes a cube a candidate lies in the window of each of its corners.)
 * Tetrahedra: a meshed cube splits into the 6 Kuhn tetrahedra along its (0,0,0)-(1,1,1) diagonal: for the axis permutations pi in
 *   the order xyz, xzy, yxz, yzx, zxy, zyx, tetrahedron T has the corners (local index 0..3) 0, e_pi1, e_pi1 + e_pi2, (1,1,1).  A
 *   corner is INSIDE iff s < 0.  Neighbouring cubes share their face diagonals, so the mesh has no cracks and no ambiguous case.
 * Vertices: one per lattice edge that is an edge of a meshed tetrahedron and whose endpoints differ in inside/outside.  A lattice
 *   edge is (origin a, direction d), d one of the 7 offsets in {0,1}^3 \ {0}, numbered 0..6 in lexicographic order of the offset
 *   ((0,0,1), (0,1,0), (0,1,1), (1,0,0), (1,0,1), (1,1,0), (1,1,1)); b = a + d.  Position, f64, left to right, never contracted:
 *   t = (double)s_a / ((double)s_a - (double)s_b), p = (float)((double)c_a + t * ((double)c_b - (double)c_a)) per axis.  nx, ny, nz,
 *   rgb and count are those of the row of the endpoint with the smaller |s| (a tie goes to a); rgb as hfpf_extract codes it
 *   (0x00RRGGBB with HFPF_FLAG_FUSE_COLOR, 0 without).  Order: lexicographic by a's (i, j, k), then by direction, so the mesh is
 *   welded and does not depend on scheduling.
 * Triangles: a tetrahedron with one or three inside corners gives one triangle, (e00, e01, e02) or (e00, e10, e20); two inside
 *   corners give the quad (e00, e01, e11), (e00, e11, e10), where eIO is the edge from the I-th inside to the O-th outside corner,
 *   each counted in local index order.  When the triangle's face normal, with its vertices at the edge midpoints, does not point from
 *   the inside corners to the outside ones (|I| * sum(outside) - |O| * sum(inside)), its second and third vertices swap: faces look to
 *   the sensor side, as row normals do.  Order: by the cube's (ix, iy, iz), then tetrahedron 0..5, then triangle 0..1.
 * Limitation: the function is only as consistent as the rows' orientation.  A row seen at grazing angles (near a silhouette) can
 * be oriented away from the surface's outside; an edge between its sample and a neighbour's then changes sign without crossing the
 * surface, and its vertex lies up to one lattice edge off it (on the synthetic sphere of tests/test_gpu_mesh.py at 2 mm: 1.8 % of
 * the sphere's vertices; the vertices whose two endpoint rows face outwards lie within 0.7 mm, 99 % within 0.3 mm).
 * A mesh changes nothing on the handle except device_bytes (its scratch: per corner its key and 20 bytes of samples, marks and
 * counts, per cube its key and 8 bytes of triangle counts, sort buffers of up to three times the largest set, and for the host form
 * the output; scratch grows by 25 % headroom when it grows).  A corner that the construction does not find in its own corner set
 * (an internal error) fails the call with HFPF_ERR_STATE and returns no mesh.  A handle before its first clean pass returns HFPF_OK with 0 vertices and 0 triangles
 * (and NULL arrays).  Rejected with HFPF_ERR_BAD_ARG (the handle stays usable, nothing is written): struct_size != sizeof, flags or
 * reserved != 0, radius outside 1..4, min_count NaN, max_distance NaN or not > 0 (+inf allowed), a NULL output pointer.  A handle
 * with an RCCL communicator returns HFPF_ERR_STATE; a failed handle returns HFPF_ERR_STATE as extract does.  Every call returns when
 * its outputs are complete. */
typedef struct hfpf_mesh_opts {
    uint32_t struct_size;        /* = sizeof(hfpf_mesh_opts) */
    int32_t radius;              /* 1..4 (typically 2): the query window of every corner sample */
    double min_count;            /* rows with count < max(1, min_count) are not candidates */
    double max_distance;         /* > 0, +inf allowed: the query's distance gate; corners farther from every row stay undefined */
    uint32_t flags;              /* 0 */
    uint32_t reserved;           /* 0 */
} hfpf_mesh_opts;

typedef struct hfpf_mesh_vertex { /* 32 bytes */
    float x, y, z;
    float nx, ny, nz;            /* the attribute row's normal */
    uint32_t rgb;                /* its colour, 0x00RRGGBB */
    uint32_t count;              /* its count */
} hfpf_mesh_vertex;

#ifdef __cplusplus
static_assert(sizeof(hfpf_mesh_opts) == 32, "hfpf_mesh_opts is 32 bytes");
static_assert(sizeof(hfpf_mesh_vertex) == 32, "hfpf_mesh_vertex is 32 bytes");
#else
_Static_assert(sizeof(hfpf_mesh_opts) == 32, "hfpf_mesh_opts is 32 bytes");
_Static_assert(sizeof(hfpf_mesh_vertex) == 32, "hfpf_mesh_vertex is 32 bytes");
#endif

/* HFPF_OK if o passes the checks above, else HFPF_ERR_BAD_ARG (host code, no handle; the node shell uses it too). */
int hfpf_check_mesh_opts(const hfpf_mesh_opts* o);
/* The mesh in HOST memory: *verts (n_verts) and *tris (3 * n_tris vertex indices), freed by hfpf_free_mesh. */
int hfpf_extract_mesh(hfpf_handle* h, const hfpf_mesh_opts* o, hfpf_mesh_vertex** verts, uint64_t* n_verts, uint32_t** tris, uint64_t* n_tris);
void hfpf_free_mesh(hfpf_mesh_vertex* verts, uint32_t* tris);
/* The same mesh in DEVICE memory (HBM), each array freed by hfpf_device_free(h, p). */
int hfpf_extract_mesh_device(hfpf_handle* h, const hfpf_mesh_opts* o, hfpf_mesh_vertex** dev_verts, uint64_t* n_verts, uint32_t** dev_tris,
                             uint64_t* n_tris);
/* PLY, format binary_little_endian 1.0: per vertex float x y z nx ny nz, uchar red green blue (from rgb); per face
 * list uchar uint vertex_indices.  Host code, no GPU needed. */
int hfpf_write_ply(const hfpf_mesh_vertex* verts, uint64_t n_verts, const uint32_t* tris, uint64_t n_tris, const char* path);

/* ---- casting rays against the fused model (first surface crossing per ray; no reference counterpart) ------------------------
 * The surface is the mesh's: the zero set of "signed distance to the tangent plane of the nearest row" (hfpf_query's
 * signed_distance), sampled along rays instead of on the lattice.  Everything is restatable from hfpf_extract's rows and
 * hfpf_get_occupied's list (tests/raycast_ref.py).  Arithmetic is f64, one rounding per operation, left to right, never contracted.
 * T is a row-major [R|t], camera -> fusion frame.
 * General ray i: a packed hfpf_ray {o, d} in the camera frame.  O[a] = ((T[4a]*ox + T[4a+1]*oy) + T[4a+2]*oz) + T[4a+3],
 *   W[a] = (T[4a]*dx + T[4a+1]*dy) + T[4a+2]*dz, L = sqrt((W0*W0 + W1*W1) + W2*W2), D[a] = W[a] / L.  The ray is USED iff its six
 *   inputs are finite and L is finite and > 0.  t0 = t_min, t1 = t_max, metres along the ray.
 * View ray of pixel (u, v), i = v*width + u, of the pinhole (width, height, fx, fy, cx, cy): xn = ((double)u - cx) / fx,
 *   yn = ((double)v - cy) / fy, O = (T[3], T[7], T[11]), D[a] = (T[4a]*xn + T[4a+1]*yn) + T[4a+2].  D is NOT normalised: the ray
 *   parameter is the camera-frame depth, so t compares directly with a depth frame and with hfpf_render's depth plane.  Always
 *   USED.  t0 = t_min is z_near, t1 = t_max is z_far.
 * Samples: dt = step * res (res = hfpf_get_dims' resolution), n = (uint64)floor((t1 - t0) / dt) + 1, t_k = t0 + (double)k * dt for
 *   k = 0..n-1 (from k, never accumulated), p_k[a] = (float)(O[a] + t_k * D[a]).  Sample k is the hfpf_query hit of the f32 point p_k
 *   under the identity pose with the call's radius, min_count and max_distance and no z-clip: exactly a mesh corner sample.  It is
 *   DEFINED iff that hit is FOUND; then s_k is its signed_distance (f32) and its row the hit's row.
 * Crossing: the ray ends at the smallest k >= 1 for which samples k-1 and k are both defined and (s_{k-1} < 0) != (s_k < 0) (INSIDE
 *   iff s < 0, as in the mesh).  s_{k-1} >= 0 > s_k is a front crossing; the other direction sets HFPF_RAY_BACKFACE, and with
 *   HFPF_RAYCAST_CULL_BACKFACES it does not end the ray: the march goes on.
 * Hit: w = (double)s_{k-1} / ((double)s_{k-1} - (double)s_k), th = t_{k-1} + w * dt, t = (float)th, p[a] = (float)(O[a] + th * D[a]),
 *   sample = k.  n, row_voxel, rgb and count are those of the row of the endpoint with the smaller |s| (a tie goes to k-1); rgb as
 *   hfpf_extract codes it, the normal as stored (fusion frame).
 * Flags: USED; HIT; BACKFACE; NEAR = some sample up to the end of the march was defined (the ray came within the window of a row).
 * No hit: t, p and n are NaN (0x7FC00000), row_voxel = -1, rgb = count = sample = 0.  An unused ray has flags = 0 and the same values.
 * Limitation (the mesh's, unchanged): the function is only as consistent as the rows' orientation.  A row oriented inwards near a
 * silhouette gives a sign change between its sample and a neighbour's that is not a crossing of the surface.
 * A raycast changes nothing on the handle except device_bytes (its scratch: one byte per brick, per 4^3 and per 16^3 bricks of
 * empty-space maps, and for the host forms up to 2^20 rays and hits per chunk; chunks do not change a byte of the result).  Host
 * frames still waiting are launched first.  A handle before its first clean pass returns no hits.  Rejected with HFPF_ERR_BAD_ARG
 * (the handle stays usable, nothing is written): struct_size != sizeof, unknown flags, reserved0 or reserved != 0, radius outside
 * 1..4, min_count NaN, not max_distance > 0 (+inf allowed), step not finite or outside 0.125..4, t_min / t_max not finite or not
 * 0 <= t_min < t_max, more than 2^20 samples per ray, a NULL or non-finite pose, NULL hits, a NULL ray buffer with n_rays > 0; for
 * views width * height = 0 or above 2^31, fx or fy not finite and positive, cx or cy not finite; on the device rays not 4-byte or
 * hits not 16-byte aligned.  n_rays = 0 (n_views = 0) returns HFPF_OK after these checks.  A handle with an RCCL communicator
 * returns HFPF_ERR_STATE (a distributed raycast is not provided); a failed handle returns HFPF_ERR_STATE as extract does.  Every
 * call returns when its outputs are complete. */
#define HFPF_RAYCAST_CULL_BACKFACES 1u /* opts.flags: a back crossing does not end the ray */

typedef struct hfpf_ray {        /* 24 bytes, packed */
    float o[3];                  /* origin, camera frame */
    float d[3];                  /* direction, camera frame, any length > 0 */
} hfpf_ray;

typedef struct hfpf_raycast_opts {
    uint32_t struct_size;        /* = sizeof(hfpf_raycast_opts) */
    uint32_t flags;              /* HFPF_RAYCAST_* */
    int32_t radius;              /* 1..4 (typically 2): the query window of every sample */
    int32_t reserved0;           /* 0 */
    double min_count;            /* rows with count < max(1, min_count) are not candidates */
    double max_distance;         /* > 0, +inf allowed: the query's distance gate */
    double step;                 /* sample spacing in voxels, 0.125..4 (0.5 is the documented default) */
    double t_min, t_max;         /* finite, 0 <= t_min < t_max: metres along a general ray, z_near / z_far of a view */
    uint64_t reserved;           /* 0 */
} hfpf_raycast_opts;

#define HFPF_RAY_USED 1u         /* finite inputs and a direction of finite length > 0 (view rays: always) */
#define HFPF_RAY_HIT 2u          /* a crossing ended the ray; t / p / n / row_voxel / rgb / count / sample describe it */
#define HFPF_RAY_BACKFACE 4u     /* that crossing goes from inside (s < 0) to outside */
#define HFPF_RAY_NEAR 8u         /* some sample of the march was defined */

typedef struct hfpf_ray_hit {    /* 64 bytes */
    float t;                     /* ray parameter of the crossing (metres; camera-frame depth for views); NaN without a hit */
    uint32_t flags;              /* HFPF_RAY_* */
    float p[3];                  /* the crossing in the fusion frame */
    float n[3];                  /* the attribute row's normal, as stored */
    int32_t row_voxel[3];        /* its (ix, iy, iz); -1 without a hit */
    uint32_t rgb;                /* its colour as hfpf_extract codes it */
    uint32_t count;              /* its count */
    uint32_t sample;             /* k: the crossing lies between samples k-1 and k */
    uint32_t reserved[2];        /* 0 */
} hfpf_ray_hit;

#ifdef __cplusplus
static_assert(sizeof(hfpf_ray) == 24, "hfpf_ray is 24 bytes");
static_assert(sizeof(hfpf_raycast_opts) == 64, "hfpf_raycast_opts is 64 bytes");
static_assert(sizeof(hfpf_ray_hit) == 64, "hfpf_ray_hit is 64 bytes");
#else
_Static_assert(sizeof(hfpf_ray) == 24, "hfpf_ray is 24 bytes");
_Static_assert(sizeof(hfpf_raycast_opts) == 64, "hfpf_raycast_opts is 64 bytes");
_Static_assert(sizeof(hfpf_ray_hit) == 64, "hfpf_ray_hit is 64 bytes");
#endif

/* HFPF_OK if o passes the struct checks above, else HFPF_ERR_BAD_ARG (host code, no handle; the sample count needs a handle's
 * resolution and is checked by the calls). */
int hfpf_check_raycast_opts(const hfpf_raycast_opts* o);
/* n_rays rays in pageable HOST memory, hits[i] in HOST memory describes ray i. */
int hfpf_raycast(hfpf_handle* h, const hfpf_raycast_opts* o, const hfpf_ray* rays, uint64_t n_rays, const double pose_3x4[12],
                 hfpf_ray_hit* hits);
/* The same with rays and hits in DEVICE memory: one launch into the caller's buffers. */
int hfpf_raycast_device(hfpf_handle* h, const hfpf_raycast_opts* o, const hfpf_ray* dev_rays, uint64_t n_rays, const double pose_3x4[12],
                        hfpf_ray_hit* dev_hits);
/* The width * height view rays of one pinhole view; hits in HOST memory. */
int hfpf_raycast_view(hfpf_handle* h, const hfpf_raycast_opts* o, uint32_t width, uint32_t height, double fx, double fy, double cx, double cy,
                      const double pose_3x4[12], hfpf_ray_hit* hits);
/* n_views views (poses: n_views * 12 doubles in HOST memory); view v's hits start v * width * height behind dev_hits (DEVICE memory). */
int hfpf_raycast_view_device(hfpf_handle* h, const hfpf_raycast_opts* o, uint32_t width, uint32_t height, double fx, double fy, double cx,
                             double cy, uint32_t n_views, const double* poses, hfpf_ray_hit* dev_hits);

/* ---- connected components of the fused model, and the model without its specks (no reference counterpart) ---------------------
 * Tells which rows belong together and drops the small islands that float off the surface (flying pixels at depth
 * discontinuities, a cable that crossed the view), which a count threshold alone cannot remove.  Everything is restatable from
 * hfpf_extract_filtered's rows (tests/components_ref.py).
 * Row set: the rows hfpf_extract_filtered would return at this point of the call sequence with the same min_count (rows with
 *   count < min_count are dropped; 0 keeps all), in lexicographic (ix, iy, iz) order; host frames still waiting are launched first.
 *   Row j below is the j-th of them.
 * Adjacency: rows a and b are adjacent iff max(|ix_a - ix_b|, |iy_a - iy_b|, |iz_a - iz_b|) <= reach (1..4; reach 1 is the
 *   26-neighbourhood) and ((double)nx_a*(double)nx_b + (double)ny_a*(double)ny_b) + (double)nz_a*(double)nz_b >= min_normal_dot:
 *   f64, left to right, never contracted, on the stored f32 normals.  The dot is taken as is (no absolute value), so it inherits the
 *   rows' orientation as mesh and raycast do.  The expression is symmetric in a and b, so the relation is; a NaN compares false.
 *   min_normal_dot = -2 is off: no pair of stored (unit) normals falls below it.
 * Components: the equivalence classes of the transitive closure.  A component's representative is its smallest row index.
 * Per component: n_rows = the number of its rows, points = the uint64 sum of their count, lo / hi = the min / max of their voxel
 *   indices per axis.  All integer reductions: nothing depends on scheduling.
 * Kept: a component is kept iff n_rows >= min_rows, points >= min_points and (keep_largest == 0 or rank < keep_largest), its rank
 *   being its position when the components that pass the first two tests are ordered by n_rows descending, then representative
 *   ascending.
 * Outputs: rows = the rows of the kept components in their original order, byte-identical to hfpf_extract_filtered's (no colour
 *   coding); labels[i] = the component of output row i, the kept components numbered 0..n_comps-1 by ascending representative;
 *   comps[c] = the hfpf_component below.  With min_rows = min_points = keep_largest = 0 the output is the plain labelling of every row.
 * A call changes nothing on the handle except device_bytes (its scratch: 4 bytes per normal record, 24 per row, 64 per component,
 * the sort and scan buffers and, for the host form, the output).  Render, track, query, mesh and raycast do NOT honour a component
 * filter, unless hidden with hfpf_hide_voxels: they see every row.  Rejected with HFPF_ERR_BAD_ARG (the handle stays usable, nothing is written): struct_size != sizeof,
 * flags, reserved0 or reserved != 0, reach outside 1..4, min_count NaN, min_normal_dot not finite or outside [-2, 1], a NULL n_rows,
 * n_comps, labels or comps pointer (rows may be NULL: not produced).  An empty handle, or one before its first clean pass, returns
 * HFPF_OK with 0 rows, 0 components and NULL arrays.  A handle with an RCCL communicator returns HFPF_ERR_STATE (a distributed form
 * is not provided); a failed handle returns HFPF_ERR_STATE as extract does.  Every call returns when its outputs are complete. */
typedef struct hfpf_component_opts {
    uint32_t struct_size;        /* = sizeof(hfpf_component_opts) */
    uint32_t flags;              /* 0 */
    int32_t reach;               /* 1..4: Chebyshev distance, in voxels, up to which two rows are neighbours */
    int32_t reserved0;           /* 0 */
    double min_count;            /* rows with count < min_count are dropped before the labelling (0 keeps all) */
    double min_normal_dot;       /* -2..1: neighbours are joined only when their normals' dot product reaches it; -2 = off */
    uint32_t min_rows;           /* components with fewer rows are dropped (0 keeps all) */
    uint32_t keep_largest;       /* 0 = off; else only the keep_largest largest components (by n_rows) are kept */
    uint64_t min_points;         /* components whose counts sum to less are dropped (0 keeps all) */
    uint64_t reserved;           /* 0 */
} hfpf_component_opts;

typedef struct hfpf_component {  /* 48 bytes */
    uint32_t first_row;          /* index of the representative in the output rows */
    uint32_t n_rows;             /* rows of the component */
    uint64_t points;             /* sum of count over its rows */
    int32_t lo[3];               /* min voxel index per axis */
    int32_t hi[3];               /* max voxel index per axis */
    uint32_t source_row;         /* the representative's index in the row set (before the keep tests; after the min_count gate) */
    uint32_t reserved;           /* 0 */
} hfpf_component;

#ifdef __cplusplus
static_assert(sizeof(hfpf_component_opts) == 56, "hfpf_component_opts is 56 bytes");
static_assert(sizeof(hfpf_component) == 48, "hfpf_component is 48 bytes");
#else
_Static_assert(sizeof(hfpf_component_opts) == 56, "hfpf_component_opts is 56 bytes");
_Static_assert(sizeof(hfpf_component) == 48, "hfpf_component is 48 bytes");
#endif

/* HFPF_OK if o passes the checks above, else HFPF_ERR_BAD_ARG (host code, no handle; the node shell uses it too). */
int hfpf_check_component_opts(const hfpf_component_opts* o);
/* Rows (optional: rows == NULL = not produced), labels (n_rows of each) and components (n_comps) in HOST memory, freed by
 * hfpf_free_components. */
int hfpf_extract_components(hfpf_handle* h, const hfpf_component_opts* o, hfpf_row** rows, uint32_t** labels, uint64_t* n_rows,
                            hfpf_component** comps, uint64_t* n_comps);
void hfpf_free_components(hfpf_row* rows, uint32_t* labels, hfpf_component* comps);
/* The same in DEVICE memory (HBM), each array freed by hfpf_device_free(h, p). */
int hfpf_extract_components_device(hfpf_handle* h, const hfpf_component_opts* o, hfpf_row** dev_rows, uint32_t** dev_labels, uint64_t* n_rows,
                                   hfpf_component** dev_comps, uint64_t* n_comps);

/* ---- deviation of the fused model from a triangle mesh (no reference counterpart) -----------------------------------------------
 * How far is what was scanned from what it should be: for every row of the model, the closest point of a reference surface (a CAD
 * model, an earlier scan's mesh.ply, hfpf_extract_mesh's own output) and the signed distance to it.  Everything is restatable from
 * hfpf_extract_filtered's rows (tests/deviation_ref.py).
 * Arithmetic: everything below is f64, one rounding per operation, left to right, never contracted.
 *   dot(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z; vector sums and differences per component.
 * Mesh: n_verts vertices, three packed f32 x, y, z at verts + i * vertex_stride (vertex_stride >= 12, a multiple of 4; 32 takes an
 *   hfpf_mesh_vertex array as hfpf_extract_mesh* returns it); 3 * n_tris u32 indices; pose_3x4 = row-major [R|t] from the mesh frame
 *   to the fusion frame.  Vertex coordinate a becomes V[a] = ((T[4a]*x + T[4a+1]*y) + T[4a+2]*z) + T[4a+3], x, y, z widened, V kept
 *   in f64 (not rounded back).
 * Valid triangles: triangle k with vertices A, B, C is VALID iff its three indices are < n_verts, its nine transformed coordinates
 *   are finite and NN = dot(N, N) is finite and > 0, where ab = B - A, ac = C - A,
 *   N = (ab.y*ac.z - ab.z*ac.y, ab.z*ac.x - ab.x*ac.z, ab.x*ac.y - ab.y*ac.x).  Invalid triangles are skipped and counted.  The
 *   device rejects an index out of range before it loads anything through it: a mesh in HBM is untrusted input.
 * Row set: the rows hfpf_extract_filtered would return at this point of the call sequence with the same min_count, in lexicographic
 *   (ix, iy, iz) order; host frames still waiting are launched first.  Row j has P = ((double)x, (double)y, (double)z).
 * Closest point Q of a valid triangle to P: the seven-region construction, the branches taken in exactly this order:
 *   ap = P-A; d1 = dot(ab,ap); d2 = dot(ac,ap);          d1<=0 && d2<=0            -> Q = A                             (VERTEX)
 *   bp = P-B; d3 = dot(ab,bp); d4 = dot(ac,bp);          d3>=0 && d4<=d3           -> Q = B                             (VERTEX)
 *   vc = d1*d4 - d3*d2;                                  vc<=0 && d1>=0 && d3<=0   -> v = d1/(d1-d3); Q = A + v*ab      (EDGE)
 *   cp = P-C; d5 = dot(ab,cp); d6 = dot(ac,cp);          d6>=0 && d5<=d6           -> Q = C                             (VERTEX)
 *   vb = d5*d2 - d1*d6;                                  vb<=0 && d2>=0 && d6<=0   -> w = d2/(d2-d6); Q = A + w*ac      (EDGE)
 *   va = d3*d6 - d5*d4; e = d4-d3; f = d5-d6;            va<=0 && e>=0 && f>=0     -> w = e/(e+f);    Q = B + w*(C-B)   (EDGE)
 *   otherwise  s = (va+vb)+vc; v = vb/s; w = vc/s;                                    Q = (A + v*ab) + w*ac             (FACE)
 *   r = P - Q, dd = dot(r, r).  The triangle is KEPT iff dd <= max_distance * max_distance (a NaN compares false).
 * Winner: the kept triangle with the smallest dd; ties go to the smallest triangle index, so the result depends on neither scheduling
 *   nor the acceleration structure.  With a winner: distance = (float)sqrt(dd); signed_distance = dot(N, r) < 0 ? -distance :
 *   distance (positive on the side the face's winding looks to); q = (float)Q per axis; tri = k; flags = HFPF_DEV_FOUND |
 *   (HFPF_DEV_ON_EDGE or HFPF_DEV_ON_VERTEX by region).  Without one: distance, signed_distance and q are NaN (0x7FC00000),
 *   tri = 0xFFFFFFFF, flags = 0.  reserved is 0 either way.
 *   LIMITATION: on an edge or vertex region the sign is the winning face's, not that of an angle-weighted pseudo-normal, so next to a
 *   sharp convex or concave edge a row can get the wrong sign.  The two flag bits exist so that a caller can tell.
 * Summary: integer and max reductions only, nothing depends on order.  The two sums are taken over the found rows from the f32
 *   distance of the output, widened: sum_abs_q30 = sum of rint((double)distance * 2^30), sum_sq_q30 = sum of
 *   rint(((double)distance * (double)distance) * 2^30).  max_distance <= 1 m (below), so 2^31 rows keep either under 2^61.
 * A call changes nothing on the handle except device_bytes (its scratch).  Rejected with HFPF_ERR_BAD_ARG (the handle stays usable,
 * nothing is written): what hfpf_check_deviation_opts rejects (struct_size != sizeof, flags or reserved != 0, min_count NaN,
 * max_distance not finite, not > 0 or > 1); max_distance > 32 * res (res = hfpf_get_dims' resolution: the bound that keeps the brick
 * search finite); a NULL or non-finite pose; vertex_stride < 12 or not a multiple of 4; NULL verts with n_verts != 0 or NULL tris with
 * n_tris != 0; n_verts or n_tris >= 2^32 - 1; NULL dev, n_rows or summary (rows may be NULL: not produced); for the device form verts
 * or tris not 4-byte aligned.  n_tris = 0 returns HFPF_OK with the row set and no row found; an empty handle, or one before its
 * first clean pass, returns HFPF_OK with 0 rows and NULL arrays.  When the list of (triangle, brick) pairs the search needs does not
 * fit (more than 2^32 - 2 pairs, or no memory for them) the call returns HFPF_ERR_CAPACITY, its message names the pair count, and the
 * handle stays usable.  A handle with an RCCL communicator, or a failed handle, returns HFPF_ERR_STATE as the other readers do. */
#define HFPF_DEV_FOUND 1u
#define HFPF_DEV_ON_EDGE 2u
#define HFPF_DEV_ON_VERTEX 4u

typedef struct hfpf_deviation_opts {
    uint32_t struct_size;        /* = sizeof(hfpf_deviation_opts) */
    uint32_t flags;              /* 0 */
    double min_count;            /* rows with count < min_count are not compared (0 keeps all) */
    double max_distance;         /* metres, > 0, <= 32 * res and <= 1: triangles farther from a row are not its winner */
    uint64_t reserved;           /* 0 */
} hfpf_deviation_opts;

typedef struct hfpf_deviation {  /* 32 bytes, one per row */
    float signed_distance;       /* +-distance: positive on the side the winning face's winding looks to */
    float distance;              /* (float)sqrt(dd) */
    uint32_t tri;                /* the winning triangle, 0xFFFFFFFF without one */
    uint32_t flags;              /* HFPF_DEV_* */
    float q[3];                  /* the closest point, fusion frame */
    uint32_t reserved;           /* 0 */
} hfpf_deviation;

typedef struct hfpf_deviation_summary {  /* 64 bytes */
    uint64_t n_rows;             /* rows compared */
    uint64_t n_found;            /* ... with a winner */
    uint64_t n_negative;         /* found rows with signed_distance < 0 */
    uint64_t n_tris_valid;
    uint64_t n_tris_invalid;
    float max_abs;               /* the largest distance, 0 without a found row */
    uint32_t pad;                /* 0 */
    int64_t sum_abs_q30;
    int64_t sum_sq_q30;
} hfpf_deviation_summary;

#ifdef __cplusplus
static_assert(sizeof(hfpf_deviation_opts) == 32, "hfpf_deviation_opts is 32 bytes");
static_assert(sizeof(hfpf_deviation) == 32, "hfpf_deviation is 32 bytes");
static_assert(sizeof(hfpf_deviation_summary) == 64, "hfpf_deviation_summary is 64 bytes");
#else
_Static_assert(sizeof(hfpf_deviation_opts) == 32, "hfpf_deviation_opts is 32 bytes");
_Static_assert(sizeof(hfpf_deviation) == 32, "hfpf_deviation is 32 bytes");
_Static_assert(sizeof(hfpf_deviation_summary) == 64, "hfpf_deviation_summary is 64 bytes");
#endif

/* HFPF_OK if o passes the checks above that need no handle, else HFPF_ERR_BAD_ARG (host code; the node shell uses it too). */
int hfpf_check_deviation_opts(const hfpf_deviation_opts* o);
/* Mesh, pose and outputs in HOST memory: *dev (and *rows when rows != NULL: the row set itself) hold *n_rows entries and are freed by
 * hfpf_free_deviation. */
int hfpf_compare_mesh(hfpf_handle* h, const hfpf_deviation_opts* o, const void* verts, uint64_t n_verts, uint32_t vertex_stride,
                      const uint32_t* tris, uint64_t n_tris, const double* pose_3x4, hfpf_row** rows, hfpf_deviation** dev, uint64_t* n_rows,
                      hfpf_deviation_summary* summary);
void hfpf_free_deviation(hfpf_row* rows, hfpf_deviation* dev);
/* The mesh is read in place from DEVICE memory (HBM); *dev_rows and *dev_dev are device arrays, each freed by hfpf_device_free(h, p).
 * pose_3x4 and summary are in host memory. */
int hfpf_compare_mesh_device(hfpf_handle* h, const hfpf_deviation_opts* o, const void* dev_verts, uint64_t n_verts, uint32_t vertex_stride,
                             const uint32_t* dev_tris, uint64_t n_tris, const double* pose_3x4, hfpf_row** dev_rows, hfpf_deviation** dev_dev,
                             uint64_t* n_rows, hfpf_deviation_summary* summary);
/* The inverse of hfpf_write_ply (host code, no GPU needed): *verts (n_verts) and *tris (3 * n_tris indices), freed by hfpf_free_mesh.
 * Accepts format binary_little_endian 1.0 only.  The vertex element must have float x, y, z; float nx, ny, nz and uchar red, green,
 * blue are optional (absent fields are 0; count is always 0); any other scalar property is skipped by its size.  The face element is
 * one list uchar uint|int vertex_indices with exactly 3 entries per face.  Other elements may follow the two, none may precede them.
 * Anything else is HFPF_ERR_IO with a message from hfpf_last_error(NULL).  The counts are checked against the bytes the file has
 * left before anything is allocated. */
int hfpf_read_ply(const char* path, hfpf_mesh_vertex** verts, uint64_t* n_verts, uint32_t** tris, uint64_t* n_tris);

/* ---- best-fitting a triangle mesh to the fused model (mesh-to-model point-to-plane ICP; no reference counterpart) ---------------
 * hfpf_compare_mesh measures the model against a mesh at a pose the caller knows; an align finds that pose.  It takes the mesh
 * arguments of the section "deviation of the fused model from a triangle mesh" above and a start pose T_0 = pose_3x4 (mesh frame ->
 * fusion frame) and returns a refined pose in the same convention; the caller then passes that pose to hfpf_compare_mesh.  It is
 * that section's closest-point search and the section "refining a frame's pose against the fused model"'s normal equations, host
 * solve and update, run in a loop, and nothing else (tests/align_ref.py).  All arithmetic is f64, one rounding per operation, left
 * to right, never contracted, as in both.
 * Row set: the row set of hfpf_compare_mesh with opts.compare.min_count, in lexicographic order; host frames still waiting are
 *   launched first.  Row j is SAMPLED iff j % stride == 0; rows_sampled counts them and must be at most 2^26.
 * Centre: c[a] = (bbox_min[a] + bbox_max[a]) * 0.5 (the handle's bounding box).
 * Per iteration k = 1, 2, ... with T = T_{k-1}, for every sampled row: D = the hfpf_deviation record hfpf_compare_mesh returns for
 *   that row against the mesh at T with opts.compare.max_distance -- exactly that record, its f32 fields included (a row's record
 *   depends on the row and the mesh only, so sampling changes no record).  The row is an INLIER iff
 *     D.flags & HFPF_DEV_FOUND;
 *     with HFPF_ALIGN_SKIP_BOUNDARY neither HFPF_DEV_ON_EDGE nor HFPF_DEV_ON_VERTEX is set (a row hanging past the rim of a partial
 *       mesh then does not pull on that rim; inside a closed mesh it drops the rows whose closest point lies on a crease);
 *     (n.x*n.x + n.y*n.y) + n.z*n.z <= 2, n = (double) of the row's nx, ny, nz;
 *     max(|a.x|, |a.y|, |a.z|) < 32 (metres: track's headroom rule)
 *   with P = (double) of the row's x, y, z, Q = (double)D.q, d = Q - P, a = Q - c.  Per inlier
 *     r = (n.x*d.x + n.y*d.y) + n.z*d.z
 *     J = (a.y*n.z - a.z*n.y, a.z*n.x - a.x*n.z, a.x*n.y - a.y*n.x, n.x, n.y, n.z)      (twist order omega, tau)
 *   and the inlier adds (int64) rint(v * s) for v = J_i*J_j (i <= j; s = 2^24), J_i*r (s = 2^28) and r*r (s = 2^32) into exact int64
 *   sums, as a track's inlier does, and 1 to the inlier count.  Headroom as there: |J_i| < 64, and |r| < 2 because max_distance <= 1.
 * On the host, word for word the track section: A, b, rr from the sums; inliers < min_inliers: HFPF_ALIGN_TOO_FEW, stop; Cholesky
 *   of A + damping*I, a pivot not > 0: HFPF_ALIGN_DEGENERATE, stop; the two triangular solves; the Cayley update about c,
 *   R_k = R(omega) R_{k-1}, t_k = (c + R(omega)(t_{k-1} - c)) + tau; HFPF_ALIGN_CONVERGED and stop when omega is below eps_rotation
 *   and tau below eps_translation (the update is applied first); otherwise stop after max_iterations.
 * The result: pose = the last estimate (T_0 when the first system was TOO_FEW or DEGENERATE), iterations = systems evaluated;
 * inliers, rms = sqrt(rr / inliers) (0 without inliers) and information = A describe the last system evaluated.  HFPF_OK is
 * returned whenever the arguments are valid: also for TOO_FEW and DEGENERATE, for an empty handle and one before its first clean
 * pass, and for n_tris = 0 (all three: TOO_FEW after one system, pose = T_0).  A call changes nothing on the handle except
 * device_bytes (its scratch: compare's, one deviation record per row, 232 bytes of sums).  Rejected with HFPF_ERR_BAD_ARG (the
 * handle stays usable, the result is not written): what hfpf_check_align_opts rejects (struct_size != sizeof, flags beyond
 * HFPF_ALIGN_SKIP_BOUNDARY, reserved0 or reserved != 0, max_iterations outside 1..64, stride outside 1..65536, min_inliers < 6,
 * damping, eps_rotation or eps_translation not finite and >= 0, and whatever hfpf_check_deviation_opts rejects of opts.compare);
 * every check hfpf_compare_mesh makes on the mesh, the pose and max_distance (at most 32 * res); a NULL result or one with a wrong
 * struct_size; more than 2^26 sampled rows.  The pair list not fitting returns HFPF_ERR_CAPACITY as in compare (the handle stays
 * usable); a handle with an RCCL communicator, or a failed handle, returns HFPF_ERR_STATE.
 * LIMITATION: a row finds the mesh only within opts.compare.max_distance, at most 32 voxels: that is the capture range.  An align
 * refines a coarse placement; it is not a global registration.
 * LIMITATION: the headroom rule is taken about the centre of the handle's bounding box, so a model all of which lies 32 m or more
 * (on one axis) from that centre has no inlier: HFPF_ALIGN_TOO_FEW after one system, pose = T_0.  A box with 2,097,150 cells of 2 mm
 * on an axis and the model at one end of it is such a case (tests/test_gpu_deep.py asserts this answer); a box up to 64 m across
 * around the model is not. */
#define HFPF_ALIGN_CONVERGED 1u  /* the last update was below both eps */
#define HFPF_ALIGN_DEGENERATE 2u /* a pivot of the damped system was <= 0; pose = the last good estimate */
#define HFPF_ALIGN_TOO_FEW 4u    /* fewer than min_inliers inliers; pose = the last good estimate */

#define HFPF_ALIGN_SKIP_BOUNDARY 1u /* hfpf_align_opts.flags: rows whose closest point lies on an edge or a vertex are no inliers */

typedef struct hfpf_align_opts {
    uint32_t struct_size;        /* = sizeof(hfpf_align_opts) */
    uint32_t flags;              /* HFPF_ALIGN_SKIP_BOUNDARY or 0 */
    uint32_t max_iterations;     /* 1..64 */
    uint32_t stride;             /* 1..65536: the row sampling above */
    uint32_t min_inliers;        /* >= 6 */
    uint32_t reserved0;          /* 0 */
    hfpf_deviation_opts compare; /* the row set's min_count and the search's max_distance (the capture range) */
    double damping;              /* >= 0, added to the diagonal of the 6x6 system */
    double eps_rotation;         /* radians */
    double eps_translation;      /* metres */
    uint64_t reserved;           /* 0 */
} hfpf_align_opts;

typedef struct hfpf_align_result {
    uint32_t struct_size;    /* = sizeof(hfpf_align_result), set by the caller */
    uint32_t iterations;
    uint32_t flags;          /* HFPF_ALIGN_* */
    uint32_t reserved;
    uint64_t rows_sampled;   /* the same in every iteration */
    uint64_t inliers;        /* of the last system evaluated */
    double rms;              /* sqrt(rr / inliers) of that system */
    double information[36];  /* its undamped J^T J, row-major, twist order (omega, tau) about the bounding box's centre */
    double pose[12];         /* refined pose, row-major [R|t], mesh frame -> fusion frame */
} hfpf_align_result;

#ifdef __cplusplus
static_assert(sizeof(hfpf_align_opts) == 88, "hfpf_align_opts is 88 bytes");
static_assert(sizeof(hfpf_align_result) == 424, "hfpf_align_result is 424 bytes");
#else
_Static_assert(sizeof(hfpf_align_opts) == 88, "hfpf_align_opts is 88 bytes");
_Static_assert(sizeof(hfpf_align_result) == 424, "hfpf_align_result is 424 bytes");
#endif

/* HFPF_OK if o passes the checks above that need no handle, else HFPF_ERR_BAD_ARG (host code; the node shell uses it too). */
int hfpf_check_align_opts(const hfpf_align_opts* o);
/* Mesh and pose in HOST memory (the mesh is uploaded once per call, as hfpf_compare_mesh uploads it). */
int hfpf_align_mesh(hfpf_handle* h, const hfpf_align_opts* o, const void* verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* tris,
                    uint64_t n_tris, const double* pose_3x4, hfpf_align_result* result);
/* The mesh is read in place from DEVICE memory (HBM); pose_3x4 and result are in host memory. */
int hfpf_align_mesh_device(hfpf_handle* h, const hfpf_align_opts* o, const void* dev_verts, uint64_t n_verts, uint32_t vertex_stride,
                           const uint32_t* dev_tris, uint64_t n_tris, const double* pose_3x4, hfpf_align_result* result);

/* ---- coverage of a triangle mesh by the fused model (no reference counterpart) --------------------------------------------------
 * hfpf_compare_mesh asks how far every scanned row is from the reference surface; a cover asks the other half of an inspection:
 * which parts of the reference surface have been scanned at all.  Every triangle is cut into sub-triangles no longer than
 * `spacing`, the centroid of each is one sample, and a sample is covered when the model has a row near it (and, with the normal
 * gate, one that faces the way the triangle does).  Everything is restatable from hfpf_extract's rows and hfpf_get_occupied's list
 * (tests/cover_ref.py).
 * Arithmetic: everything below is f64, one rounding per operation, left to right, never contracted, dot() as in the deviation
 *   section.
 * Mesh, pose, valid triangles: word for word those of the section "deviation of the fused model from a triangle mesh": verts,
 *   n_verts, vertex_stride, tris, n_tris, pose_3x4 from the mesh frame to the fusion frame; V kept in f64; triangle k is VALID iff
 *   its three indices are < n_verts, its nine transformed coordinates are finite and NN = dot(N, N) is finite and > 0.  The device
 *   rejects an index out of range before it loads anything through it.  Invalid triangles are skipped and counted; their record is
 *   all zero.
 * Subdivision: per valid triangle with ab = B - A, ac = C - A, bc = C - B:
 *   L2 = max(dot(ab,ab), max(dot(ac,ac), dot(bc,bc))); q = sqrt(L2) / spacing;
 *   n = 1 when !(q > 1); n = max_subdivision when q >= max_subdivision, and HFPF_COV_CAPPED is set iff q > max_subdivision (the
 *   samples are then coarser than asked); otherwise n = (uint32)ceil(q).
 *   The triangle is cut into its n^2 congruent sub-triangles (i, j, kind): kind 0 is upright, for 0 <= i, 0 <= j, i + j <= n - 1;
 *   kind 1 is inverted, for i + j <= n - 2.  Each contributes its centroid as one sample, which stands for area / n^2:
 *     v = (double)(3i + 1 + kind) / (double)(3n); w = (double)(3j + 1 + kind) / (double)(3n);
 *     S[a] = (A[a] + v*ab[a]) + w*ac[a]; p[a] = (float)S[a].
 *   Nothing below depends on the order of the samples.
 * Sample test: the sample's hit is the hfpf_query hit of the f32 point p under the identity pose with the call's radius, min_count
 *   and max_distance and without the z-clip (exactly how a mesh corner sample and a raycast sample are defined).  IN_BBOX is that
 *   hit's HFPF_QHIT_IN_BBOX.  With c = (N.x*nx + N.y*ny) + N.z*nz (nx, ny, nz the found row's f32 normal widened, N the triangle's)
 *   and s = sqrt(NN), the sample is COVERED iff the hit is HFPF_QHIT_FOUND and
 *     min_normal_dot == -2 (the gate is off), or c >= min_normal_dot * s, or HFPF_COVER_ABS_NORMAL is set and
 *     fabs(c) >= min_normal_dot * s.
 *   The gate inherits the rows' orientation, as the mesh, the raycast and the components do: a row's normal points to the side its
 *   points were seen from, so a reference mesh wound the other way needs HFPF_COVER_ABS_NORMAL (or the gate off).  A covered sample
 *   contributes distance = the hit's f32 distance.
 * Per triangle (hfpf_tri_coverage): n_samples = n^2; n_in_bbox, n_covered; flags; area = (float)area_d with area_d = 0.5 * s;
 *   max_distance = the largest covered sample's distance (0 without one; a max on the float's bits); sum_dist_q30 = the sum over
 *   covered samples of rint((double)distance * 2^30).
 * Summary: integer and max reductions only.  Per valid triangle ta = (uint64)rint(area_d * 2^40) and
 *   tc = (uint64)rint(((area_d * (double)n_covered) / (double)n_samples) * 2^40).  A triangle with !(area_d < 2^23) is HUGE
 *   (HFPF_COV_HUGE): it is sampled and recorded like any other, but adds nothing to the four area words.  Otherwise area_q40_lo adds
 *   ta & 0xFFFFFFFF, area_q40_hi adds ta >> 32, and covered_q40_lo / covered_q40_hi the same of tc; n_tris < 2^32 - 1 keeps every word
 *   below 2^64.  The area in m^2 is (hi * 2^32 + lo) / 2^40.  max_distance <= 1 keeps sum_dist_q30 below 2^62 for the 2^32 - 2
 *   samples allowed.
 * A call changes nothing on the handle except device_bytes (its scratch); host frames still waiting are launched first.  Rejected
 * with HFPF_ERR_BAD_ARG (the handle stays usable, nothing is written): what hfpf_check_cover_opts rejects (struct_size != sizeof,
 * flags beyond HFPF_COVER_ABS_NORMAL, reserved != 0, radius outside 1..4, max_subdivision outside 1..64, min_count NaN, max_distance
 * not finite, not > 0 or > 1, spacing not finite or not > 0, min_normal_dot not finite or outside [-2, 1]); every check
 * hfpf_compare_mesh makes on the mesh and the pose; a NULL cov or summary; for the device form verts or tris not 4-byte aligned.
 * n_tris = 0 returns HFPF_OK with *cov = NULL and a zero summary; an empty handle, or one before its first clean pass, returns
 * HFPF_OK with every valid triangle recorded and n_covered = 0.  More than 2^32 - 2 samples in total return HFPF_ERR_CAPACITY, the
 * message names the count, and the handle stays usable.  A handle with an RCCL communicator, or a failed handle, returns
 * HFPF_ERR_STATE as the other readers do. */
#define HFPF_COV_VALID 1u  /* hfpf_tri_coverage.flags: the triangle is valid (an invalid one has an all-zero record) */
#define HFPF_COV_CAPPED 2u /* q > max_subdivision: the samples are coarser than spacing */
#define HFPF_COV_HUGE 4u   /* !(area_d < 2^23): not part of the summary's area words */

#define HFPF_COVER_ABS_NORMAL 1u /* hfpf_cover_opts.flags: the normal gate also passes fabs(c) >= min_normal_dot * s */

typedef struct hfpf_cover_opts {
    uint32_t struct_size;        /* = sizeof(hfpf_cover_opts) */
    uint32_t flags;              /* HFPF_COVER_ABS_NORMAL or 0 */
    int32_t radius;              /* 1..4: the voxel window of the sample test */
    uint32_t max_subdivision;    /* 1..64: the largest n */
    double min_count;            /* rows with count < max(1, min_count) are no candidates */
    double max_distance;         /* metres, > 0 and <= 1: a row farther from a sample does not cover it */
    double spacing;              /* metres, > 0: the sub-triangles' longest edge is at most this (unless CAPPED) */
    double min_normal_dot;       /* -2 = gate off, else in (-2, 1]: the cosine between the triangle's and the row's normal */
    uint64_t reserved;           /* 0 */
} hfpf_cover_opts;

typedef struct hfpf_tri_coverage { /* 32 bytes, one per triangle */
    uint32_t n_samples;          /* n^2 */
    uint32_t n_in_bbox;          /* samples inside the bounding box */
    uint32_t n_covered;          /* samples covered */
    uint32_t flags;              /* HFPF_COV_* */
    float area;                  /* (float)(0.5 * sqrt(NN)), m^2 */
    float max_distance;          /* the largest covered sample's distance, 0 without one */
    int64_t sum_dist_q30;
} hfpf_tri_coverage;

typedef struct hfpf_coverage_summary { /* 96 bytes */
    uint64_t n_tris_valid;
    uint64_t n_tris_invalid;
    uint64_t n_tris_huge;
    uint64_t n_samples;
    uint64_t n_in_bbox;
    uint64_t n_covered;
    int64_t sum_dist_q30;
    uint64_t area_q40_lo, area_q40_hi;       /* the mesh's area: (hi * 2^32 + lo) / 2^40 m^2 */
    uint64_t covered_q40_lo, covered_q40_hi; /* the covered share of it, the same way */
    float max_distance;          /* the largest covered sample's distance, 0 without one */
    uint32_t pad;                /* 0 */
} hfpf_coverage_summary;

#ifdef __cplusplus
static_assert(sizeof(hfpf_cover_opts) == 56, "hfpf_cover_opts is 56 bytes");
static_assert(sizeof(hfpf_tri_coverage) == 32, "hfpf_tri_coverage is 32 bytes");
static_assert(sizeof(hfpf_coverage_summary) == 96, "hfpf_coverage_summary is 96 bytes");
#else
_Static_assert(sizeof(hfpf_cover_opts) == 56, "hfpf_cover_opts is 56 bytes");
_Static_assert(sizeof(hfpf_tri_coverage) == 32, "hfpf_tri_coverage is 32 bytes");
_Static_assert(sizeof(hfpf_coverage_summary) == 96, "hfpf_coverage_summary is 96 bytes");
#endif

/* HFPF_OK if o passes the checks above, else HFPF_ERR_BAD_ARG (host code, no handle; the node shell uses it too). */
int hfpf_check_cover_opts(const hfpf_cover_opts* o);
/* Mesh, pose and outputs in HOST memory (the mesh is uploaded once per call, as hfpf_compare_mesh uploads it): *cov holds n_tris
 * records and is freed by hfpf_free_coverage. */
int hfpf_cover_mesh(hfpf_handle* h, const hfpf_cover_opts* o, const void* verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* tris,
                    uint64_t n_tris, const double* pose_3x4, hfpf_tri_coverage** cov, hfpf_coverage_summary* summary);
void hfpf_free_coverage(hfpf_tri_coverage* cov);
/* The mesh is read in place from DEVICE memory (HBM); *dev_cov is a device array of n_tris records, freed by hfpf_device_free(h, p).
 * pose_3x4 and summary are in host memory. */
int hfpf_cover_mesh_device(hfpf_handle* h, const hfpf_cover_opts* o, const void* dev_verts, uint64_t n_verts, uint32_t vertex_stride,
                           const uint32_t* dev_tris, uint64_t n_tris, const double* pose_3x4, hfpf_tri_coverage** dev_cov,
                           hfpf_coverage_summary* summary);

/* ---- planning the next views: candidate poses scored by unscanned reference surface (no reference counterpart) -------------------
 * hfpf_cover_mesh says which parts of a reference mesh have not been scanned; a plan says where to move the sensor next.  Every
 * cover sample that is in the box and not covered is a TARGET; per candidate camera pose the call counts the targets that pose
 * would see -- in range, facing the camera and not hidden behind the reference surface (or, on request, the model) -- and a greedy
 * selection picks up to max_views poses by marginal gain.  Everything is restatable from hfpf_extract's rows and
 * hfpf_get_occupied's list (tests/plan_ref.py).
 * Arithmetic: everything below is f64, one rounding per operation, left to right, never contracted, unless stated otherwise.
 * Mesh, pose, valid triangles, subdivision, sample points, sample test: word for word those of the coverage section, driven by the
 *   embedded hfpf_cover_opts `cover`.  Per sample s of a valid triangle k that gives the f32 point p, the triangle's f64 normal N
 *   with NN = dot(N, N) and s_k = sqrt(NN), IN_BBOX and COVERED.  A sample is a TARGET iff it is IN_BBOX and not COVERED.  The call
 *   also returns the hfpf_coverage_summary hfpf_cover_mesh would return for the same arguments, byte for byte.
 * Weight: w_s = (uint64)rint((area_d / (double)n_samples) * 2^40), and 0 for a triangle with HFPF_COV_HUGE.  When the summary's area
 *   hi * 2^32 + lo is >= 2^62 the call returns HFPF_ERR_CAPACITY (the handle stays usable): every sum below stays under 2^63.
 * View: the embedded hfpf_render_opts `view`, checked as hfpf_render checks it, supplies width, height, the intrinsics, z_near,
 *   z_far, min_count, splat_radius, max_splat_radius and HFPF_RENDER_CULL_BACKFACES (HFPF_RENDER_WORLD_NORMALS has no effect).
 *   occluder_near, 0 < occluder_near <= z_near: a surface nearer than the sensor's minimum range still blocks a ray.  poses holds
 *   n_views * 12 f64 in HOST memory, row-major [R|t], camera -> fusion frame.
 * Projection of a point into view v: the lines of the render section with (x, y, z) = p widened: dx, dy, dz, xc, yc, zc, u, v,
 *   pu, pv and depth32 = (float)zc.
 * Occluders of view v: every sample of a valid triangle whose p is finite, in the box or not, target or not, with
 *   occluder_near < zc < z_far and |u|, |v| < 2^30, splat over (pu + i, pv + j), |i|, |j| <= r, inside the image; r = splat_radius,
 *   or for -1: min(max_splat_radius, floor(((0.5 * cover.spacing) * max(fx, fy)) / zc)).  With HFPF_PLAN_MODEL_OCCLUDES also the rows
 *   hfpf_render would draw with `view`, z_near replaced by occluder_near, with their own splat rule (res in the auto radius) and
 *   the back-face cull when the view asks for it (the cull applies to the rows only).  zmin(v, pixel) = the smallest depth32 of all
 *   occluder candidates of that pixel: a minimum, independent of any order.
 * Target classes in view v: c = -((N.x*dx + N.y*dy) + N.z*dz), d2 = (dx*dx + dy*dy) + dz*dz.
 *   IN_VIEW iff z_near < zc < z_far, |u|, |v| < 2^30 and (pu, pv) is inside the image.
 *   FACING iff IN_VIEW and: min_cos < 0 (the gate is off), or c > 0 && c*c >= ((min_cos*min_cos) * NN) * d2, or
 *     HFPF_PLAN_TWO_SIDED is set and c*c >= ((min_cos*min_cos) * NN) * d2.
 *   VISIBLE iff FACING and (double)depth32 - (double)zmin(v, (pu, pv)) <= tolerance + slope * zc.  A target splats into its own
 *     pixel, so zmin <= depth32 always.
 * Per view (hfpf_view_score): n_in_view, n_facing, n_visible count targets; visible_q40 = the sum of w_s over VISIBLE targets;
 *   rank, gain_q40, gain_samples from the selection.
 * Greedy selection: R_0 = all targets.  Round k = 0 .. max_views - 1, over the views not yet selected: G(v) = the sum of w_s over
 *   R_k n VIS(v), C(v) = that set's size.  The best view has the largest G; ties go to the larger C, then to the smaller view index.
 *   The selection stops when G(best) < max(1, min_gain_q40).  Otherwise rank[best] = k, gain_q40 = G, gain_samples = C and
 *   R_{k+1} = R_k \ VIS(best).  Unselected views keep rank = -1 and zero gains.
 * Per triangle (hfpf_tri_plan, optional): n_targets; n_reachable = targets VISIBLE from at least one candidate; n_planned = targets
 *   VISIBLE from at least one selected view; flags = the cover flags (an invalid triangle has an all-zero record).
 * Summary (hfpf_plan_summary): the coverage summary; n_views, n_selected; n_targets, n_reachable, n_planned; target_q40,
 *   reachable_q40, planned_q40 = the sums of w_s over those sets.  Everything is an integer sum or a minimum: nothing depends on
 *   scheduling or on how the views are split into depth-buffer chunks (HFPF_PLAN_CHUNK=1..64 in the environment forces the views per
 *   chunk, for tests).
 * A call changes nothing on the handle except device_bytes (its scratch); host frames still waiting are launched first.  Rejected
 * with HFPF_ERR_BAD_ARG (the handle stays usable, nothing is written): what hfpf_check_plan_opts rejects (struct_size != sizeof,
 * flags beyond the two below, reserved fields != 0, everything hfpf_check_cover_opts rejects in `cover`, everything hfpf_render
 * rejects in `view`, occluder_near not finite or outside (0, z_near], min_cos not finite or outside [-1, 1], tolerance not finite
 * or outside (0, 1], slope not finite or outside [0, 1], max_views outside 1..256); n_views > 4096; NULL or non-finite poses with
 * n_views > 0; a NULL scores or summary; the mesh checks of hfpf_compare_mesh; for the device form verts or tris not 4-byte
 * aligned.  More than 2^35 (target, view) pairs return HFPF_ERR_CAPACITY, the message names both numbers, and the handle stays
 * usable.  n_views = 0 gives the coverage summary and a zero plan; n_tris = 0 gives all zero (n_views and the ranks of -1 apart) and a
 * NULL plan.  A handle before
 * its first clean pass makes every in-box sample a target.  A handle with an RCCL communicator, or a failed handle, returns
 * HFPF_ERR_STATE as the other readers do. */
#define HFPF_PLAN_TWO_SIDED 1u      /* hfpf_plan_opts.flags: the facing gate passes either side of a triangle */
#define HFPF_PLAN_MODEL_OCCLUDES 2u /* the rows hfpf_render would draw occlude too */

typedef struct hfpf_plan_opts {
    uint32_t struct_size;    /* = sizeof(hfpf_plan_opts) */
    uint32_t flags;          /* HFPF_PLAN_* */
    hfpf_cover_opts cover;   /* what a target is */
    hfpf_render_opts view;   /* the sensor at every candidate pose */
    double occluder_near;    /* metres, in (0, view.z_near] */
    double min_cos;          /* < 0 = gate off, else the smallest cosine between the triangle's normal and the ray to the camera */
    double tolerance, slope; /* a target is visible when it lies at most tolerance + slope * zc behind the pixel's nearest occluder */
    uint64_t min_gain_q40;   /* the selection stops below max(1, min_gain_q40) */
    uint32_t max_views;      /* 1..256 */
    uint32_t reserved0;      /* 0 */
    uint64_t reserved;       /* 0 */
} hfpf_plan_opts;

typedef struct hfpf_view_score { /* 40 bytes, one per candidate view */
    int32_t rank;            /* the round that selected the view, -1 = not selected */
    uint32_t n_in_view, n_facing, n_visible;
    uint64_t visible_q40;    /* visible target area: / 2^40 m^2 */
    uint64_t gain_q40, gain_samples; /* what the view added when it was selected */
} hfpf_view_score;

typedef struct hfpf_tri_plan { /* 16 bytes, one per triangle */
    uint32_t n_targets, n_reachable, n_planned;
    uint32_t flags;          /* HFPF_COV_* */
} hfpf_tri_plan;

typedef struct hfpf_plan_summary { /* 152 bytes */
    hfpf_coverage_summary coverage;
    uint32_t n_views, n_selected;
    uint64_t n_targets, n_reachable, n_planned;
    uint64_t target_q40, reachable_q40, planned_q40;
} hfpf_plan_summary;

#ifdef __cplusplus
static_assert(sizeof(hfpf_plan_opts) == 208, "hfpf_plan_opts is 208 bytes");
static_assert(sizeof(hfpf_view_score) == 40, "hfpf_view_score is 40 bytes");
static_assert(sizeof(hfpf_tri_plan) == 16, "hfpf_tri_plan is 16 bytes");
static_assert(sizeof(hfpf_plan_summary) == 152, "hfpf_plan_summary is 152 bytes");
#else
_Static_assert(sizeof(hfpf_plan_opts) == 208, "hfpf_plan_opts is 208 bytes");
_Static_assert(sizeof(hfpf_view_score) == 40, "hfpf_view_score is 40 bytes");
_Static_assert(sizeof(hfpf_tri_plan) == 16, "hfpf_tri_plan is 16 bytes");
_Static_assert(sizeof(hfpf_plan_summary) == 152, "hfpf_plan_summary is 152 bytes");
#endif

/* HFPF_OK if o passes the checks above, else HFPF_ERR_BAD_ARG (host code, no handle; the node shell uses it too). */
int hfpf_check_plan_opts(const hfpf_plan_opts* o);
/* Mesh, pose, poses and outputs in HOST memory: scores holds n_views records (the caller's array); *plan, when plan is not NULL,
 * holds n_tris records and is freed by hfpf_free_plan. */
int hfpf_plan_views(hfpf_handle* h, const hfpf_plan_opts* o, const void* verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* tris,
                    uint64_t n_tris, const double* pose_3x4, const double* poses, uint32_t n_views, hfpf_view_score* scores, hfpf_tri_plan** plan,
                    hfpf_plan_summary* summary);
void hfpf_free_plan(hfpf_tri_plan* plan);
/* The mesh is read in place from DEVICE memory (HBM); *dev_plan is a device array of n_tris records, freed by hfpf_device_free(h, p).
 * pose_3x4, poses, scores and summary are in host memory. */
int hfpf_plan_views_device(hfpf_handle* h, const hfpf_plan_opts* o, const void* dev_verts, uint64_t n_verts, uint32_t vertex_stride,
                           const uint32_t* dev_tris, uint64_t n_tris, const double* pose_3x4, const double* poses, uint32_t n_views,
                           hfpf_view_score* scores, hfpf_tri_plan** dev_plan, hfpf_plan_summary* summary);

/* ---- planar sections of a triangle mesh: contours, lengths and areas (no reference counterpart) -------------------------------------
 * The read-outs above measure the model against a reference mesh; a section measures geometry on its own terms: the profile of a
 * mesh in a given plane, its length, the area it encloses, whether it is closed.  The mesh is any mesh -- a CAD model, or the
 * model's own (hfpf_extract_mesh_device leaves it in HBM, and the device form cuts it there).  Every output is an integer
 * reduction, a sort rank or a union-find label: nothing depends on scheduling.  Everything is restatable from the arguments alone
 * (tests/section_ref.py); the fused model plays no part.
 * Arithmetic: everything below is f64, one rounding per operation, left to right, never contracted.
 *   dot(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z; cross(u, v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x), written
 *   out as N is in the deviation section; vector sums and differences per component.
 * Mesh, pose, valid triangles: word for word those of the section "deviation of the fused model from a triangle mesh": verts,
 *   n_verts, vertex_stride, tris, n_tris, pose_3x4 from the mesh frame to the fusion frame; V kept in f64; triangle k is VALID iff
 *   its three indices are < n_verts, its nine transformed coordinates are finite and NN = dot(N, N) is finite and > 0.  The device
 *   rejects an index out of range before it loads anything through it.  A valid triangle is IN RANGE iff each of its nine
 *   coordinates has |V[a] - c[a]| < 32 (metres: track's headroom rule), c[a] = (bbox_min[a] + bbox_max[a]) * 0.5 the centre
 *   hfpf_align_mesh uses.  Invalid triangles and valid triangles that are not in range (FAR) are skipped and counted:
 *   n_tris_invalid, n_tris_far; n_tris_valid counts the valid ones, far or not.
 * Planes: n_planes * 4 f64 in HOST memory, (n.x, n.y, n.z, d) per plane, in the fusion frame; n need not be a unit vector.  For
 *   vertex i and plane j: s = dot(n, V_i) - d.  The vertex is INSIDE iff s < 0 (the rule of the mesh and of raycast).  There is no
 *   "on the plane" case: s == 0 is outside.
 * Crossing: an in-range triangle crosses plane j iff its three vertices are not all inside and not all outside.  Exactly one
 *   vertex L (position 0, 1 or 2 in the triangle) then differs from the other two; with next(L) and prev(L) the positions after
 *   and before it in the triangle's cyclic index order, the crossing lies on the edges (L, next(L)) and (prev(L), L).
 * Points: a point is identified by (plane, va, vb), va < vb the vertex indices of the edge (a crossing edge has two distinct
 *   indices: its ends lie on different sides).  t = s_va / (s_va - s_vb); P[a] = V_va[a] + t * (V_vb[a] - V_va[a]): always from the
 *   lower index to the higher, so the triangles that share an edge share the point bit for bit.  The points are numbered 0.. in
 *   ascending (plane, va, vb) order.  Welding follows the mesh's indices: two vertices with equal coordinates but different indices
 *   are NOT merged (a triangle soup gives one open contour per segment).  n_verts <= 2^26, so that (plane: 12 bits | va: 26 | vb:
 *   26) is one 64-bit sort key.
 * Segments: one per (crossing triangle, plane), in ascending (plane, triangle) order.  If L is INSIDE the segment runs from the
 *   point on (prev(L), L) to the point on (L, next(L)); if L is outside, the other way.  That is the direction of cross(n, N), N
 *   the triangle's winding normal: the section of a closed, outward-wound mesh runs counter-clockwise seen from the side n points
 *   to, and its area below is positive.  A plane through vertices gives zero-length segments; they are kept, there is no special
 *   case.
 * Contours: the connected components of the points under "joined by a segment".  A contour's representative is its smallest
 *   point; contours are numbered by ascending representative, which groups them by plane.  Per point n_out counts the segments that
 *   start there and n_in those that end there, each saturated at 65535.  A contour is CLOSED iff every point of it has n_in == 1
 *   and n_out == 1; BRANCHED iff some point of it has n_in > 1 or n_out > 1 (a non-manifold edge, or inconsistent winding);
 *   n_ends = its points with n_in + n_out == 1.
 * Length and area: order-free fixed-point sums over the contour's segments, P0 and P1 the f64 points of p0 and p1:
 *     e = P1 - P0;                       length_q32 += (int64)rint(sqrt(dot(e, e)) * 2^32)
 *     a = P0 - Pr; b = P1 - Pr;          area_q28   += (int64)rint((0.5 * dot(U, cross(a, b))) * 2^28)
 *   with nn = dot(n, n), U[a] = n[a] / sqrt(nn) and Pr the representative's f64 point.  The area is meaningful for a closed contour
 *   and reported for all; its sign is only as good as the mesh's winding.  Headroom: in-range coordinates keep a segment below 2^7 m
 *   and an area term below 2^13 m^2, so the at most 2^20 segments a plane may have keep either sum below 2^62.
 * Records: hfpf_section_point (x, y, z = (float)P per axis; ends = n_out | n_in << 16), hfpf_section_segment, hfpf_section_contour
 *   (first_point = the representative), one hfpf_section_plane per plane (first_segment, first_point and first_contour are the
 *   totals of the planes before it, also for a plane that has none; length_q32 over all its contours, area_q28 over its CLOSED
 *   contours only) and one hfpf_section_summary.  Reserved words are 0.
 * A call needs no fused model (an empty handle works) and changes nothing on the handle except device_bytes (its scratch); it
 * returns when its outputs are complete.  Rejected with HFPF_ERR_BAD_ARG (the handle stays usable, nothing is written), all of it
 * before anything is read through a mesh pointer: what hfpf_check_section_opts rejects (struct_size != sizeof, flags or reserved != 0);
 * every check hfpf_compare_mesh makes on the mesh and the pose; n_verts > 2^26; n_planes > 4096; NULL planes with n_planes > 0; a
 * plane with a non-finite value or with nn not finite or not > 0; a NULL output pointer (points, n_points, segments, n_segments,
 * contours, n_contours, summary; plane_recs with n_planes > 0); for the device form verts or tris not 4-byte aligned.  n_planes = 0
 * or n_tris = 0 returns HFPF_OK with NULL arrays, zeroed plane records and the triangle counts.  A plane with more than 2^20
 * segments, or more than 2^31 - 1 segments in all, returns HFPF_ERR_CAPACITY; the message names the plane and its count (or the
 * total), nothing is written, and the handle stays usable.  A handle with an RCCL communicator, or a failed handle, returns
 * HFPF_ERR_STATE as the other mesh readers do.
 * LIMITATION: sections of the model's own mesh are open wherever the scan is: the CLOSED flags then say where the scan has holes. */
#define HFPF_SECTION_CLOSED 1u   /* hfpf_section_contour.flags: every point has n_in == 1 and n_out == 1 */
#define HFPF_SECTION_BRANCHED 2u /* some point has n_in > 1 or n_out > 1 */
#define HFPF_SECTION_MAX_PLANES 4096u
#define HFPF_SECTION_MAX_PLANE_SEGMENTS (1u << 20)

typedef struct hfpf_section_opts {
    uint32_t struct_size;        /* = sizeof(hfpf_section_opts) */
    uint32_t flags;              /* 0 */
    uint64_t reserved;           /* 0 */
} hfpf_section_opts;

typedef struct hfpf_section_point { /* 32 bytes */
    float x, y, z;               /* (float)P */
    uint32_t plane;
    uint32_t va, vb;             /* the edge's vertex indices, va < vb */
    uint32_t contour;
    uint32_t ends;               /* n_out | n_in << 16 */
} hfpf_section_point;

typedef struct hfpf_section_segment { /* 16 bytes */
    uint32_t p0, p1;             /* from point p0 to point p1 */
    uint32_t tri;
    uint32_t contour;
} hfpf_section_segment;

typedef struct hfpf_section_contour { /* 48 bytes */
    uint32_t plane;
    uint32_t first_point;        /* the representative */
    uint32_t n_points, n_segments, n_ends;
    uint32_t flags;              /* HFPF_SECTION_* */
    int64_t length_q32;          /* / 2^32 m */
    int64_t area_q28;            /* / 2^28 m^2 */
    uint64_t reserved;           /* 0 */
} hfpf_section_contour;

typedef struct hfpf_section_plane { /* 64 bytes, one per plane */
    uint32_t first_segment, n_segments;
    uint32_t first_point, n_points;
    uint32_t first_contour, n_contours;
    uint32_t n_closed, n_branched;
    int64_t length_q32;          /* over all its contours */
    int64_t area_q28;            /* over its closed contours */
    uint64_t reserved[2];        /* 0 */
} hfpf_section_plane;

typedef struct hfpf_section_summary { /* 64 bytes */
    uint64_t n_tris_valid, n_tris_invalid, n_tris_far;
    uint64_t n_segments, n_points, n_contours, n_closed;
    uint64_t reserved;           /* 0 */
} hfpf_section_summary;

#ifdef __cplusplus
static_assert(sizeof(hfpf_section_opts) == 16, "hfpf_section_opts is 16 bytes");
static_assert(sizeof(hfpf_section_point) == 32, "hfpf_section_point is 32 bytes");
static_assert(sizeof(hfpf_section_segment) == 16, "hfpf_section_segment is 16 bytes");
static_assert(sizeof(hfpf_section_contour) == 48, "hfpf_section_contour is 48 bytes");
static_assert(sizeof(hfpf_section_plane) == 64, "hfpf_section_plane is 64 bytes");
static_assert(sizeof(hfpf_section_summary) == 64, "hfpf_section_summary is 64 bytes");
#else
_Static_assert(sizeof(hfpf_section_opts) == 16, "hfpf_section_opts is 16 bytes");
_Static_assert(sizeof(hfpf_section_point) == 32, "hfpf_section_point is 32 bytes");
_Static_assert(sizeof(hfpf_section_segment) == 16, "hfpf_section_segment is 16 bytes");
_Static_assert(sizeof(hfpf_section_contour) == 48, "hfpf_section_contour is 48 bytes");
_Static_assert(sizeof(hfpf_section_plane) == 64, "hfpf_section_plane is 64 bytes");
_Static_assert(sizeof(hfpf_section_summary) == 64, "hfpf_section_summary is 64 bytes");
#endif

/* HFPF_OK if o passes the checks above, else HFPF_ERR_BAD_ARG (host code, no handle; the node shell uses it too). */
int hfpf_check_section_opts(const hfpf_section_opts* o);
/* Mesh, pose, planes and outputs in HOST memory (the mesh is uploaded once per call, as hfpf_compare_mesh uploads it): *points,
 * *segments and *contours hold *n_points, *n_segments and *n_contours records and are freed by hfpf_free_section; plane_recs is the
 * caller's array of n_planes records. */
int hfpf_section_mesh(hfpf_handle* h, const hfpf_section_opts* o, const void* verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* tris,
                      uint64_t n_tris, const double* pose_3x4, const double* planes, uint32_t n_planes, hfpf_section_point** points, uint64_t* n_points,
                      hfpf_section_segment** segments, uint64_t* n_segments, hfpf_section_contour** contours, uint64_t* n_contours,
                      hfpf_section_plane* plane_recs, hfpf_section_summary* summary);
void hfpf_free_section(hfpf_section_point* points, hfpf_section_segment* segments, hfpf_section_contour* contours);
/* The mesh is read in place from DEVICE memory (HBM); *dev_points, *dev_segments and *dev_contours are device arrays, each freed by
 * hfpf_device_free(h, p).  pose_3x4, planes, plane_recs and summary are in host memory. */
int hfpf_section_mesh_device(hfpf_handle* h, const hfpf_section_opts* o, const void* dev_verts, uint64_t n_verts, uint32_t vertex_stride,
                             const uint32_t* dev_tris, uint64_t n_tris, const double* pose_3x4, const double* planes, uint32_t n_planes,
                             hfpf_section_point** dev_points, uint64_t* n_points, hfpf_section_segment** dev_segments, uint64_t* n_segments,
                             hfpf_section_contour** dev_contours, uint64_t* n_contours, hfpf_section_plane* plane_recs,
                             hfpf_section_summary* summary);

/* ---- open edges of a triangle mesh: boundary loops, shells, watertightness, area and volume (no reference counterpart) ----------------
 * The first questions put to a scanned mesh: is it closed; if not, where are the holes and how long are their rims; if it is, what
 * area and volume does it enclose; is it consistently wound.  A section answers them only in the planes the caller happened to
 * choose; this read-out answers them for the whole mesh.  The mesh is any mesh, the model's own included (hfpf_extract_mesh_device
 * leaves it in HBM, and the device form reads it there).  Every output is an integer reduction, a sort rank or a union-find label:
 * nothing depends on scheduling, and everything is restatable from the arguments alone (tests/topology_ref.py); the fused model
 * plays no part.
 * Arithmetic: f64, one rounding per operation, left to right, never contracted; dot, cross, N and NN as the section and deviation
 *   texts above define them.
 * Mesh, pose, VALID, IN RANGE and FAR triangles: word for word those of the section "planar sections of a triangle mesh", the centre
 *   c and the 32 m rule included; the device rejects an index out of range before it loads anything through it.  Invalid and far
 *   triangles are skipped and counted (n_tris_invalid, n_tris_far; n_tris_valid counts the valid ones, far or not).  A USED triangle
 *   is valid and in range; its three indices are distinct (a repeated one gives NN = 0).  n_verts <= 2^26 and 3 * n_tris < 2^32.
 * Half-edges: used triangle k with the indices (i0, i1, i2) gives the half-edges 3k + c from i_c to i_(c+1 mod 3), c = 0, 1, 2.  The
 *   EDGE of a half-edge is (va, vb) = (min, max) of its two indices; the half-edge is FORWARD iff i_c < i_(c+1).  Welding follows the
 *   mesh's indices, as everywhere else: two vertices with equal coordinates but different indices are NOT merged, and a triangle soup
 *   is all boundary.
 * Edges: the distinct (va, vb), numbered in ascending (va, vb) order.  n_fwd and n_bwd count an edge's forward and backward
 *   half-edges (each saturated at 65535 in the record, exact for the classification):
 *     INTERIOR     n_fwd == 1 and n_bwd == 1           BOUNDARY   n_fwd + n_bwd == 1
 *     NONMANIFOLD  n_fwd + n_bwd >= 3                  MISWOUND   n_fwd + n_bwd == 2, both in the same direction
 *   (a triangle listed twice therefore shows as three MISWOUND edges).
 * Shells: the connected components of the vertices of used triangles under "joined by a used triangle".  A shell's representative
 *   is its smallest vertex index; shells are numbered by ascending representative; a vertex of no used triangle is in no shell.  Per
 *   shell: n_verts, n_tris, n_edges, n_boundary, n_nonmanifold, n_miswound, n_loops; flags OPEN (n_boundary > 0), NONMANIFOLD
 *   (n_nonmanifold > 0), MISWOUND (n_miswound > 0) and WATERTIGHT iff all three counts are 0.  With Pr the f64 point of the
 *   representative and P0, P1, P2 those of a triangle's indices, over the shell's used triangles:
 *     area_q32   += (int64)rint((0.5 * sqrt(NN)) * 2^32)
 *     a = P0 - Pr; b = P1 - Pr; c = P2 - Pr;    volume_q40 += (int64)rint((dot(a, cross(b, c)) / 6.0) * 2^40)
 *   The volume is reported for every shell and meaningful for a WATERTIGHT one: positive when the shell is wound outwards.
 *   In-range coordinates keep a term below 2^16 m^3, so each fits an int64; the sums are two's-complement and wrap, and are right
 *   whenever the true total fits.
 * Loops: the connected components of the vertices of BOUNDARY edges under "joined by a boundary edge".  A loop's representative
 *   is its smallest vertex index; loops are numbered by ascending representative.  A boundary edge runs from p0 to p1 as its one
 *   half-edge runs (with its triangle's winding).  Per boundary vertex n_out counts the boundary edges that start there and n_in
 *   those that end there.  A loop is CLOSED iff every vertex of it has n_in == 1 and n_out == 1; BRANCHED iff some vertex has
 *   n_in > 1 or n_out > 1 (two holes that touch in a vertex, or mixed winding); n_ends = its vertices with n_in + n_out == 1;
 *   shell = the shell of the representative (all of a loop's vertices share it).  Over the loop's edges, P0 and P1 the f64 points
 *   of p0 and p1 and Pr the representative's:
 *     e = P1 - P0;                    length_q32  += (int64)rint(sqrt(dot(e, e)) * 2^32)
 *     X = cross(P0 - Pr, P1 - Pr);    area_q28[k] += (int64)rint((0.5 * X[k]) * 2^28), k = 0, 1, 2: the loop's vector area
 *   The rim of a hole in an outward-wound surface runs clockwise seen from outside: its vector area points against the surface
 *   normal.  The outer rim of a patch points along it; a lone triangle's loop has 0.5 * N.
 * Records: one hfpf_topology_edge per edge that is NOT interior, in ascending (va, vb) order (p0, p1 = the half-edge's direction
 *   for a BOUNDARY edge, (va, vb) otherwise; tri = the triangle of the edge's smallest half-edge id; uses = n_fwd | n_bwd << 16;
 *   loop = 0xFFFFFFFF unless BOUNDARY); one hfpf_topology_loop per loop, one hfpf_topology_shell per shell; optionally tri_shell,
 *   one uint32 per triangle: its shell, or 0xFFFFFFFF for a skipped one (not produced when its pointer is NULL; it is what lets a
 *   caller drop small shells); one hfpf_topology_summary.  Reserved words are 0.  An array pointer is NULL exactly when its count
 *   is 0 (tri_shell: n_tris).
 * A call needs no fused model (an empty handle works) and changes nothing on the handle except device_bytes (its scratch); it
 * returns when its outputs are complete.  Rejected with HFPF_ERR_BAD_ARG (the handle stays usable, nothing is written), all of it
 * before anything is read through a mesh pointer: what hfpf_check_topology_opts rejects (struct_size != sizeof, flags or
 * reserved != 0); every check hfpf_compare_mesh makes on the mesh and the pose; n_verts > 2^26; 3 * n_tris >= 2^32; a NULL output
 * pointer (edges, n_edges, loops, n_loops, shells, n_shells, summary); for the device form verts or tris not 4-byte aligned.
 * n_tris = 0 returns HFPF_OK with NULL arrays and a zeroed summary.  A handle with an RCCL communicator, or a failed handle, returns
 * HFPF_ERR_STATE as the other mesh readers do.
 * LIMITATION: welding is by index only.  Not provided: hole filling, repair, merging of coincident vertices. */
#define HFPF_TOPOLOGY_BOUNDARY 1u    /* hfpf_topology_edge.kind */
#define HFPF_TOPOLOGY_NONMANIFOLD 2u
#define HFPF_TOPOLOGY_MISWOUND 3u
#define HFPF_TOPOLOGY_LOOP_CLOSED 1u   /* hfpf_topology_loop.flags: every vertex has n_in == 1 and n_out == 1 */
#define HFPF_TOPOLOGY_LOOP_BRANCHED 2u /* some vertex has n_in > 1 or n_out > 1 */
#define HFPF_TOPOLOGY_SHELL_OPEN 1u        /* hfpf_topology_shell.flags: n_boundary > 0 */
#define HFPF_TOPOLOGY_SHELL_NONMANIFOLD 2u /* n_nonmanifold > 0 */
#define HFPF_TOPOLOGY_SHELL_MISWOUND 4u    /* n_miswound > 0 */
#define HFPF_TOPOLOGY_SHELL_WATERTIGHT 8u  /* none of the three */
#define HFPF_TOPOLOGY_NONE 0xFFFFFFFFu     /* no loop (hfpf_topology_edge.loop), no shell (tri_shell) */
#define HFPF_TOPOLOGY_MAX_VERTS (1u << 26)

typedef struct hfpf_topology_opts {
    uint32_t struct_size;        /* = sizeof(hfpf_topology_opts) */
    uint32_t flags;              /* 0 */
    uint64_t reserved;           /* 0 */
} hfpf_topology_opts;

typedef struct hfpf_topology_edge { /* 32 bytes, one per edge that is not INTERIOR */
    uint32_t p0, p1;             /* the half-edge's direction for BOUNDARY, (va, vb) otherwise */
    uint32_t tri;                /* the triangle of the edge's smallest half-edge id */
    uint32_t kind;               /* HFPF_TOPOLOGY_BOUNDARY, _NONMANIFOLD or _MISWOUND */
    uint32_t uses;               /* n_fwd | n_bwd << 16, each saturated at 65535 */
    uint32_t loop;               /* HFPF_TOPOLOGY_NONE unless BOUNDARY */
    uint32_t shell;
    uint32_t reserved;           /* 0 */
} hfpf_topology_edge;

typedef struct hfpf_topology_loop { /* 64 bytes */
    uint32_t first_vertex;       /* the representative */
    uint32_t n_verts, n_edges, n_ends;
    uint32_t flags;              /* HFPF_TOPOLOGY_LOOP_* */
    uint32_t shell;
    int64_t length_q32;          /* / 2^32 m */
    int64_t area_q28[3];         /* / 2^28 m^2: the vector area */
    uint64_t reserved;           /* 0 */
} hfpf_topology_loop;

typedef struct hfpf_topology_shell { /* 64 bytes */
    uint32_t first_vertex;       /* the representative */
    uint32_t n_verts, n_tris;
    uint32_t flags;              /* HFPF_TOPOLOGY_SHELL_* */
    uint32_t n_edges, n_boundary, n_nonmanifold, n_miswound;
    uint32_t n_loops;
    uint32_t reserved0;          /* 0 */
    int64_t area_q32;            /* / 2^32 m^2 */
    int64_t volume_q40;          /* / 2^40 m^3 */
    uint64_t reserved;           /* 0 */
} hfpf_topology_shell;

typedef struct hfpf_topology_summary { /* 128 bytes */
    uint64_t n_tris_valid, n_tris_invalid, n_tris_far;
    uint64_t n_verts_used;
    uint64_t n_edges, n_interior, n_boundary, n_nonmanifold, n_miswound;
    uint64_t n_loops, n_closed_loops;
    uint64_t n_shells, n_watertight;
    uint64_t reserved[3];        /* 0 */
} hfpf_topology_summary;

#ifdef __cplusplus
static_assert(sizeof(hfpf_topology_opts) == 16, "hfpf_topology_opts is 16 bytes");
static_assert(sizeof(hfpf_topology_edge) == 32, "hfpf_topology_edge is 32 bytes");
static_assert(sizeof(hfpf_topology_loop) == 64, "hfpf_topology_loop is 64 bytes");
static_assert(sizeof(hfpf_topology_shell) == 64, "hfpf_topology_shell is 64 bytes");
static_assert(sizeof(hfpf_topology_summary) == 128, "hfpf_topology_summary is 128 bytes");
#else
_Static_assert(sizeof(hfpf_topology_opts) == 16, "hfpf_topology_opts is 16 bytes");
_Static_assert(sizeof(hfpf_topology_edge) == 32, "hfpf_topology_edge is 32 bytes");
_Static_assert(sizeof(hfpf_topology_loop) == 64, "hfpf_topology_loop is 64 bytes");
_Static_assert(sizeof(hfpf_topology_shell) == 64, "hfpf_topology_shell is 64 bytes");
_Static_assert(sizeof(hfpf_topology_summary) == 128, "hfpf_topology_summary is 128 bytes");
#endif

/* HFPF_OK if o passes the checks above, else HFPF_ERR_BAD_ARG (host code, no handle; the node shell uses it too). */
int hfpf_check_topology_opts(const hfpf_topology_opts* o);
/* Mesh, pose and outputs in HOST memory (the mesh is uploaded once per call, as hfpf_compare_mesh uploads it): *edges, *loops and
 * *shells hold *n_edges, *n_loops and *n_shells records, *tri_shell (tri_shell may be NULL) n_tris words; hfpf_free_topology frees
 * the four. */
int hfpf_mesh_topology(hfpf_handle* h, const hfpf_topology_opts* o, const void* verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* tris,
                       uint64_t n_tris, const double* pose_3x4, hfpf_topology_edge** edges, uint64_t* n_edges, hfpf_topology_loop** loops, uint64_t* n_loops,
                       hfpf_topology_shell** shells, uint64_t* n_shells, uint32_t** tri_shell, hfpf_topology_summary* summary);
void hfpf_free_topology(hfpf_topology_edge* edges, hfpf_topology_loop* loops, hfpf_topology_shell* shells, uint32_t* tri_shell);
/* The mesh is read in place from DEVICE memory (HBM); *dev_edges, *dev_loops, *dev_shells and *dev_tri_shell are device arrays,
 * each freed by hfpf_device_free(h, p).  pose_3x4 and summary are in host memory. */
int hfpf_mesh_topology_device(hfpf_handle* h, const hfpf_topology_opts* o, const void* dev_verts, uint64_t n_verts, uint32_t vertex_stride,
                              const uint32_t* dev_tris, uint64_t n_tris, const double* pose_3x4, hfpf_topology_edge** dev_edges, uint64_t* n_edges,
                              hfpf_topology_loop** dev_loops, uint64_t* n_loops, hfpf_topology_shell** dev_shells, uint64_t* n_shells,
                              uint32_t** dev_tri_shell, hfpf_topology_summary* summary);

/* ---- rows that later depth frames see through (the inverse of hfpf_render; no reference counterpart) ----------------------------
 * An occupancy grid keeps a voxel that was occupied once: a hand that crossed the view, a part that was moved, a slab of flying
 * pixels that passed the gate.  min_count cannot drop them when they were seen for many frames, hfpf_extract_components cannot when
 * they touch the surface.  What tells them apart is that depth frames look straight through them: this read-out gathers, per
 * (row, frame), the depth pixel the row projects onto and counts what it says.  Everything is restatable from
 * hfpf_extract_filtered's rows (tests/consistency_ref.py).
 * Arithmetic: everything below is f64, one rounding per operation, left to right, never contracted, unless stated otherwise.
 * Row set: the rows hfpf_extract_filtered would return at this point of the call sequence with the same min_count (0 keeps all), in
 *   lexicographic (ix, iy, iz) order; host frames still waiting are launched first.  Row j has f32 (x, y, z) and normal (nx, ny, nz),
 *   widened to f64.
 * Frames: n_frames depth images of ONE descriptor desc, frame f's image f * depth_frame_stride bytes behind `depth`; poses holds
 *   n_frames * 12 f64, row-major [R|t], camera -> fusion frame (the integrate convention).  desc is checked exactly as hfpf_query_depth
 *   checks it (colour fields included; no colour image is read).
 * Projection of row j into frame f, T = pose f (the lines of the render contract):
 *   dx = (double)x - T[3], dy = (double)y - T[7], dz = (double)z - T[11]
 *   xc = (T[0]*dx + T[4]*dy) + T[8]*dz,  yc = (T[1]*dx + T[5]*dy) + T[9]*dz,  zc = (T[2]*dx + T[6]*dy) + T[10]*dz
 *   u = (xc / zc) * fx + cx,  v = (yc / zc) * fy + cy;  pu = floor(u + 0.5), pv = floor(v + 0.5)
 *   IN_VIEW iff z_near < zc < z_far, |u| < 2^30 and |v| < 2^30, 0 <= pu < width and 0 <= pv < height.
 * Facing gate: c = -((nx*dx + ny*dy) + nz*dz), d2 = (dx*dx + dy*dy) + dz*dz.  With min_cos >= 0 an IN_VIEW row is TESTED iff
 *   c > 0 && c*c >= (min_cos*min_cos) * d2 (no square root); with min_cos < 0 the gate is off and every IN_VIEW row is TESTED.
 * Depth sample of pixel (px, py) of frame f: HFPF_DEPTH_U16: count d, valid iff d != 0, zd = (double)((float)d * unit) with
 *   unit = (float)depth_scale (the f32 product of the depth-frame contract); HFPF_DEPTH_F32: valid iff isfinite(d), zd = (double)d.
 *   Nothing behind (height - 1) * depth_step + width * sample size of a frame is read.
 * Class of a TESTED (row, frame): tol = tolerance + slope * zc; over the valid pixels (pu + i, pv + j), |i|, |j| <= window, inside
 *   the image, with g = zd - zc, the first rule that matches:
 *     1. SUPPORT   iff some fabs(g) <= tol
 *     2. NO_DEPTH  iff there is no valid pixel
 *     3. OCCLUDED  iff some g < -tol
 *     4. THROUGH   otherwise: every valid pixel lies more than tol behind the row.
 *   The class does not depend on the order the window is visited in.
 * Per row: n_in_view, n_tested, n_support, n_through, n_occluded count frames; first_through = the smallest frame index classed
 *   THROUGH (0xFFFFFFFF: none).  A row is CONTRADICTED iff n_through >= max(1, min_through) and
 *   (double)n_through > through_ratio * (double)n_support.
 * Output: without HFPF_CONSISTENCY_DROP every row of the row set and its record; with it only the rows that are not CONTRADICTED
 *   and their records, order kept.  Rows are byte-identical to hfpf_extract_filtered's.  summary always describes the whole row set;
 *   n_kept = n_rows - n_contradicted.  Everything is an integer sum or a minimum: nothing depends on scheduling, nor on how the
 *   frames are split into launches or uploads (HFPF_CONSISTENCY_CHUNK=1..64 forces the frames per chunk; tests).
 * A call changes nothing on the handle except device_bytes (its scratch: 32 bytes and two words per row, the poses and, for the host
 * form, one upload's frames and the output).  Rejected with HFPF_ERR_BAD_ARG (the handle stays usable, nothing is written):
 * struct_size != sizeof, unknown flags, reserved != 0, window outside 0..2, min_count NaN, not 0 < z_near < z_far with both finite,
 * tolerance not finite or outside (0, 1], slope not finite or outside [0, 1], min_cos not finite or outside [-1, 1], through_ratio
 * not finite or below 0, every check of hfpf_depth_image, a NULL depth or poses with n_frames > 0, a non-finite pose,
 * depth_frame_stride below one image or not a multiple of the sample size, n_frames > 2^20, a NULL cons, n_rows or summary (rows may
 * be NULL: not produced), on the device an image not aligned to its sample size.  n_frames = 0 returns the row set with all-zero
 * records and first_through = 0xFFFFFFFF.  An empty handle, or one before its first clean pass, returns HFPF_OK with 0 rows and NULL
 * arrays.  A handle with an RCCL communicator returns HFPF_ERR_STATE (a distributed form is not provided); a failed handle returns
 * HFPF_ERR_STATE as extract does.  Render, track, mesh and the other readers do NOT honour the result, unless hidden with
 * hfpf_hide_voxels.  Every call returns when its
 * outputs are complete. */
#define HFPF_CONSISTENCY_DROP 1u /* output only the rows that are not CONTRADICTED */
#define HFPF_CONS_SEEN 1u         /* hfpf_row_consistency.flags: n_tested > 0 */
#define HFPF_CONS_SUPPORTED 2u    /* n_support > 0 */
#define HFPF_CONS_CONTRADICTED 4u /* the rule above */

typedef struct hfpf_consistency_opts {
    uint32_t struct_size;  /* = sizeof(hfpf_consistency_opts) */
    uint32_t flags;        /* HFPF_CONSISTENCY_* */
    int32_t window;        /* 0..2: half-width, in pixels, of the window searched around (pu, pv) */
    uint32_t min_through;  /* a row is CONTRADICTED only with at least max(1, min_through) THROUGH frames */
    double min_count;      /* rows with count < min_count are dropped before the test (0 keeps all) */
    double z_near, z_far;  /* a row is IN_VIEW only iff z_near < zc < z_far */
    double tolerance;      /* metres, (0, 1]: tol = tolerance + slope * zc */
    double slope;          /* [0, 1] */
    double min_cos;        /* [-1, 1]: the facing gate; below 0 = off */
    double through_ratio;  /* >= 0: CONTRADICTED needs n_through > through_ratio * n_support */
    uint64_t reserved;     /* 0 */
} hfpf_consistency_opts;

typedef struct hfpf_row_consistency { /* 32 bytes, one per output row */
    uint32_t n_in_view, n_tested, n_support, n_through, n_occluded;
    uint32_t first_through; /* smallest frame index classed THROUGH; 0xFFFFFFFF: none */
    uint32_t flags;         /* HFPF_CONS_* */
    uint32_t reserved;      /* 0 */
} hfpf_row_consistency;

typedef struct hfpf_consistency_summary { /* 64 bytes; always of the whole row set */
    uint64_t n_rows, n_seen, n_supported, n_contradicted, n_kept;
    uint64_t pairs_tested, pairs_support, pairs_through; /* the sums of n_tested, n_support, n_through */
} hfpf_consistency_summary;

/* (four 32-bit fields, seven doubles and the reserved word: 80 bytes) */
#ifdef __cplusplus
static_assert(sizeof(hfpf_consistency_opts) == 80, "hfpf_consistency_opts is 80 bytes");
static_assert(sizeof(hfpf_row_consistency) == 32, "hfpf_row_consistency is 32 bytes");
static_assert(sizeof(hfpf_consistency_summary) == 64, "hfpf_consistency_summary is 64 bytes");
#else
_Static_assert(sizeof(hfpf_consistency_opts) == 80, "hfpf_consistency_opts is 80 bytes");
_Static_assert(sizeof(hfpf_row_consistency) == 32, "hfpf_row_consistency is 32 bytes");
_Static_assert(sizeof(hfpf_consistency_summary) == 64, "hfpf_consistency_summary is 64 bytes");
#endif

/* HFPF_OK if o passes the checks above, else HFPF_ERR_BAD_ARG (host code, no handle; the node shell uses it too). */
int hfpf_check_consistency_opts(const hfpf_consistency_opts* o);
/* Frames, poses and outputs in pageable HOST memory: the frames are uploaded in chunks through the pinned staging (the split does
 * not change a byte of the result); *rows (optional: rows == NULL = not produced) and *cons hold *n_rows entries each and are freed
 * by hfpf_free_consistency. */
int hfpf_depth_consistency(hfpf_handle* h, const hfpf_consistency_opts* o, const hfpf_depth_image* desc, const void* depth,
                           uint64_t depth_frame_stride, uint32_t n_frames, const double* poses, hfpf_row** rows, hfpf_row_consistency** cons,
                           uint64_t* n_rows, hfpf_consistency_summary* summary);
void hfpf_free_consistency(hfpf_row* rows, hfpf_row_consistency* cons);
/* The frames are read in place from DEVICE memory (HBM); poses and summary stay in host memory; *dev_rows and *dev_cons are device
 * arrays, each freed by hfpf_device_free(h, p). */
int hfpf_depth_consistency_device(hfpf_handle* h, const hfpf_consistency_opts* o, const hfpf_depth_image* desc, const void* dev_depth,
                                  uint64_t depth_frame_stride, uint32_t n_frames, const double* poses, hfpf_row** dev_rows,
                                  hfpf_row_consistency** dev_cons, uint64_t* n_rows, hfpf_consistency_summary* summary);

/* ---- hiding rows from every read-out: erase, crop, and making the filters above count (no reference counterpart) ----------------
 * hfpf_extract_components and hfpf_depth_consistency tell which rows do not belong to the surface; these calls make every read-out
 * leave such rows out, and add "erase this box" and "crop to this box".  Everything is restatable from hfpf_extract's rows
 * (tests/hide_ref.py).
 * State: a handle carries a set H of HIDDEN voxels, empty at create.  F, the FULL ROW SET, is the voxels of the rows hfpf_extract
 *   would return with H empty; H is a subset of F at all times.  "The rows hfpf_extract would return" means F minus H everywhere in
 *   this header: extract, extract_filtered, render*, track*, query* (HAS_ROW / FOUND), extract_mesh*, raycast*, extract_components*,
 *   compare_mesh*, align_mesh*, cover_mesh* and depth_consistency* are defined through those rows and inherit the rule.  NOT affected:
 *   occupancy (hfpf_get_occupied, HFPF_QHIT_OCCUPIED), every field of hfpf_counters except device_bytes, hfpf_is_dirty, integrate and
 *   clean: a hidden voxel goes on collecting points and acts as a dependant like any other.  A voxel that gets its row in a later
 *   clean pass is visible.  H lasts until these calls change it, hfpf_clear empties it, or hfpf_restore / hfpf_load replace it by the
 *   snapshot's.
 * Entries: a voxel list has n entries; entry i's voxel is three int32 (ix, iy, iz) at voxels + i * voxel_stride (12: a packed
 *   triplet list such as hfpf_get_occupied's; 64: an hfpf_row array as it is; at least 12 and a multiple of 4).  An optional selector
 *   word is a uint32 at select + i * select_stride (at least 4, a multiple of 4).  Entry i is SELECTED iff select == NULL or
 *   (word & select_mask) == select_value: hfpf_row_consistency.flags (select = &cons[0].flags, stride 32) with mask = value =
 *   HFPF_CONS_CONTRADICTED and the rows of the same call as voxels hides the contradicted rows; a labels array with mask ~0 and
 *   value c hides component c.  An entry is MATCHED iff it is SELECTED, 0 <= i_a < dim_a on every axis and its voxel is in F.
 *   M = the set of distinct matched voxels.  Nothing behind the 12 bytes of an entry's voxel or the 4 of its selector word is read.
 * Ops: HFPF_HIDE: H' = H + M.  HFPF_SHOW: H' = H - M.  HFPF_HIDE_OTHERS: H' = H + (F - M): "keep only these", "crop"; cumulative
 *   (it never shows what was hidden before); with n = 0 it hides everything.
 * Box form: M = the voxels of F with lo[a] <= i_a <= hi[a] on every axis (inclusive voxel indices; the box may reach outside
 *   0..dim-1; lo > hi on an axis is the empty box); same ops.
 * Result (res may be NULL): n_selected = entries selected, n_matched = entries matched (duplicates counted), n_changed = the voxels
 *   in exactly one of H and H', n_hidden = |H'|, n_full = |F|; for the box form n_selected = n_matched = |M|.  Integer counts:
 *   nothing depends on scheduling, nor on duplicates in the list or on how a host list is split into uploads.
 * Host frames still waiting are launched first and a clean pass that returned without waiting is waited for, as hfpf_extract does;
 * deferred errors surface as they do there.  Every call returns when H' is in place.  The first call that hides a voxel allocates
 * the hidden bits (64 bytes per brick of max_bricks, counted in device_bytes).
 * Rejected with HFPF_ERR_BAD_ARG (the handle stays usable, H is unchanged): struct_size != sizeof, an unknown op, flags or reserved
 * != 0, a bad stride, a NULL voxels with n > 0, a device pointer not 4-byte aligned, NULL lo or hi, a result whose struct_size !=
 * sizeof.  HFPF_ERR_STATE: a failed handle, as extract; a handle with an RCCL communicator; a handle that has exported or imported
 * epoch records (the rule of hfpf_snapshot: a distributed form is not provided).  An empty handle, or one before its first clean
 * pass, returns HFPF_OK with an all-zero result. */
#define HFPF_HIDE 1u        /* H' = H + M */
#define HFPF_SHOW 2u        /* H' = H - M */
#define HFPF_HIDE_OTHERS 3u /* H' = H + (F - M) */

typedef struct hfpf_hide_opts {
    uint32_t struct_size;  /* = sizeof(hfpf_hide_opts) */
    uint32_t op;           /* HFPF_HIDE, HFPF_SHOW or HFPF_HIDE_OTHERS */
    uint32_t select_mask;  /* entry i is SELECTED iff select == NULL or (word & select_mask) == select_value */
    uint32_t select_value;
    uint32_t flags;        /* 0 */
    uint32_t reserved;     /* 0 */
} hfpf_hide_opts;

typedef struct hfpf_hide_result {
    uint32_t struct_size;  /* = sizeof(hfpf_hide_result), set by the caller */
    uint32_t reserved;     /* written 0 */
    uint64_t n_selected, n_matched, n_changed, n_hidden, n_full;
} hfpf_hide_result;

#ifdef __cplusplus
static_assert(sizeof(hfpf_hide_opts) == 24, "hfpf_hide_opts is 24 bytes");
static_assert(sizeof(hfpf_hide_result) == 48, "hfpf_hide_result is 48 bytes");
#else
_Static_assert(sizeof(hfpf_hide_opts) == 24, "hfpf_hide_opts is 24 bytes");
_Static_assert(sizeof(hfpf_hide_result) == 48, "hfpf_hide_result is 48 bytes");
#endif

/* HFPF_OK if o passes the checks above, else HFPF_ERR_BAD_ARG (host code, no handle; the node shell uses it too). */
int hfpf_check_hide_opts(const hfpf_hide_opts* o);
/* voxels and select in pageable HOST memory: uploaded in chunks through the pinned staging. */
int hfpf_hide_voxels(hfpf_handle* h, const hfpf_hide_opts* o, const void* voxels, uint64_t n, uint32_t voxel_stride, const void* select,
                     uint32_t select_stride, hfpf_hide_result* res);
/* The same with voxels and select in DEVICE memory (HBM), 4-byte aligned, read in place: the rows, labels or records a *_device
 * read-out returned go straight back in.  o and res stay in host memory. */
int hfpf_hide_voxels_device(hfpf_handle* h, const hfpf_hide_opts* o, const void* dev_voxels, uint64_t n, uint32_t voxel_stride,
                            const void* dev_select, uint32_t select_stride, hfpf_hide_result* res);
/* op on the box lo..hi (host memory, inclusive voxel indices). */
int hfpf_hide_box(hfpf_handle* h, uint32_t op, const int32_t lo[3], const int32_t hi[3], hfpf_hide_result* res);
/* H = {} (the hidden bits stay allocated). */
int hfpf_show_all(hfpf_handle* h);
/* The voxels of H in ascending (x,y,z) order, as hfpf_get_occupied lists the occupied ones: xyz may be NULL to query the count; at
 * most cap triplets are written. */
int hfpf_get_hidden(hfpf_handle* h, int32_t* xyz, uint64_t cap, uint64_t* n_out);

/* <directory_name>/test_cloud.pcd (node.cpp:395): PCD v0.7 ASCII, FIELDS x y z rgb normal_x normal_y normal_z curvature */
int hfpf_write_pcd(const hfpf_row* rows, uint64_t n_rows, const char* path);
/* <directory_name>/meta.csv (node.cpp:396) with the header string of grid.hpp:462 */
int hfpf_write_meta_csv(const hfpf_row* rows, uint64_t n_rows, const char* path);

/* The alternate extractors the reference keeps behind `#if 0` (node.cpp:399-437): download(XYZRGB), downloadHQ(threshold)
 * and downloadClassified (grid.hpp:491-575), as one PointXYZRGB writer over extracted rows.  min_count: rows with
 * count < min_count are skipped (downloadHQ; 0 keeps all).  white != 0 paints r=g=b=255 as those functions do.
 * classify_threshold >= 0 paints rows with count > threshold red (downloadClassified uses kGoodPointsThreshold = 100). */
int hfpf_write_pcd_xyzrgb(const hfpf_row* rows, uint64_t n_rows, const char* path, uint32_t min_count,
                          int32_t classify_threshold, int32_t white);
/* test_cloud.pcd with DATA binary (same fields; for the 10k-frame configs where ASCII formatting dominates). */
int hfpf_write_pcd_binary(const hfpf_row* rows, uint64_t n_rows, const char* path);

/* OccupancyGrid::clearVoxels (grid.hpp:167-183; call site node.cpp:438).  Full reset (documented
 * deviation: the reference leaves stale keys and dependants-only blocks behind).  Waits for the work enqueued on the handle
 * (it reads how many bricks and records the session used and resets that much of the tables, not their whole capacity);
 * frames of hfpf_integrate still waiting for their launch are dropped. */
int hfpf_clear(hfpf_handle* h);

/* Wait for all queued work of this handle; surfaces deferred capacity/HIP errors. */
int hfpf_sync(hfpf_handle* h);
int hfpf_get_counters(hfpf_handle* h, hfpf_counters* out);

/* Occupied voxel triplets in ascending (x,y,z) order (test/diagnostic: bit-exact occupancy parity).
 * xyz may be NULL to query the count; at most cap triplets are written. */
int hfpf_get_occupied(hfpf_handle* h, int32_t* xyz, uint64_t cap, uint64_t* n_out);

/* ---- snapshot and restore of a fusion session (no reference counterpart: its grid lives and dies with the process) ----------
 * WHAT A SNAPSHOT IS.  The state of the handle at this point of the call sequence, as one block of HOST memory.  Host frames still
 * waiting for their launch are launched first and a clean pass that returned without waiting is waited for, as hfpf_extract does;
 * deferred errors surface here as they do there.  A snapshot may be taken at any point: before the first frame, between integrate
 * and clean (dirty: points buffered but not yet replayed, cells waiting for the gate), after a clean, after hfpf_clear.  It changes
 * nothing on the handle except device_bytes (its staging scratch).
 *
 * WHAT A RESTORE IS.  hfpf_clear followed by putting that state in place.  Afterwards the handle is indistinguishable from the
 * source handle at the moment of the snapshot, in this sense:
 *   1. every read-only call (extract, extract_filtered, get_occupied, get_hidden, is_dirty, render*, query*, extract_mesh*,
 *      raycast*, track*, extract_components*, compare_mesh*, align_mesh*, cover_mesh*, depth_consistency*)
 *      returns byte-identical output: the HIDDEN set of hfpf_hide_* travels in the snapshot, as one more section that is present only
 *      when the set is not empty (a snapshot of a handle that hides nothing, hfpf_show_all included, is the blob it always was);
 *   2. any continuation (integrate*, clean, extract, clear, hide_*, show_all, automatic frame ids included) produces byte-identical rows and occupied
 *      lists to the same continuation on the source handle;
 *   3. hfpf_get_counters agrees in every field results depend on: points_presented, points_zclip_pass, points_in_bbox,
 *      points_buffered, dep_pairs_tested, dep_pairs_member, voxels_occupied, voxels_with_normal, bricks_allocated, registrations,
 *      frames_integrated, clean_passes, replay_members.  The scheduling diagnostics (points_direct, table_misses,
 *      update_extra_rounds, dep_entries, device_bytes) and the kernel timings need not.
 * Scheduling state that results never depend on (bin plans, the shape of the dependant update, staging rings) is not part of a
 * snapshot.  This relies on what the engine already guarantees -- integer statistic sums, ties broken by key -- and on nothing new.
 *
 * COMPATIBILITY.  The target handle must have the same resolution (as f32 bits), bbox, k, K, gate, radii, z-clips and the same
 * HFPF_FLAG_FUSE_COLOR and HFPF_FLAG_PCL_SHIFTED_COV: HFPF_ERR_BAD_CONFIG otherwise.  It may differ in device,
 * HFPF_FLAG_DIRECT_UPDATE, frame_width and max_call_points, and in max_bricks, max_normals and max_frames as long as what the
 * session used fits (HFPF_ERR_CAPACITY otherwise; the handle is not poisoned).  max_log_points must be EQUAL (as the engine
 * rounded it: hfpf_snapshot_info reports the value to create with): indices into the point log encode its append region, and they
 * are not remapped.  A snapshot also carries a tag of the layout of the engine's internal tables; a blob with another format
 * version or layout tag is refused with HFPF_ERR_BAD_ARG.  Snapshots are a RESUME format between builds of one table layout, not
 * an archive format.
 *
 * ERRORS.  Everything the host can decide is decided before a byte reaches the device: NULL arguments, a blob shorter than its
 * header says, bad magic, version or layout tag, a header or payload whose 64-bit checksum does not match (all HFPF_ERR_BAD_ARG, from
 * hfpf_load too), configuration or capacity mismatch.  All of these leave the target exactly as it was: usable, same
 * rows.  hfpf_save / hfpf_load add HFPF_ERR_IO for a file that cannot be opened, read or written in full (a short write removes the
 * partial file).  A failure after the upload has begun (a HIP error, or the device-side range check of the restored indices:
 * HFPF_ERR_IO) leaves the handle as after hfpf_clear.  A poisoned handle cannot be snapshotted (HFPF_ERR_STATE, as extract) but
 * can be restored into.  A handle with an RCCL communicator, or one that has exported or imported epoch records (hfpf_epoch_*,
 * hfpf_stats_export), returns HFPF_ERR_STATE from all four calls: a distributed snapshot is not provided.
 *
 * SIZE.  A snapshot's size follows what the session used, never the pool capacities; unused bytes are zero, so two snapshots of one
 * state are equal byte for byte.  The size is a function of the session's counts alone (bricks, records, occupied and pending cells,
 * registrations, dependant entries, buffered points, frames, whether anything is hidden) -- not of how the buffered points happened
 * to spread over the point log's append regions, which differs from run to run.  Between a snapshot and the snapshot of its restore elsewhere the payload and its checksum are equal; of
 * the header only `flags` may differ (it records the handle's own flags word, HFPF_FLAG_DIRECT_UPDATE included): capacities are not
 * stored, only the needed ones. */
#define HFPF_SNAPSHOT_HEADER_BYTES 4096u /* hfpf_snapshot_info needs this many leading bytes of a blob or file */
/* Filled from the header alone (host code; no handle, no GPU).  struct tag only: the function below carries the same name. */
struct hfpf_snapshot_info {
    uint32_t struct_size;     /* = sizeof(struct hfpf_snapshot_info), set by the caller */
    uint32_t format_version;
    uint64_t layout_tag;      /* table layout of the build that wrote the blob */
    uint64_t total_bytes;     /* header + payload = the size of the blob / file */
    uint64_t payload_bytes;
    uint64_t payload_checksum;
    /* the grid configuration the snapshot was made with */
    float resolution;         /* as the f32 hfpf_config carried */
    uint32_t flags;           /* HFPF_FLAG_* of the source handle */
    double bbox[6];
    int32_t k, K, gate;
    int32_t reserved0;
    double cylinder_radius, ball_radius, z_clip_min, z_clip_max;
    /* the smallest pool capacities a handle needs to take it (max_log_points: exactly this value) */
    uint64_t max_bricks, max_log_points, max_normals, max_frames;
    /* the session */
    uint64_t frames_integrated, clean_passes, next_frame_id, voxels_occupied, voxels_with_normal;
    uint64_t reserved[4];     /* 0 */
};
int hfpf_snapshot(hfpf_handle* h, void** blob, uint64_t* bytes); /* HOST memory, freed by hfpf_free_snapshot */
void hfpf_free_snapshot(void* blob);
int hfpf_restore(hfpf_handle* h, const void* blob, uint64_t bytes);
int hfpf_save(hfpf_handle* h, const char* path); /* the same bytes, written to a file */
int hfpf_load(hfpf_handle* h, const char* path);
/* HFPF_ERR_BAD_ARG (nothing written): NULL, bytes below HFPF_SNAPSHOT_HEADER_BYTES, wrong magic, out->struct_size, format version
 * or header checksum.  The payload is neither needed nor looked at. */
int hfpf_snapshot_info(const void* blob, uint64_t bytes, struct hfpf_snapshot_info* out);
/* hfpf_default_config, then the grid configuration of the snapshot, its semantic flags (colour fusion, shifted covariance) and the
 * needed capacities; device and scheduling hints stay at their defaults. */
int hfpf_config_from_snapshot(const struct hfpf_snapshot_info* info, hfpf_config* cfg);

/* ---- harness helpers (device staging without any framework) ---- */
int hfpf_device_alloc(hfpf_handle* h, uint64_t bytes, void** dev_ptr);
int hfpf_device_free(hfpf_handle* h, void* dev_ptr);
int hfpf_device_upload(hfpf_handle* h, void* dev_dst, const void* host_src, uint64_t bytes);


/* ---- multi-GPU (one handle per GPU, one process per GPU) ----------------------------------------------
 * The reference is single-process; sharding follows SURVEY.md 8(e): frames (or cameras) are dealt to ranks, each
 * rank integrates only its own frames with GLOBAL frame ids (hfpf_integrate_device frame_ids), and every rank calls
 * hfpf_clean / hfpf_extract at the same points of the schedule (they become collectives).  At a clean the ranks
 * exchange the cells they occupied since the last clean (key, smallest frame id, its viewpoint); normals and
 * registrations are then computed redundantly and identically on every rank; buffers and statistic sums stay
 * private and are added (exact int64) at extract.  The result is bit-identical to one GPU fusing all frames.
 *
 * Transport 1: RCCL.  Rank 0 calls hfpf_dist_unique_id, the launcher broadcasts the 128 bytes (bench.py uses
 * torch.distributed/gloo, a C++ host would use MPI or a file), every rank calls hfpf_dist_init. */
int hfpf_dist_unique_id(void* id128);
int hfpf_dist_init(hfpf_handle* h, int rank, int world, const void* id128);
/* Rank and rank count as the RCCL communicator reports them (ncclCommUserRank / ncclCommCount); 0 and 1 without one. */
int hfpf_dist_info(hfpf_handle* h, int32_t* rank, int32_t* world);
/* Drop the communicator again (e.g. when not every rank managed to create one); clean/extract become local calls. */
int hfpf_dist_disable(hfpf_handle* h);
/* Transport 2: bring your own.  The same exchange as explicit steps on device buffers (also how tests run several
 * virtual ranks on one GPU): export -> move the 16-byte records (ABI 6; 32 bytes until ABI 5: one record per newly occupied cell --
 * key, smallest frame id -- and two per frame integrated since the last exchange -- its viewpoint, which used to ride on every
 * cell record) -> import into every other rank -> hfpf_clean;
 * at the end add the ranks' hfpf_stats_export words and hand the totals to hfpf_extract_with_stats.
 * Exported pointers are device memory owned by the handle, valid until its next mutating call.
 * What an import does with a record a transport hands in: a cell key is x << sx | y << sy | z with just enough bits per axis for
 * 0..dim (hfpf_get_dims); storage is dim + 1 cells an axis, so a coordinate EQUAL to dim is kept and a key with a coordinate of
 * dim + 1 or more -- x judged on all the key's bits above y -- is dropped.  A first_frame >= max_frames leaves the cell's latch as
 * it was (the cell itself is still taken), and a frame record whose id is >= max_frames changes nothing.  None of these is an error.
 * The cells an import adds count against max_normals * 4 and max_bricks like local ones: an overflow is HFPF_ERR_CAPACITY from
 * the next call that reads the counters back (hfpf_clean), as for hfpf_integrate. */
int hfpf_epoch_export(hfpf_handle* h, const void** dev_records, uint64_t* n_records);
int hfpf_epoch_import(hfpf_handle* h, const void* dev_records, uint64_t n_records);
/* Since ABI 3 the optional colour sums are words 5-7 of the same 8-word records: *dev_cwords is NULL, *n_cwords 0, and
 * hfpf_extract_with_stats ignores dev_cwords (both parameters are kept so that ABI-2 callers still link). */
/* The receive side of a padded all-gather, as the RCCL path runs it: `world` slices of slice_stride_bytes each, slice r holding
 * counts[r] 16-byte records (padding behind them is never read); every slice but my_rank's is imported.  Unequal and zero
 * counts are the normal case.  A foreign count that does not fit the stride is HFPF_ERR_BAD_ARG, and no slice is imported. */
int hfpf_epoch_import_gathered(hfpf_handle* h, const void* dev_buffer, uint64_t slice_stride_bytes, int32_t world, int32_t my_rank,
                               const uint64_t* counts);
int hfpf_stats_export(hfpf_handle* h, const void** dev_words, uint64_t* n_words, const void** dev_cwords, uint64_t* n_cwords);
int hfpf_extract_with_stats(hfpf_handle* h, const void* dev_words, const void* dev_cwords, hfpf_row** rows, uint64_t* n_rows);
int hfpf_device_download(hfpf_handle* h, void* host_dst, const void* dev_src, uint64_t bytes);
int hfpf_device_copy(hfpf_handle* h, void* dev_dst, const void* dev_src, uint64_t bytes); /* device to device, synchronous */

/* ---- measurement: HIP-event timing of the engine's own kernels on the engine's stream ----
 * kernel ids: 0 = integrate calls (bin plan + k_integrate + k_update_cells + k_buffer), 1 = whole clean passes (first to last
 * kernel of hfpf_clean, host read-backs included).  enable = 2 additionally brackets the kernels of every integrate call:
 * 2 = k_integrate, 3 = k_update_cells / k_update, 4 = k_buffer (three more event records per call: use it for a breakdown
 * pass, not for the headline timing).  5 = k_raycast launches of hfpf_raycast* (the march alone, without the empty-space maps and
 * the copies; any enable).  6 = the component kernels of one hfpf_extract_components* call (index to compaction, the scans' read-backs
 * included, without the row set and the copies; any enable).  7 = the compare kernels of one hfpf_compare_mesh* call (binning to
 * the row kernel, the read-backs of the sizes included, without the row set and the copies; any enable).  total_ms / launches
 * accumulate since enable.  hfpf_align_mesh* has no id of its own and is not filed under 7. */
int hfpf_kernel_timing(hfpf_handle* h, int enable);
int hfpf_get_kernel_time(hfpf_handle* h, int kernel_id, double* total_ms, uint64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* HFPF_H */
