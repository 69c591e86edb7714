// host/fusion_node.cpp -- ROS-free shell of pointcloud_fusion_and_filter over the C ABI (include/hfpf_node.h).
//
// What changed relative to the reference's threading (node.cpp:166-168): the decode/clip thread (addPoints,
// node.cpp:218-263) and the transform/insert thread (updateStates, node.cpp:265-299) existed to overlap CPU work;
// both stages are one GPU launch now, so the subscriber callback hands the message straight to hfpf_integrate
// (which copies it to pinned staging and returns).  The clean thread (cleanGrid, node.cpp:301-325) is kept.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hfpf_node.h"

struct hfpf_node {
    hfpf_handle* grid = nullptr;
    std::string fusion_frame, directory_name, err;
    hfpf_tf_lookup_fn tf = nullptr;
    void* tf_user = nullptr;
    std::atomic<bool> start_{false};                       // node.cpp:135 (a plain bool shared across threads there)
    std::atomic<bool> cloud_subscription_started_{false};  // node.cpp:136
    std::string pointcloud_frame_;                         // node.cpp:128
    std::mutex frame_mtx;
    double bbox_min[3] = {0, 0, 0};  // of the grid: hfpf_node_hide_box turns metres into voxel indices
    double clean_period_s = 5.0;
    bool final_clean = false;
    bool write_variants = false;
    hfpf_publish_fn publish = nullptr;  // ~pcl_fusion_node/processed_cloud_normals (node.cpp:158)
    bool mesh_on = false;               // hfpf_node_set_mesh_output: ~process also writes mesh.ply
    hfpf_mesh_opts mesh_opts{};
    bool comp_on = false;               // hfpf_node_set_component_filter: ~process saves the rows of the kept components only
    hfpf_component_opts comp_opts{};
    bool hide_filtered = false;         // hfpf_node_set_hide_filtered: ~process hides what the component filter drops, so that every file leaves it out
    bool comp_rows = false;             // of the running ~process: the saved rows are the filter's selection from the full row set (comp_on, not hidden)
    bool ref_on = false;               // hfpf_node_set_reference_mesh: ~process also writes deviation.csv and deviation_summary.csv
    hfpf_deviation_opts ref_opts{};
    std::vector<float> ref_verts;       // packed x, y, z
    std::vector<uint32_t> ref_tris;
    double ref_pose[12] = {0};
    bool align_on = false;              // hfpf_node_set_reference_alignment: the reference mesh is best-fitted before it is compared
    hfpf_align_opts align_opts{};
    bool cover_on = false;              // hfpf_node_set_reference_coverage: ~process also writes coverage.csv and coverage_summary.csv
    hfpf_cover_opts cover_opts{};
    bool plan_on = false;               // hfpf_node_set_view_candidates: ~process also writes view_plan.csv and view_plan_summary.csv
    hfpf_plan_opts plan_opts{};
    std::vector<double> plan_poses;     // 12 per candidate view
    bool cons_on = false;               // hfpf_node_set_depth_consistency: ~process also writes consistency.csv and consistency_summary.csv
    hfpf_consistency_opts cons_opts{};
    uint32_t cons_keep = 0;             // depth images the ring holds at most
    std::mutex cons_mtx;                // the ring below: the depth callback fills it, ~process reads it
    hfpf_depth_image cons_desc{};       // descriptor of the images in the ring
    std::vector<std::vector<uint8_t>> cons_frames;  // host copies of the last integrated depth images, oldest first
    std::vector<double> cons_poses;     // 12 per image
    bool sec_on = false;                // hfpf_node_set_section_planes: ~process also writes sections.csv and section_summary.csv
    hfpf_section_opts sec_opts{};
    std::vector<double> sec_planes;     // 4 per plane
    bool top_on = false;                // hfpf_node_set_mesh_topology: ~process also writes mesh_edges.csv, mesh_loops.csv, mesh_shells.csv and the summary
    hfpf_topology_opts top_opts{};
    void* publish_user = nullptr;
    std::thread clean_thread;
    std::mutex cv_mtx;
    std::condition_variable cv;
    bool quit = false;
    std::atomic<uint64_t> received{0}, integrated{0}, dropped_not_started{0}, dropped_tf{0}, clean_passes{0}, process_calls{0};
};

namespace {
thread_local std::string g_err;  // last error of hfpf_node_create

int nfail(hfpf_node* n, int code, const std::string& msg)
{
    if (n) n->err = msg;
    else g_err = msg;
    return code;
}

void set_res(hfpf_trigger_response* res, bool ok, const std::string& msg)
{
    if (!res) return;
    res->success = ok ? 1 : 0;
    snprintf(res->message, sizeof res->message, "%s", msg.c_str());
}

void clean_loop(hfpf_node* n)  // cleanGrid, node.cpp:301-325
{
    std::unique_lock<std::mutex> lk(n->cv_mtx);
    while (!n->quit) {
        lk.unlock();
        if (hfpf_is_dirty(n->grid) > 0) {  // if(grid_.state_changed)
            if (hfpf_clean(n->grid) == HFPF_OK) n->clean_passes++;
            else fprintf(stderr, "[hfpf_node] clean failed: %s\n", hfpf_last_error(n->grid));
        }
        lk.lock();
        n->cv.wait_for(lk, std::chrono::duration<double>(n->clean_period_s), [n] { return n->quit; });  // sleep(5)
    }
}
}  // namespace

extern "C" {

void hfpf_node_default_params(hfpf_node_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->struct_size = sizeof *p;
    p->fusion_frame = "fusion_frame";  // node.cpp:447
    p->directory_name = "./";          // node.cpp:449
    p->bounding_box = nullptr;         // node.cpp:451 default: empty vector
    p->bounding_box_len = 0;
    hfpf_default_config(&p->engine);
    p->clean_period_s = 5.0;  // node.cpp:323
    p->final_clean_on_process = 0;
    p->write_variants = 0;
}

const char* hfpf_node_last_error(const hfpf_node* n) { return n ? n->err.c_str() : g_err.c_str(); }

int hfpf_node_create(const hfpf_node_params* p, hfpf_tf_lookup_fn tf, void* tf_user, hfpf_node** out)
{
    if (!p || !out) return nfail(nullptr, HFPF_ERR_BAD_ARG, "hfpf_node_create: null argument");
    *out = nullptr;
    if (p->struct_size != sizeof(hfpf_node_params)) return nfail(nullptr, HFPF_ERR_BAD_CONFIG, "hfpf_node_params.struct_size mismatch");
    // the reference reads box[0..5] of whatever the parameter server returned (node.cpp:451,162): out-of-bounds when empty
    if (!p->bounding_box || p->bounding_box_len != 6)
        return nfail(nullptr, HFPF_ERR_BAD_CONFIG, "param bounding_box must hold 6 values (xmin,xmax,ymin,ymax,zmin,zmax)");
    hfpf_node* n = new hfpf_node();
    n->fusion_frame = p->fusion_frame ? p->fusion_frame : "fusion_frame";
    n->directory_name = p->directory_name ? p->directory_name : "./";
    n->tf = tf;
    n->tf_user = tf_user;
    n->clean_period_s = p->clean_period_s;
    n->final_clean = p->final_clean_on_process != 0;
    n->write_variants = p->write_variants != 0;
    hfpf_config cfg = p->engine;
    cfg.struct_size = sizeof cfg;
    memcpy(cfg.bbox, p->bounding_box, 6 * sizeof(double));
    for (int a = 0; a < 3; a++) n->bbox_min[a] = p->bounding_box[2 * a];
    int rc = hfpf_create(&cfg, &n->grid);
    if (rc != HFPF_OK) {
        g_err = hfpf_last_error(nullptr);
        delete n;
        return rc;
    }
    if (n->clean_period_s > 0) n->clean_thread = std::thread(clean_loop, n);
    *out = n;
    return HFPF_OK;
}

int hfpf_node_destroy(hfpf_node* n)
{
    if (!n) return HFPF_OK;
    {
        std::lock_guard<std::mutex> lk(n->cv_mtx);
        n->quit = true;
    }
    n->cv.notify_all();
    if (n->clean_thread.joinable()) n->clean_thread.join();
    hfpf_destroy(n->grid);
    delete n;
    return HFPF_OK;
}

// onReceivedPointCloud up to the integrate call (node.cpp:327-344): 1 = integrate with `pose`, 0 = dropped.
static int gate_and_lookup(hfpf_node* n, const char* frame_id, double pose[12])
{
    n->received++;
    {
        std::lock_guard<std::mutex> lk(n->frame_mtx);
        n->pointcloud_frame_ = frame_id ? frame_id : "";  // node.cpp:329
    }
    n->cloud_subscription_started_ = true;  // node.cpp:330
    if (!n->start_) {                       // node.cpp:331
        n->dropped_not_started++;
        return 0;
    }
    const double identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};  // Affine3d::Identity(), node.cpp:333
    memcpy(pose, identity, sizeof identity);
    if (n->tf) {
        char err[256] = {0};
        if (n->tf(n->tf_user, n->fusion_frame.c_str(), frame_id ? frame_id : "", pose, err, sizeof err) != 0) {
            fprintf(stderr, "[hfpf_node] WARN %s\n", err);  // ROS_WARN + drop, node.cpp:340-344
            n->dropped_tf++;
            return 0;
        }
    }
    return 1;
}

int hfpf_node_on_point_cloud(hfpf_node* n, const hfpf_cloud_msg* msg)
{
    if (!n || !msg) return HFPF_ERR_BAD_ARG;
    double pose[12];
    if (gate_and_lookup(n, msg->frame_id, pose) == 0) return 0;
    if (!msg->data || msg->point_step == 0) return nfail(n, HFPF_ERR_BAD_ARG, "empty PointCloud2");
    const uint32_t n_points = msg->row_step / msg->point_step;  // first row only, node.cpp:185,190
    int rc = hfpf_integrate(n->grid, msg->data, n_points, msg->point_step, msg->off_x, msg->off_y, msg->off_z, msg->off_rgb, pose);
    if (rc != HFPF_OK) return nfail(n, rc, hfpf_last_error(n->grid));
    n->integrated++;
    return 1;
}

static void forget_depth(hfpf_node* n)
{
    std::lock_guard<std::mutex> lk(n->cons_mtx);
    n->cons_frames.clear();
    n->cons_poses.clear();
}

// The ring of hfpf_node_set_depth_consistency: a host copy of a depth image the engine has just taken (so its descriptor is valid)
// and its pose.  An image of another descriptor empties the ring first: one call compares frames of one descriptor.
static void remember_depth(hfpf_node* n, const hfpf_depth_msg* msg, const double pose[12])
{
    std::lock_guard<std::mutex> lk(n->cons_mtx);
    if (!n->cons_on || n->cons_keep == 0) return;
    const hfpf_depth_image& d = msg->image;
    if (!n->cons_frames.empty() && memcmp(&n->cons_desc, &d, sizeof d) != 0) n->cons_frames.clear(), n->cons_poses.clear();
    n->cons_desc = d;
    const size_t bytes = (size_t)(d.height - 1) * d.depth_step + (size_t)d.width * (d.depth_format == HFPF_DEPTH_F32 ? 4u : 2u);
    if (n->cons_frames.size() >= n->cons_keep) {
        n->cons_frames.erase(n->cons_frames.begin());
        n->cons_poses.erase(n->cons_poses.begin(), n->cons_poses.begin() + 12);
    }
    const uint8_t* src = (const uint8_t*)msg->depth;
    n->cons_frames.emplace_back(src, src + bytes);
    n->cons_poses.insert(n->cons_poses.end(), pose, pose + 12);
}

int hfpf_node_on_depth_image(hfpf_node* n, const hfpf_depth_msg* msg)
{
    if (!n || !msg) return HFPF_ERR_BAD_ARG;
    double pose[12];
    if (gate_and_lookup(n, msg->frame_id, pose) == 0) return 0;
    int rc = hfpf_integrate_depth(n->grid, &msg->image, msg->depth, msg->color, pose);
    if (rc != HFPF_OK) return nfail(n, rc, hfpf_last_error(n->grid));
    n->integrated++;
    remember_depth(n, msg, pose);
    return 1;
}

int hfpf_node_start(hfpf_node* n, hfpf_trigger_response* res)
{
    if (!n) return HFPF_ERR_BAD_ARG;
    n->start_ = true;  // node.cpp:364
    set_res(res, true, "");
    return HFPF_OK;
}

int hfpf_node_stop(hfpf_node* n, hfpf_trigger_response* res)
{
    if (!n) return HFPF_ERR_BAD_ARG;
    n->start_ = false;  // node.cpp:372
    set_res(res, true, "");
    return HFPF_OK;
}

int hfpf_node_reset(hfpf_node* n, hfpf_trigger_response* res)
{
    if (!n) return HFPF_ERR_BAD_ARG;
    n->start_ = false;                       // node.cpp:354
    n->cloud_subscription_started_ = false;  // node.cpp:357 (clouds_.clear(): no queue here; the grid is NOT touched)
    forget_depth(n);
    set_res(res, true, "");
    return HFPF_OK;
}

// deviation.csv and deviation_summary.csv beside the cloud: one line per saved row.  The compare runs on the full row set (with the
// component filter's min_count when one is set); the saved rows are a subsequence of it in the same lexicographic order, so one walk
// selects their records, and the row part of the summary is rebuilt from the selected records as include/hfpf.h defines it.
// With alignment on the reference mesh is first best-fitted from its stored pose; the compare then runs at the refined pose, which
// alignment.csv records.  pose: out, the pose the compare ran at.
static int write_deviation(hfpf_node* n, const hfpf_row* saved, uint64_t n_saved, double pose[12])
{
    hfpf_deviation_opts o = n->ref_opts;
    if (n->comp_rows) o.min_count = n->comp_opts.min_count;
    memcpy(pose, n->ref_pose, 12 * sizeof(double));
    if (n->align_on) {
        hfpf_align_opts ao = n->align_opts;
        if (n->comp_rows) ao.compare.min_count = n->comp_opts.min_count;
        hfpf_align_result ar;
        memset(&ar, 0, sizeof ar);
        ar.struct_size = sizeof ar;
        int arc = hfpf_align_mesh(n->grid, &ao, n->ref_verts.data(), n->ref_verts.size() / 3, 12, n->ref_tris.data(), n->ref_tris.size() / 3, n->ref_pose, &ar);
        if (arc != HFPF_OK) return arc;
        memcpy(pose, ar.pose, 12 * sizeof(double));
        FILE* af = fopen((n->directory_name + "/alignment.csv").c_str(), "w");
        if (!af) return HFPF_ERR_IO;
        fprintf(af, "iterations,flags,rows_sampled,inliers,rms,p0,p1,p2,p3,p4,p5,p6,p7,p8,p9,p10,p11\n%u,%u,%llu,%llu,%.17g", ar.iterations, ar.flags,
                (unsigned long long)ar.rows_sampled, (unsigned long long)ar.inliers, ar.rms);
        for (int i = 0; i < 12; i++) fprintf(af, ",%.17g", pose[i]);
        fprintf(af, "\n");
        const bool ok = !ferror(af);
        if (fclose(af) != 0 || !ok) return HFPF_ERR_IO;
    }
    hfpf_row* all = nullptr;
    hfpf_deviation* dev = nullptr;
    uint64_t n_all = 0;
    hfpf_deviation_summary s;
    int rc = hfpf_compare_mesh(n->grid, &o, n->ref_verts.data(), n->ref_verts.size() / 3, 12, n->ref_tris.data(), n->ref_tris.size() / 3, pose,
                               n->comp_rows ? &all : nullptr, &dev, &n_all, &s);
    if (rc != HFPF_OK) return rc;
    FILE* f = fopen((n->directory_name + "/deviation.csv").c_str(), "w");
    if (!f) rc = HFPF_ERR_IO;
    if (f) {
        fprintf(f, "ix,iy,iz,signed_distance,distance,tri,flags\n");
        if (n->comp_rows) s.n_rows = s.n_found = s.n_negative = 0, s.max_abs = 0.f, s.sum_abs_q30 = s.sum_sq_q30 = 0;
        uint64_t j = 0;
        for (uint64_t i = 0; i < n_saved && rc == HFPF_OK; i++) {
            const hfpf_row& r = saved[i];
            if (n->comp_rows)
                while (j < n_all && (all[j].ix != r.ix || all[j].iy != r.iy || all[j].iz != r.iz)) j++;
            else j = i;
            if (j >= n_all) {
                rc = HFPF_ERR_STATE;  // cannot happen: both row sets come from one state of the grid
                break;
            }
            const hfpf_deviation& d = dev[j];
            fprintf(f, "%d,%d,%d,%.9g,%.9g,%u,%u\n", r.ix, r.iy, r.iz, d.signed_distance, d.distance, d.tri, d.flags);
            if (n->comp_rows) {
                s.n_rows++;
                if (d.flags & HFPF_DEV_FOUND) {
                    const double w = (double)d.distance;
                    s.n_found++;
                    s.n_negative += d.signed_distance < 0.f ? 1 : 0;
                    s.max_abs = std::max(s.max_abs, d.distance);
                    s.sum_abs_q30 += (int64_t)llrint(w * 0x1p30);
                    s.sum_sq_q30 += (int64_t)llrint((w * w) * 0x1p30);
                }
            }
        }
        const bool ok = !ferror(f);
        if (fclose(f) != 0 || !ok) rc = rc == HFPF_OK ? HFPF_ERR_IO : rc;
    }
    if (rc == HFPF_OK) {
        f = fopen((n->directory_name + "/deviation_summary.csv").c_str(), "w");
        if (!f) rc = HFPF_ERR_IO;
        else {
            fprintf(f, "n_rows,n_found,n_negative,n_tris_valid,n_tris_invalid,max_abs,sum_abs_q30,sum_sq_q30\n%llu,%llu,%llu,%llu,%llu,%.9g,%lld,%lld\n",
                    (unsigned long long)s.n_rows, (unsigned long long)s.n_found, (unsigned long long)s.n_negative, (unsigned long long)s.n_tris_valid,
                    (unsigned long long)s.n_tris_invalid, s.max_abs, (long long)s.sum_abs_q30, (long long)s.sum_sq_q30);
            const bool ok = !ferror(f);
            if (fclose(f) != 0 || !ok) rc = HFPF_ERR_IO;
        }
    }
    hfpf_free_deviation(all, dev);
    return rc;
}

// coverage.csv and coverage_summary.csv beside the cloud: hfpf_cover_mesh of the reference mesh at `pose`, the pose the deviation
// files were written at; one line per triangle.  A component filter's min_count replaces the option's, as it does for the compare.
static int write_coverage(hfpf_node* n, const double pose[12])
{
    hfpf_cover_opts o = n->cover_opts;
    if (n->comp_rows) o.min_count = n->comp_opts.min_count;
    hfpf_tri_coverage* cov = nullptr;
    hfpf_coverage_summary s;
    const uint64_t n_tris = n->ref_tris.size() / 3;
    int rc = hfpf_cover_mesh(n->grid, &o, n->ref_verts.data(), n->ref_verts.size() / 3, 12, n->ref_tris.data(), n_tris, pose, &cov, &s);
    if (rc != HFPF_OK) return rc;
    FILE* f = fopen((n->directory_name + "/coverage.csv").c_str(), "w");
    if (!f) rc = HFPF_ERR_IO;
    if (f) {
        fprintf(f, "tri,n_samples,n_in_bbox,n_covered,flags,area,max_distance,sum_dist_q30\n");
        for (uint64_t k = 0; k < n_tris; k++) {
            const hfpf_tri_coverage& c = cov[k];
            fprintf(f, "%llu,%u,%u,%u,%u,%.9g,%.9g,%lld\n", (unsigned long long)k, c.n_samples, c.n_in_bbox, c.n_covered, c.flags, c.area, c.max_distance,
                    (long long)c.sum_dist_q30);
        }
        const bool ok = !ferror(f);
        if (fclose(f) != 0 || !ok) rc = HFPF_ERR_IO;
    }
    if (rc == HFPF_OK) {
        f = fopen((n->directory_name + "/coverage_summary.csv").c_str(), "w");
        if (!f) rc = HFPF_ERR_IO;
        else {
            fprintf(f, "n_tris_valid,n_tris_invalid,n_tris_huge,n_samples,n_in_bbox,n_covered,sum_dist_q30,area_q40_lo,area_q40_hi,covered_q40_lo,"
                       "covered_q40_hi,max_distance\n%llu,%llu,%llu,%llu,%llu,%llu,%lld,%llu,%llu,%llu,%llu,%.9g\n",
                    (unsigned long long)s.n_tris_valid, (unsigned long long)s.n_tris_invalid, (unsigned long long)s.n_tris_huge, (unsigned long long)s.n_samples,
                    (unsigned long long)s.n_in_bbox, (unsigned long long)s.n_covered, (long long)s.sum_dist_q30, (unsigned long long)s.area_q40_lo,
                    (unsigned long long)s.area_q40_hi, (unsigned long long)s.covered_q40_lo, (unsigned long long)s.covered_q40_hi, s.max_distance);
            const bool ok = !ferror(f);
            if (fclose(f) != 0 || !ok) rc = HFPF_ERR_IO;
        }
    }
    hfpf_free_coverage(cov);
    return rc;
}

// view_plan.csv and view_plan_summary.csv beside the cloud: hfpf_plan_views of the reference mesh at `pose`, the pose the deviation
// files were written at, for the candidate views; one line per view.  A component filter's min_count replaces the cover's, as it does
// for the coverage files.
static int write_view_plan(hfpf_node* n, const double pose[12])
{
    hfpf_plan_opts o = n->plan_opts;
    if (n->comp_rows) o.cover.min_count = n->comp_opts.min_count;
    const uint32_t n_views = (uint32_t)(n->plan_poses.size() / 12);
    std::vector<hfpf_view_score> sc(std::max<uint32_t>(n_views, 1));
    hfpf_plan_summary s;
    int rc = hfpf_plan_views(n->grid, &o, n->ref_verts.data(), n->ref_verts.size() / 3, 12, n->ref_tris.data(), n->ref_tris.size() / 3, pose,
                             n->plan_poses.data(), n_views, sc.data(), nullptr, &s);
    if (rc != HFPF_OK) return rc;
    FILE* f = fopen((n->directory_name + "/view_plan.csv").c_str(), "w");
    if (!f) return HFPF_ERR_IO;
    fprintf(f, "view,rank,n_in_view,n_facing,n_visible,visible_q40,gain_q40,gain_samples\n");
    for (uint32_t v = 0; v < n_views; v++)
        fprintf(f, "%u,%d,%u,%u,%u,%llu,%llu,%llu\n", v, sc[v].rank, sc[v].n_in_view, sc[v].n_facing, sc[v].n_visible, (unsigned long long)sc[v].visible_q40,
                (unsigned long long)sc[v].gain_q40, (unsigned long long)sc[v].gain_samples);
    bool ok = !ferror(f);
    if (fclose(f) != 0 || !ok) return HFPF_ERR_IO;
    f = fopen((n->directory_name + "/view_plan_summary.csv").c_str(), "w");
    if (!f) return HFPF_ERR_IO;
    fprintf(f, "n_views,n_selected,n_targets,n_reachable,n_planned,target_q40,reachable_q40,planned_q40,n_samples,n_in_bbox,n_covered\n"
               "%u,%u,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu\n",
            s.n_views, s.n_selected, (unsigned long long)s.n_targets, (unsigned long long)s.n_reachable, (unsigned long long)s.n_planned,
            (unsigned long long)s.target_q40, (unsigned long long)s.reachable_q40, (unsigned long long)s.planned_q40,
            (unsigned long long)s.coverage.n_samples, (unsigned long long)s.coverage.n_in_bbox, (unsigned long long)s.coverage.n_covered);
    ok = !ferror(f);
    return fclose(f) != 0 || !ok ? HFPF_ERR_IO : HFPF_OK;
}

// consistency.csv and consistency_summary.csv beside the cloud: hfpf_depth_consistency of the depth images in the ring, one line per
// saved row.  Built like the deviation files: the call runs on the full row set (with the component filter's min_count when one is
// set, and never with HFPF_CONSISTENCY_DROP: this is a report), one walk selects the saved rows' records, and under a filter the
// summary is rebuilt from the selected records as include/hfpf.h defines it.
static int write_consistency(hfpf_node* n, const hfpf_row* saved, uint64_t n_saved)
{
    hfpf_consistency_opts o;
    hfpf_depth_image desc;
    std::vector<uint8_t> frames;
    std::vector<double> poses;
    uint64_t stride = 0;
    uint32_t n_frames = 0;
    {
        std::lock_guard<std::mutex> lk(n->cons_mtx);
        o = n->cons_opts;
        desc = n->cons_desc;
        poses = n->cons_poses;
        n_frames = (uint32_t)n->cons_frames.size();
        stride = n_frames ? n->cons_frames[0].size() : 0;  // a whole number of samples: depth_step is one
        frames.resize((size_t)stride * n_frames);
        for (uint32_t f = 0; f < n_frames; f++) memcpy(frames.data() + (size_t)f * stride, n->cons_frames[f].data(), stride);
    }
    o.flags &= ~HFPF_CONSISTENCY_DROP;
    if (n->comp_rows) o.min_count = n->comp_opts.min_count;
    if (n_frames == 0) {  // nothing seen yet: any valid descriptor serves a call without frames
        memset(&desc, 0, sizeof desc);
        desc.struct_size = sizeof desc;
        desc.width = desc.height = 1, desc.depth_format = HFPF_DEPTH_U16, desc.depth_step = 2, desc.depth_scale = 0.001f;
        desc.fx = desc.fy = 1.0;
    }
    hfpf_row* all = nullptr;
    hfpf_row_consistency* cons = nullptr;
    uint64_t n_all = 0;
    hfpf_consistency_summary s;
    int rc = hfpf_depth_consistency(n->grid, &o, &desc, frames.data(), stride, n_frames, poses.data(), n->comp_rows ? &all : nullptr, &cons, &n_all, &s);
    if (rc != HFPF_OK) return rc;
    FILE* f = fopen((n->directory_name + "/consistency.csv").c_str(), "w");
    if (!f) rc = HFPF_ERR_IO;
    if (f) {
        fprintf(f, "ix,iy,iz,n_in_view,n_tested,n_support,n_through,n_occluded,first_through,flags\n");
        if (n->comp_rows) memset(&s, 0, sizeof s);
        uint64_t j = 0;
        for (uint64_t i = 0; i < n_saved && rc == HFPF_OK; i++) {
            const hfpf_row& r = saved[i];
            if (n->comp_rows)
                while (j < n_all && (all[j].ix != r.ix || all[j].iy != r.iy || all[j].iz != r.iz)) j++;
            else j = i;
            if (j >= n_all) {
                rc = HFPF_ERR_STATE;  // cannot happen: both row sets come from one state of the grid
                break;
            }
            const hfpf_row_consistency& c = cons[j];
            fprintf(f, "%d,%d,%d,%u,%u,%u,%u,%u,%u,%u\n", r.ix, r.iy, r.iz, c.n_in_view, c.n_tested, c.n_support, c.n_through, c.n_occluded, c.first_through,
                    c.flags);
            if (n->comp_rows) {
                s.n_rows++;
                s.n_seen += (c.flags & HFPF_CONS_SEEN) ? 1 : 0;
                s.n_supported += (c.flags & HFPF_CONS_SUPPORTED) ? 1 : 0;
                s.n_contradicted += (c.flags & HFPF_CONS_CONTRADICTED) ? 1 : 0;
                s.pairs_tested += c.n_tested, s.pairs_support += c.n_support, s.pairs_through += c.n_through;
            }
        }
        if (n->comp_rows) s.n_kept = s.n_rows - s.n_contradicted;
        const bool ok = !ferror(f);
        if (fclose(f) != 0 || !ok) rc = rc == HFPF_OK ? HFPF_ERR_IO : rc;
    }
    if (rc == HFPF_OK) {
        f = fopen((n->directory_name + "/consistency_summary.csv").c_str(), "w");
        if (!f) rc = HFPF_ERR_IO;
        else {
            fprintf(f, "n_rows,n_seen,n_supported,n_contradicted,n_kept,pairs_tested,pairs_support,pairs_through\n%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu\n",
                    (unsigned long long)s.n_rows, (unsigned long long)s.n_seen, (unsigned long long)s.n_supported, (unsigned long long)s.n_contradicted,
                    (unsigned long long)s.n_kept, (unsigned long long)s.pairs_tested, (unsigned long long)s.pairs_support, (unsigned long long)s.pairs_through);
            const bool ok = !ferror(f);
            if (fclose(f) != 0 || !ok) rc = HFPF_ERR_IO;
        }
    }
    hfpf_free_consistency(all, cons);
    return rc;
}

// sections.csv and section_summary.csv beside mesh.ply: hfpf_section_mesh of the mesh that file holds (identity pose) with the node's
// planes; one line per segment, then one line per plane.
static int write_sections(hfpf_node* n, const hfpf_mesh_vertex* mv, uint64_t nmv, const uint32_t* mt, uint64_t nmt)
{
    const double ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const uint32_t n_planes = (uint32_t)(n->sec_planes.size() / 4);
    hfpf_section_point* pts = nullptr;
    hfpf_section_segment* segs = nullptr;
    hfpf_section_contour* conts = nullptr;
    uint64_t np = 0, ns = 0, nc = 0;
    std::vector<hfpf_section_plane> recs(n_planes);
    hfpf_section_summary s;
    int rc = hfpf_section_mesh(n->grid, &n->sec_opts, mv, nmv, sizeof(hfpf_mesh_vertex), mt, nmt, ident, n->sec_planes.data(), n_planes, &pts, &np, &segs, &ns,
                               &conts, &nc, recs.data(), &s);
    if (rc != HFPF_OK) return rc;
    FILE* f = fopen((n->directory_name + "/sections.csv").c_str(), "w");
    if (!f) rc = HFPF_ERR_IO;
    else {
        fprintf(f, "plane,contour,tri,x0,y0,z0,x1,y1,z1\n");
        for (uint64_t i = 0; i < ns; i++) {
            const hfpf_section_point &a = pts[segs[i].p0], &b = pts[segs[i].p1];
            fprintf(f, "%u,%u,%u,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g\n", a.plane, segs[i].contour, segs[i].tri, a.x, a.y, a.z, b.x, b.y, b.z);
        }
        const bool ok = !ferror(f);
        if (fclose(f) != 0 || !ok) rc = HFPF_ERR_IO;
    }
    if (rc == HFPF_OK) {
        f = fopen((n->directory_name + "/section_summary.csv").c_str(), "w");
        if (!f) rc = HFPF_ERR_IO;
        else {
            fprintf(f, "plane,first_segment,n_segments,first_point,n_points,first_contour,n_contours,n_closed,n_branched,length_q32,area_q28\n");
            for (uint32_t j = 0; j < n_planes; j++) {
                const hfpf_section_plane& r = recs[j];
                fprintf(f, "%u,%u,%u,%u,%u,%u,%u,%u,%u,%lld,%lld\n", j, r.first_segment, r.n_segments, r.first_point, r.n_points, r.first_contour, r.n_contours,
                        r.n_closed, r.n_branched, (long long)r.length_q32, (long long)r.area_q28);
            }
            const bool ok = !ferror(f);
            if (fclose(f) != 0 || !ok) rc = HFPF_ERR_IO;
        }
    }
    hfpf_free_section(pts, segs, conts);
    return rc;
}

// mesh_edges.csv, mesh_loops.csv, mesh_shells.csv and mesh_topology_summary.csv beside mesh.ply: hfpf_mesh_topology_device of the mesh
// that file holds (the same options extract the same mesh), read in HBM where hfpf_extract_mesh_device leaves it, identity pose.
static int write_topology(hfpf_node* n)
{
    const double ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    hfpf_mesh_vertex* dv = nullptr;
    uint32_t* dt = nullptr;
    uint64_t nv = 0, nt = 0, ne = 0, nl = 0, ns = 0;
    hfpf_topology_edge* de = nullptr;
    hfpf_topology_loop* dl = nullptr;
    hfpf_topology_shell* ds = nullptr;
    hfpf_topology_summary s;
    int rc = hfpf_extract_mesh_device(n->grid, &n->mesh_opts, &dv, &nv, &dt, &nt);
    if (rc == HFPF_OK) rc = hfpf_mesh_topology_device(n->grid, &n->top_opts, dv, nv, sizeof(hfpf_mesh_vertex), dt, nt, ident, &de, &ne, &dl, &nl, &ds, &ns, nullptr, &s);
    std::vector<hfpf_topology_edge> edges(rc == HFPF_OK ? ne : 0);
    std::vector<hfpf_topology_loop> loops(rc == HFPF_OK ? nl : 0);
    std::vector<hfpf_topology_shell> shells(rc == HFPF_OK ? ns : 0);
    if (rc == HFPF_OK && ne) rc = hfpf_device_download(n->grid, edges.data(), de, ne * sizeof(hfpf_topology_edge));
    if (rc == HFPF_OK && nl) rc = hfpf_device_download(n->grid, loops.data(), dl, nl * sizeof(hfpf_topology_loop));
    if (rc == HFPF_OK && ns) rc = hfpf_device_download(n->grid, shells.data(), ds, ns * sizeof(hfpf_topology_shell));
    for (void* p : {(void*)dv, (void*)dt, (void*)de, (void*)dl, (void*)ds})
        if (p) hfpf_device_free(n->grid, p);
    if (rc != HFPF_OK) return rc;
    auto finish = [](FILE* f) { return ferror(f) | fclose(f) ? HFPF_ERR_IO : HFPF_OK; };
    FILE* f = fopen((n->directory_name + "/mesh_edges.csv").c_str(), "w");
    if (!f) return HFPF_ERR_IO;
    fprintf(f, "p0,p1,tri,kind,uses,loop,shell\n");
    for (const hfpf_topology_edge& e : edges) fprintf(f, "%u,%u,%u,%u,%u,%u,%u\n", e.p0, e.p1, e.tri, e.kind, e.uses, e.loop, e.shell);
    if ((rc = finish(f))) return rc;
    if (!(f = fopen((n->directory_name + "/mesh_loops.csv").c_str(), "w"))) return HFPF_ERR_IO;
    fprintf(f, "loop,first_vertex,n_verts,n_edges,n_ends,flags,shell,length_q32,area_q28_x,area_q28_y,area_q28_z\n");
    for (uint64_t i = 0; i < nl; i++) {
        const hfpf_topology_loop& l = loops[i];
        fprintf(f, "%llu,%u,%u,%u,%u,%u,%u,%lld,%lld,%lld,%lld\n", (unsigned long long)i, l.first_vertex, l.n_verts, l.n_edges, l.n_ends, l.flags, l.shell,
                (long long)l.length_q32, (long long)l.area_q28[0], (long long)l.area_q28[1], (long long)l.area_q28[2]);
    }
    if ((rc = finish(f))) return rc;
    if (!(f = fopen((n->directory_name + "/mesh_shells.csv").c_str(), "w"))) return HFPF_ERR_IO;
    fprintf(f, "shell,first_vertex,n_verts,n_tris,flags,n_edges,n_boundary,n_nonmanifold,n_miswound,n_loops,area_q32,volume_q40\n");
    for (uint64_t i = 0; i < ns; i++) {
        const hfpf_topology_shell& h = shells[i];
        fprintf(f, "%llu,%u,%u,%u,%u,%u,%u,%u,%u,%u,%lld,%lld\n", (unsigned long long)i, h.first_vertex, h.n_verts, h.n_tris, h.flags, h.n_edges, h.n_boundary,
                h.n_nonmanifold, h.n_miswound, h.n_loops, (long long)h.area_q32, (long long)h.volume_q40);
    }
    if ((rc = finish(f))) return rc;
    if (!(f = fopen((n->directory_name + "/mesh_topology_summary.csv").c_str(), "w"))) return HFPF_ERR_IO;
    fprintf(f, "n_tris_valid,n_tris_invalid,n_tris_far,n_verts_used,n_edges,n_interior,n_boundary,n_nonmanifold,n_miswound,n_loops,n_closed_loops,n_shells,"
               "n_watertight\n");
    const uint64_t w[13] = {s.n_tris_valid, s.n_tris_invalid, s.n_tris_far, s.n_verts_used, s.n_edges, s.n_interior, s.n_boundary,
                            s.n_nonmanifold, s.n_miswound, s.n_loops, s.n_closed_loops, s.n_shells, s.n_watertight};
    for (int i = 0; i < 13; i++) fprintf(f, "%llu%c", (unsigned long long)w[i], i == 12 ? '\n' : ',');
    return finish(f);
}

int hfpf_node_process(hfpf_node* n, hfpf_trigger_response* res)
{
    if (!n) return HFPF_ERR_BAD_ARG;
    n->process_calls++;
    if (n->top_on && !n->mesh_on) {  // EXTENSION: the topology is that of the mesh of mesh.ply; nothing is written and the grid is kept
        const std::string m = "mesh topology is set but mesh output is not (hfpf_node_set_mesh_output)";
        set_res(res, false, m);
        return nfail(n, HFPF_ERR_STATE, m);
    }
    if (n->sec_on && !n->mesh_on) {  // EXTENSION: the sections cut the mesh of mesh.ply; nothing is written and the grid is kept
        const std::string m = "section planes are set but mesh output is not (hfpf_node_set_mesh_output)";
        set_res(res, false, m);
        return nfail(n, HFPF_ERR_STATE, m);
    }
    // The reference polls until both queues are empty (node.cpp:380-394); integrate calls are already in stream order here.
    if (n->final_clean && hfpf_is_dirty(n->grid) > 0) {
        int rc = hfpf_clean(n->grid);
        if (rc != HFPF_OK) {
            set_res(res, false, hfpf_last_error(n->grid));
            return nfail(n, rc, hfpf_last_error(n->grid));
        }
        n->clean_passes++;
    }
    const std::string cloud_location = n->directory_name + "/test_cloud.pcd";  // node.cpp:395
    const std::string meta_location = n->directory_name + "/meta.csv";         // node.cpp:396
    hfpf_row* rows = nullptr;
    uint64_t nr = 0;
    uint32_t* labels = nullptr;
    hfpf_component* comps = nullptr;
    uint64_t ncomp = 0;
    int rc = HFPF_OK;
    n->comp_rows = n->comp_on && !n->hide_filtered;
    if (n->comp_on && n->hide_filtered) {
        // EXTENSION: the filter runs in HBM and what it drops is hidden (HFPF_HIDE_OTHERS on the kept rows, read in place): from here
        // on this is a node without a component filter whose every file leaves those rows out.  hfpf_clear below empties the set.
        hfpf_row* d_rows = nullptr;
        uint32_t* d_labels = nullptr;
        hfpf_component* d_comps = nullptr;
        uint64_t n_kept = 0;
        rc = hfpf_extract_components_device(n->grid, &n->comp_opts, &d_rows, &d_labels, &n_kept, &d_comps, &ncomp);
        if (rc == HFPF_OK) {
            hfpf_hide_opts ho;
            memset(&ho, 0, sizeof ho);
            ho.struct_size = sizeof ho;
            ho.op = HFPF_HIDE_OTHERS;
            rc = hfpf_hide_voxels_device(n->grid, &ho, d_rows, n_kept, sizeof(hfpf_row), nullptr, 0, nullptr);
        }
        for (void* p : {(void*)d_rows, (void*)d_labels, (void*)d_comps})
            if (p) hfpf_device_free(n->grid, p);
    }
    if (rc == HFPF_OK)
        rc = n->comp_rows ? hfpf_extract_components(n->grid, &n->comp_opts, &rows, &labels, &nr, &comps, &ncomp)  // EXTENSION: without the specks
                          : hfpf_extract(n->grid, &rows, &nr);                                                  // grid_.downloadData, node.cpp:398
    if (rc == HFPF_OK) rc = hfpf_write_pcd(rows, nr, cloud_location.c_str());
    if (rc == HFPF_OK) rc = hfpf_write_meta_csv(rows, nr, meta_location.c_str());
    if (rc == HFPF_OK && n->publish) n->publish(n->publish_user, rows, nr, n->fusion_frame.c_str());  // processed_cloud_, node.cpp:158
    double ref_pose[12];
    if (rc == HFPF_OK && n->ref_on) rc = write_deviation(n, rows, nr, ref_pose);  // EXTENSION: the saved cloud measured against the reference mesh
    if (rc == HFPF_OK && n->ref_on && n->cover_on) rc = write_coverage(n, ref_pose);  // EXTENSION: ... and how much of that mesh the model covers
    if (rc == HFPF_OK && n->ref_on && n->plan_on) rc = write_view_plan(n, ref_pose);  // EXTENSION: ... and from where to scan what it does not
    if (rc == HFPF_OK && n->cons_on) rc = write_consistency(n, rows, nr);  // EXTENSION: what the last depth images say about every saved row
    if (n->comp_rows) hfpf_free_components(rows, labels, comps);
    else hfpf_free_rows(rows);
    if (rc == HFPF_OK && n->mesh_on) {  // EXTENSION: a triangle mesh of the same model next to the cloud
        hfpf_mesh_vertex* mv = nullptr;
        uint32_t* mt = nullptr;
        uint64_t nmv = 0, nmt = 0;
        rc = hfpf_extract_mesh(n->grid, &n->mesh_opts, &mv, &nmv, &mt, &nmt);
        if (rc == HFPF_OK) rc = hfpf_write_ply(mv, nmv, mt, nmt, (n->directory_name + "/mesh.ply").c_str());
        if (rc == HFPF_OK && n->sec_on) rc = write_sections(n, mv, nmv, mt, nmt);  // EXTENSION: ... and its profiles in the node's planes
        hfpf_free_mesh(mv, mt);
        if (rc == HFPF_OK && n->top_on) rc = write_topology(n);  // EXTENSION: ... and its open edges, loops and shells
    }
    if (rc == HFPF_OK && n->write_variants) {  // the reference's `#if 0` block, node.cpp:399-437
        struct Variant {
            const char* file;
            double min_count;
            int classify;
            int white;
        };
        const Variant vs[] = {{"test_cloud_50.pcd", 50, -1, 1},   {"test_cloud_100.pcd", 100, -1, 1}, {"test_cloud_150.pcd", 150, -1, 1},
                              {"test_cloud_200.pcd", 200, -1, 1}, {"test_cloud_250.pcd", 250, -1, 1}, {"test_cloud_300.pcd", 300, -1, 1},
                              {"test_cloud_classified.pcd", 0, 100 /* kGoodPointsThreshold, grid.hpp:34 */, 0}};
        for (const Variant& v : vs) {
            hfpf_extract_opts o;
            memset(&o, 0, sizeof o);
            o.struct_size = sizeof o;
            o.min_count = v.min_count;
            o.classify_threshold = v.classify;
            o.paint_white = v.white;
            hfpf_row* vr = nullptr;
            uint64_t vn = 0;
            rc = hfpf_extract_filtered(n->grid, &o, &vr, &vn);  // filtered and colour-coded on the device
            if (rc == HFPF_OK) rc = hfpf_write_pcd_xyzrgb(vr, vn, (n->directory_name + "/" + v.file).c_str(), 0, -1, 0);
            hfpf_free_rows(vr);
            if (rc != HFPF_OK) break;
        }
        if (rc == HFPF_OK) {  // download(PointXYZRGBNormal), grid.hpp:577-601
            hfpf_row* vr = nullptr;
            uint64_t vn = 0;
            rc = hfpf_extract(n->grid, &vr, &vn);
            if (rc == HFPF_OK) rc = hfpf_write_pcd(vr, vn, (n->directory_name + "/test_cloud_normals.pcd").c_str());
            hfpf_free_rows(vr);
        }
    }
    if (rc != HFPF_OK) {
        std::string m = rc == HFPF_ERR_IO ? "cannot write " + cloud_location + " / " + meta_location : std::string(hfpf_last_error(n->grid));
        // The reference ends getFusedCloud with grid_.clearVoxels() whatever happened before (node.cpp:438).  An engine failure
        // (capacity overflow, poisoned handle) leaves nothing worth keeping and hfpf_clear is the only way out of that state, so
        // the grid is cleared here too and the node can capture again without a restart; after an I/O error the fused data is
        // intact and kept, so that ~process can be repeated once the directory is writable.
        if (rc != HFPF_ERR_IO) {
            if (hfpf_clear(n->grid) == HFPF_OK) m += " (grid cleared)";
        }
        set_res(res, false, m);
        return nfail(n, rc, m);
    }
    rc = hfpf_clear(n->grid);  // grid_.clearVoxels(), node.cpp:438
    if (rc != HFPF_OK) {
        set_res(res, false, hfpf_last_error(n->grid));
        return nfail(n, rc, hfpf_last_error(n->grid));
    }
    forget_depth(n);  // the images in the ring belong to the session that was just saved and cleared
    char m[200];
    snprintf(m, sizeof m, "saved %llu points", (unsigned long long)nr);
    set_res(res, true, std::string(m) + " to " + cloud_location);
    return HFPF_OK;
}

int hfpf_node_set_mesh_output(hfpf_node* n, const hfpf_mesh_opts* opts)
{
    if (!n) return HFPF_ERR_BAD_ARG;
    if (opts) {
        if (hfpf_check_mesh_opts(opts) != HFPF_OK) return nfail(n, HFPF_ERR_BAD_ARG, "hfpf_node_set_mesh_output: invalid hfpf_mesh_opts");
        n->mesh_opts = *opts;
    }
    n->mesh_on = opts != nullptr;
    return HFPF_OK;
}

int hfpf_node_set_section_planes(hfpf_node* n, const hfpf_section_opts* opts, const double* planes, uint32_t n_planes)
{
    if (!n) return HFPF_ERR_BAD_ARG;
    if (opts) {
        bool ok = hfpf_check_section_opts(opts) == HFPF_OK && n_planes <= HFPF_SECTION_MAX_PLANES && (planes || !n_planes);
        for (uint32_t j = 0; ok && j < n_planes; j++) {
            const double* p = planes + 4ull * j;
            const double nn = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
            ok = std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(p[3]) && std::isfinite(nn) && nn > 0.0;
        }
        if (!ok) return nfail(n, HFPF_ERR_BAD_ARG, "hfpf_node_set_section_planes: invalid hfpf_section_opts, more than 4096 planes, or a plane that is not finite");
        n->sec_opts = *opts;
        n->sec_planes.assign(planes, planes + 4ull * n_planes);
    } else {
        n->sec_planes.clear();
    }
    n->sec_on = opts != nullptr;
    return HFPF_OK;
}

int hfpf_node_set_mesh_topology(hfpf_node* n, const hfpf_topology_opts* opts)
{
    if (!n) return HFPF_ERR_BAD_ARG;
    if (opts) {
        if (hfpf_check_topology_opts(opts) != HFPF_OK) return nfail(n, HFPF_ERR_BAD_ARG, "hfpf_node_set_mesh_topology: invalid hfpf_topology_opts");
        n->top_opts = *opts;
    }
    n->top_on = opts != nullptr;
    return HFPF_OK;
}

int hfpf_node_set_component_filter(hfpf_node* n, const hfpf_component_opts* opts)
{
    if (!n) return HFPF_ERR_BAD_ARG;
    if (opts) {
        if (hfpf_check_component_opts(opts) != HFPF_OK)
            return nfail(n, HFPF_ERR_BAD_ARG, "hfpf_node_set_component_filter: invalid hfpf_component_opts");
        n->comp_opts = *opts;
    }
    n->comp_on = opts != nullptr;
    return HFPF_OK;
}

int hfpf_node_set_hide_filtered(hfpf_node* n, int on)
{
    if (!n) return HFPF_ERR_BAD_ARG;
    n->hide_filtered = on != 0;
    return HFPF_OK;
}

int hfpf_node_hide_box(hfpf_node* n, uint32_t op, const double box_m[6], hfpf_hide_result* res)
{
    if (!n) return HFPF_ERR_BAD_ARG;
    if (!box_m) return nfail(n, HFPF_ERR_BAD_ARG, "hfpf_node_hide_box: NULL box");
    int32_t dims[3], lo[3], hi[3];
    double resolution = 0.0;
    int rc = hfpf_get_dims(n->grid, dims, &resolution);
    if (rc != HFPF_OK) return nfail(n, rc, hfpf_last_error(n->grid));
    for (int a = 0; a < 3; a++) {
        int32_t* out[2] = {&lo[a], &hi[a]};
        for (int k = 0; k < 2; k++) {
            const double v = floor((box_m[2 * a + k] - n->bbox_min[a]) / resolution);  // voxel = floor((p - bbox_min) / res), the query contract
            if (std::isnan(v)) return nfail(n, HFPF_ERR_BAD_ARG, "hfpf_node_hide_box: a bound is not a number");
            *out[k] = v < -2147483648.0 ? INT32_MIN : v > 2147483647.0 ? INT32_MAX : (int32_t)v;
        }
    }
    rc = hfpf_hide_box(n->grid, op, lo, hi, res);  // (takes the grid's lock: frames and clean passes fall before or after it)
    return rc == HFPF_OK ? rc : nfail(n, rc, hfpf_last_error(n->grid));
}

int hfpf_node_set_reference_mesh(hfpf_node* n, const hfpf_deviation_opts* opts, const void* verts, uint64_t n_verts, uint32_t vertex_stride,
                                 const uint32_t* tris, uint64_t n_tris, const double* pose_3x4)
{
    if (!n) return HFPF_ERR_BAD_ARG;
    if (!opts) {
        n->ref_on = false;
        n->ref_verts.clear(), n->ref_tris.clear();
        return HFPF_OK;
    }
    bool ok = hfpf_check_deviation_opts(opts) == HFPF_OK && pose_3x4 && vertex_stride >= 12 && (vertex_stride & 3) == 0 && (verts || !n_verts) &&
              (tris || !n_tris) && n_verts < 0xFFFFFFFFull && n_tris < 0xFFFFFFFFull;
    for (int i = 0; ok && i < 12; i++) ok = std::isfinite(pose_3x4[i]);
    if (!ok) return nfail(n, HFPF_ERR_BAD_ARG, "hfpf_node_set_reference_mesh: invalid options, mesh or pose");
    std::vector<float> v(3 * n_verts);
    for (uint64_t i = 0; i < n_verts; i++) memcpy(&v[3 * i], (const char*)verts + i * vertex_stride, 12);
    n->ref_verts.swap(v);
    n->ref_tris.assign(tris, tris + 3 * n_tris);
    memcpy(n->ref_pose, pose_3x4, sizeof n->ref_pose);
    n->ref_opts = *opts;
    n->ref_on = true;
    return HFPF_OK;
}

int hfpf_node_set_reference_alignment(hfpf_node* n, const hfpf_align_opts* opts)
{
    if (!n) return HFPF_ERR_BAD_ARG;
    if (opts) {
        if (hfpf_check_align_opts(opts) != HFPF_OK) return nfail(n, HFPF_ERR_BAD_ARG, "hfpf_node_set_reference_alignment: invalid hfpf_align_opts");
        n->align_opts = *opts;
    }
    n->align_on = opts != nullptr;
    return HFPF_OK;
}

int hfpf_node_set_reference_coverage(hfpf_node* n, const hfpf_cover_opts* opts)
{
    if (!n) return HFPF_ERR_BAD_ARG;
    if (opts) {
        if (hfpf_check_cover_opts(opts) != HFPF_OK) return nfail(n, HFPF_ERR_BAD_ARG, "hfpf_node_set_reference_coverage: invalid hfpf_cover_opts");
        n->cover_opts = *opts;
    }
    n->cover_on = opts != nullptr;
    return HFPF_OK;
}

int hfpf_node_set_view_candidates(hfpf_node* n, const hfpf_plan_opts* opts, const double* poses, uint32_t n_views)
{
    if (!n) return HFPF_ERR_BAD_ARG;
    if (opts) {
        bool ok = hfpf_check_plan_opts(opts) == HFPF_OK && n_views <= 4096 && (poses || !n_views);
        for (uint64_t i = 0; ok && i < 12ull * n_views; i++) ok = std::isfinite(poses[i]);
        if (!ok) return nfail(n, HFPF_ERR_BAD_ARG, "hfpf_node_set_view_candidates: invalid hfpf_plan_opts, more than 4096 views, or NULL or non-finite poses");
        n->plan_opts = *opts;
        n->plan_poses.assign(poses, poses + 12ull * n_views);
    }
    n->plan_on = opts != nullptr;
    return HFPF_OK;
}

int hfpf_node_set_depth_consistency(hfpf_node* n, const hfpf_consistency_opts* opts, uint32_t keep_frames)
{
    if (!n) return HFPF_ERR_BAD_ARG;
    if (opts && (hfpf_check_consistency_opts(opts) != HFPF_OK || keep_frames < 1 || keep_frames > 4096))
        return nfail(n, HFPF_ERR_BAD_ARG, "hfpf_node_set_depth_consistency: invalid hfpf_consistency_opts, or keep_frames outside 1..4096");
    std::lock_guard<std::mutex> lk(n->cons_mtx);
    if (opts) n->cons_opts = *opts, n->cons_keep = keep_frames;
    n->cons_on = opts != nullptr;
    if (!opts) n->cons_frames.clear(), n->cons_poses.clear();
    while (n->cons_frames.size() > n->cons_keep) {  // a smaller ring keeps the newest
        n->cons_frames.erase(n->cons_frames.begin());
        n->cons_poses.erase(n->cons_poses.begin(), n->cons_poses.begin() + 12);
    }
    return HFPF_OK;
}

int hfpf_node_save_session(hfpf_node* n, const char* path)
{
    if (!n || !path) return HFPF_ERR_BAD_ARG;
    const int rc = hfpf_save(n->grid, path);  // (takes the grid's lock: frames and clean passes fall before or after it)
    return rc == HFPF_OK ? rc : nfail(n, rc, hfpf_last_error(n->grid));
}

int hfpf_node_load_session(hfpf_node* n, const char* path)
{
    if (!n || !path) return HFPF_ERR_BAD_ARG;
    const int rc = hfpf_load(n->grid, path);  // start_ / cloud_subscription_started_ and the node's counters stay as they are
    forget_depth(n);                          // the images in the ring were not fused into the loaded session (nor into what a failed load leaves)
    return rc == HFPF_OK ? rc : nfail(n, rc, hfpf_last_error(n->grid));
}

int hfpf_node_set_publisher(hfpf_node* n, hfpf_publish_fn fn, void* user)
{
    if (!n) return HFPF_ERR_BAD_ARG;
    n->publish = fn;
    n->publish_user = user;
    return HFPF_OK;
}

int hfpf_node_clean_now(hfpf_node* n)
{
    if (!n) return HFPF_ERR_BAD_ARG;
    if (hfpf_is_dirty(n->grid) <= 0) return 0;
    int rc = hfpf_clean(n->grid);
    if (rc != HFPF_OK) return nfail(n, rc, hfpf_last_error(n->grid));
    n->clean_passes++;
    return 1;
}

hfpf_handle* hfpf_node_grid(hfpf_node* n) { return n ? n->grid : nullptr; }

int hfpf_node_get_stats(hfpf_node* n, hfpf_node_stats* out)
{
    if (!n || !out) return HFPF_ERR_BAD_ARG;
    out->received = n->received;
    out->integrated = n->integrated;
    out->dropped_not_started = n->dropped_not_started;
    out->dropped_tf = n->dropped_tf;
    out->clean_passes = n->clean_passes;
    out->process_calls = n->process_calls;
    out->started = n->start_ ? 1 : 0;
    out->cloud_subscription_started = n->cloud_subscription_started_ ? 1 : 0;
    return HFPF_OK;
}

}  // extern "C"
