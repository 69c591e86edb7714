// examples/hfpf_demo.cpp -- a C++-only run of the whole path through the node shell (no Python, no ROS):
// synthetic sensor -> ~start -> N x PointCloud2 callbacks with tf poses -> periodic clean -> ~process ->
// <dir>/test_cloud.pcd + <dir>/meta.csv.  Prints per-stage wall times.
//
//   hfpf_demo [--mesh-topology] [--section planes.txt] [--min-component N [--hide-filtered]] [--reference mesh.ply [--max-deviation metres] [--align] [--coverage [spacing]] [--plan poses.txt]] <out_dir> [frames=30] [W=640] [H=480] [resolution=0.001] [clean_every=10] [seed=0xF051] [pose_seed=0x5E3]
// --section planes.txt: ~process also writes mesh.ply (hfpf_node_set_mesh_output: a window of 2 voxels) and cuts that mesh with the
//   planes in planes.txt (four numbers per plane, n.x n.y n.z d in the fusion frame, separated by white space;
//   hfpf_node_set_section_planes): sections.csv and section_summary.csv, and the demo prints every plane's contours, length and area.
// --mesh-topology: ~process also writes mesh.ply (as --section does) and the open edges, boundary loops and shells of that mesh
//   (hfpf_node_set_mesh_topology): mesh_edges.csv, mesh_loops.csv, mesh_shells.csv and mesh_topology_summary.csv, and the demo prints
//   the summary and the five longest loops.
// --min-component N: ~process saves only the connected components (26-neighbourhood) of at least N rows (hfpf_node_set_component_filter).
//   --hide-filtered: the rows the filter drops are hidden on the device (hfpf_node_set_hide_filtered), so that the reports of --reference
//   see the cleaned model too, not only test_cloud.pcd and meta.csv.
// --reference mesh.ply: ~process also writes deviation.csv and deviation_summary.csv, the saved cloud measured against that mesh
//   (binary little-endian PLY in the fusion frame; hfpf_node_set_reference_mesh); --max-deviation is the largest distance looked for
//   (default 10 voxels, at most 32).  --align: the mesh is first best-fitted to the model from that pose with the same distance as its
//   capture range (hfpf_node_set_reference_alignment); the compare runs at the refined pose, which alignment.csv records.
//   --coverage [spacing]: ~process also writes coverage.csv and coverage_summary.csv, how much of that mesh the model has rows near
//   (hfpf_node_set_reference_coverage: samples `spacing` metres apart, one voxel by default, a window of 2 voxels, rows within 2
//   voxels), and the demo prints the covered share of the mesh's area and of its samples.  A number behind --coverage is the spacing
//   only when another argument follows it (the output directory).
//   --plan poses.txt: ~process also writes view_plan.csv and view_plan_summary.csv, which of the candidate camera poses in poses.txt
//   (12 numbers per pose, row-major [R|t], camera -> fusion frame, separated by white space) would see the most of that mesh not
//   yet scanned (hfpf_node_set_view_candidates: the coverage settings above, a 640 x 480 sensor of 525 px focal length between 0.3 and
//   3 m, up to 8 views), and the demo prints the selected views in rank order.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hfpf_node.h"

extern "C" {
void hfpf_synth_pose(uint64_t seed, uint32_t frame_idx, double max_angle_deg, double jitter, double pose_out[12]);
void hfpf_synth_frame(uint64_t seed, uint32_t frame_idx, uint32_t W, uint32_t H, double fx_override, const double pose[12], double noise_sigma,
                      uint32_t nan_permille, uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z, uint32_t off_rgb, void* out);
}

namespace {
struct Tf {
    uint64_t pose_seed;
};
int lookup(void* user, const char*, const char* source, double pose[12], char* err, uint32_t cap)
{
    const Tf* tf = static_cast<const Tf*>(user);
    if (strncmp(source, "camera_", 7) != 0) {
        snprintf(err, cap, "unknown frame %s", source);
        return 1;
    }
    hfpf_synth_pose(tf->pose_seed, (uint32_t)atoi(source + 7), 30.0, 0.05, pose);
    return 0;
}
double now()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
}  // namespace

int main(int argc, char** argv)
{
    uint32_t min_component = 0;
    const char* reference = nullptr;
    double max_deviation = 0.0;
    bool align = false, coverage = false, hide_filtered = false;
    double spacing = 0.0;
    const char* plan = nullptr;
    const char* section = nullptr;
    bool topology = false;
    while (argc > 2 && strncmp(argv[1], "--", 2) == 0) {
        if (strcmp(argv[1], "--align") == 0) {
            align = true;
            argv += 1, argc -= 1;
            continue;
        }
        if (strcmp(argv[1], "--mesh-topology") == 0) {
            topology = true;
            argv += 1, argc -= 1;
            continue;
        }
        if (strcmp(argv[1], "--hide-filtered") == 0) {
            hide_filtered = true;
            argv += 1, argc -= 1;
            continue;
        }
        if (strcmp(argv[1], "--coverage") == 0) {
            coverage = true;
            char* end = nullptr;
            const double v = strtod(argv[2], &end);
            const bool number = argc > 3 && end != argv[2] && *end == 0 && v > 0;
            if (number) spacing = v;
            argv += number ? 2 : 1, argc -= number ? 2 : 1;
            continue;
        }
        if (strcmp(argv[1], "--min-component") == 0) min_component = (uint32_t)strtoul(argv[2], nullptr, 0);
        else if (strcmp(argv[1], "--reference") == 0) reference = argv[2];
        else if (strcmp(argv[1], "--max-deviation") == 0) max_deviation = atof(argv[2]);
        else if (strcmp(argv[1], "--plan") == 0) plan = argv[2];
        else if (strcmp(argv[1], "--section") == 0) section = argv[2];
        else break;
        argv += 2, argc -= 2;
    }
    if (argc < 2 || strncmp(argv[1], "--", 2) == 0) {
        fprintf(stderr, "usage: hfpf_demo [--mesh-topology] [--section planes.txt] [--min-component N [--hide-filtered]] [--reference mesh.ply [--max-deviation metres] [--align] [--coverage [spacing]] [--plan poses.txt]] <out_dir> [frames] [W] [H] [resolution] [clean_every] [seed] [pose_seed]\n");
        return 2;
    }
    const std::string dir = argv[1];
    const uint32_t frames = argc > 2 ? (uint32_t)atoi(argv[2]) : 30;
    const uint32_t W = argc > 3 ? (uint32_t)atoi(argv[3]) : 640, H = argc > 4 ? (uint32_t)atoi(argv[4]) : 480;
    const float res = argc > 5 ? (float)atof(argv[5]) : 0.001f;
    const uint32_t clean_every = argc > 6 ? (uint32_t)atoi(argv[6]) : 10;
    const uint64_t seed = argc > 7 ? strtoull(argv[7], nullptr, 0) : 0xF051;
    Tf tf{argc > 8 ? strtoull(argv[8], nullptr, 0) : 0x5E3};
    const double fx = W == 640 ? 0.0 : 615.0;  // smaller images are crops of the 640x480 sensor

    const double box[6] = {-0.5, 0.5, -0.5, 0.5, 0.0, 1.0};
    hfpf_node_params p;
    hfpf_node_default_params(&p);
    p.fusion_frame = "base_link";
    p.directory_name = dir.c_str();
    p.bounding_box = box;
    p.bounding_box_len = 6;
    p.engine.resolution = res;
    p.clean_period_s = 0;  // explicit schedule instead of the 5 s thread
    p.final_clean_on_process = 1;
    hfpf_node* node = nullptr;
    if (hfpf_node_create(&p, lookup, &tf, &node) != HFPF_OK) {
        fprintf(stderr, "create: %s\n", hfpf_node_last_error(nullptr));
        return 1;
    }
    if (topology) {
        hfpf_mesh_opts mo;
        memset(&mo, 0, sizeof mo);
        mo.struct_size = sizeof mo;
        mo.radius = 2, mo.max_distance = HUGE_VAL;
        hfpf_topology_opts to;
        memset(&to, 0, sizeof to);
        to.struct_size = sizeof to;
        if (hfpf_node_set_mesh_output(node, &mo) != HFPF_OK || hfpf_node_set_mesh_topology(node, &to) != HFPF_OK) {
            fprintf(stderr, "mesh-topology: %s\n", hfpf_node_last_error(node));
            return 1;
        }
    }
    if (section) {
        std::vector<double> planes;
        FILE* f = fopen(section, "r");
        double v;
        while (f && fscanf(f, "%lf", &v) == 1) planes.push_back(v);
        if (f) fclose(f);
        if (!f || planes.empty() || planes.size() % 4) {
            fprintf(stderr, "section: %s does not hold 4 numbers per plane\n", section);
            return 1;
        }
        hfpf_mesh_opts mo;
        memset(&mo, 0, sizeof mo);
        mo.struct_size = sizeof mo;
        mo.radius = 2, mo.max_distance = HUGE_VAL;
        hfpf_section_opts so;
        memset(&so, 0, sizeof so);
        so.struct_size = sizeof so;
        if (hfpf_node_set_mesh_output(node, &mo) != HFPF_OK || hfpf_node_set_section_planes(node, &so, planes.data(), (uint32_t)(planes.size() / 4)) != HFPF_OK) {
            fprintf(stderr, "section: %s\n", hfpf_node_last_error(node));
            return 1;
        }
    }
    if (min_component) {
        hfpf_component_opts co;
        memset(&co, 0, sizeof co);
        co.struct_size = sizeof co;
        co.reach = 1;
        co.min_normal_dot = -2.0;
        co.min_rows = min_component;
        if (hfpf_node_set_component_filter(node, &co) != HFPF_OK) {
            fprintf(stderr, "component filter: %s\n", hfpf_node_last_error(node));
            return 1;
        }
        hfpf_node_set_hide_filtered(node, hide_filtered ? 1 : 0);
    }
    if (reference) {
        hfpf_mesh_vertex* mv = nullptr;
        uint32_t* mt = nullptr;
        uint64_t nmv = 0, nmt = 0;
        if (hfpf_read_ply(reference, &mv, &nmv, &mt, &nmt) != HFPF_OK) {
            fprintf(stderr, "reference: %s\n", hfpf_last_error(nullptr));
            return 1;
        }
        hfpf_deviation_opts dopt;
        memset(&dopt, 0, sizeof dopt);
        dopt.struct_size = sizeof dopt;
        dopt.max_distance = max_deviation > 0 ? max_deviation : 10.0 * (double)res;
        const double ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        const int rc = hfpf_node_set_reference_mesh(node, &dopt, mv, nmv, sizeof(hfpf_mesh_vertex), mt, nmt, ident);
        hfpf_free_mesh(mv, mt);
        if (rc != HFPF_OK) {
            fprintf(stderr, "reference: %s\n", hfpf_node_last_error(node));
            return 1;
        }
        if (align) {
            hfpf_align_opts ao;
            memset(&ao, 0, sizeof ao);
            ao.struct_size = sizeof ao;
            ao.max_iterations = 20, ao.stride = 1, ao.min_inliers = 6;
            ao.compare = dopt;
            ao.damping = 1e-6, ao.eps_rotation = 1e-5, ao.eps_translation = 0.01 * (double)res;
            if (hfpf_node_set_reference_alignment(node, &ao) != HFPF_OK) {
                fprintf(stderr, "align: %s\n", hfpf_node_last_error(node));
                return 1;
            }
        }
        if (coverage) {
            hfpf_cover_opts vo;
            memset(&vo, 0, sizeof vo);
            vo.struct_size = sizeof vo;
            vo.radius = 2, vo.max_subdivision = 64;
            vo.max_distance = 2.0 * (double)res, vo.spacing = spacing > 0 ? spacing : (double)res, vo.min_normal_dot = -2.0;
            if (hfpf_node_set_reference_coverage(node, &vo) != HFPF_OK) {
                fprintf(stderr, "coverage: %s\n", hfpf_node_last_error(node));
                return 1;
            }
        }
        if (plan) {
            std::vector<double> poses;
            FILE* f = fopen(plan, "r");
            double v;
            while (f && fscanf(f, "%lf", &v) == 1) poses.push_back(v);
            if (f) fclose(f);
            if (!f || poses.empty() || poses.size() % 12) {
                fprintf(stderr, "plan: %s does not hold 12 numbers per pose\n", plan);
                return 1;
            }
            hfpf_plan_opts po;
            memset(&po, 0, sizeof po);
            po.struct_size = sizeof po;
            po.cover.struct_size = sizeof po.cover;
            po.cover.radius = 2, po.cover.max_subdivision = 64;
            po.cover.max_distance = 2.0 * (double)res, po.cover.spacing = spacing > 0 ? spacing : (double)res, po.cover.min_normal_dot = -2.0;
            po.view.struct_size = sizeof po.view;
            po.view.width = 640, po.view.height = 480;
            po.view.fx = po.view.fy = 525.0, po.view.cx = 319.5, po.view.cy = 239.5;
            po.view.z_near = 0.3, po.view.z_far = 3.0, po.view.splat_radius = -1, po.view.max_splat_radius = 4;
            po.occluder_near = 0.01, po.min_cos = 0.2, po.tolerance = 2.0 * (double)res, po.slope = 0.0, po.max_views = 8;
            if (hfpf_node_set_view_candidates(node, &po, poses.data(), (uint32_t)(poses.size() / 12)) != HFPF_OK) {
                fprintf(stderr, "plan: %s\n", hfpf_node_last_error(node));
                return 1;
            }
        }
    }
    hfpf_trigger_response r;
    hfpf_node_start(node, &r);
    std::vector<uint8_t> buf((size_t)W * H * 16);
    double t_cb = 0, t_clean = 0;
    for (uint32_t f = 0; f < frames; f++) {
        double pose[12];
        hfpf_synth_pose(tf.pose_seed, f, 30.0, 0.05, pose);
        hfpf_synth_frame(seed, f, W, H, fx, pose, 0.0005, 20, 16, 0, 4, 8, 12, buf.data());
        const std::string frame_id = "camera_" + std::to_string(f);
        hfpf_cloud_msg m{buf.data(), 1, W * H, 16, W * H * 16, 0, 4, 8, 12, frame_id.c_str()};  // published height=1 (first-row rule)
        double t0 = now();
        if (hfpf_node_on_point_cloud(node, &m) != 1) {
            fprintf(stderr, "frame %u not integrated: %s\n", f, hfpf_node_last_error(node));
            return 1;
        }
        t_cb += now() - t0;
        if (clean_every && (f + 1) % clean_every == 0 && f + 1 < frames) {
            t0 = now();
            hfpf_node_clean_now(node);
            t_clean += now() - t0;
        }
    }
    hfpf_sync(hfpf_node_grid(node));
    double t0 = now();
    if (hfpf_node_process(node, &r) != HFPF_OK || !r.success) {
        fprintf(stderr, "process: %s\n", r.message);
        return 1;
    }
    const double t_proc = now() - t0;
    hfpf_node_stats st;
    hfpf_node_get_stats(node, &st);
    printf("%s\nframes %llu integrated %llu  callbacks %.3f s  cleans %.3f s (%llu passes)  process %.3f s\n", r.message,
           (unsigned long long)st.received, (unsigned long long)st.integrated, t_cb, t_clean, (unsigned long long)st.clean_passes, t_proc);
    if (topology) {  // mesh_topology_summary.csv: one line; mesh_loops.csv: one line per loop
        unsigned long long w[13];
        FILE* f = fopen((dir + "/mesh_topology_summary.csv").c_str(), "r");
        if (!f || fscanf(f, "%*[^\n]\n") != 0 ||
            fscanf(f, "%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu", &w[0], &w[1], &w[2], &w[3], &w[4], &w[5], &w[6], &w[7], &w[8], &w[9], &w[10],
                   &w[11], &w[12]) != 13) {
            fprintf(stderr, "mesh_topology_summary.csv: cannot read it back\n");
            return 1;
        }
        fclose(f);
        printf("mesh topology: %llu triangles used (%llu invalid, %llu far), %llu vertices, %llu edges: %llu interior, %llu boundary, %llu non-manifold, "
               "%llu miswound; %llu loops (%llu closed); %llu shells (%llu watertight)\n",
               w[0] - w[2], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10], w[11], w[12]);
        struct Loop {
            unsigned id, first, nv, ne, ends, flags, shell;
            long long len, a[3];
        };
        std::vector<Loop> loops;
        Loop l;
        f = fopen((dir + "/mesh_loops.csv").c_str(), "r");
        if (!f || fscanf(f, "%*[^\n]\n") != 0) {
            fprintf(stderr, "mesh_loops.csv: cannot read it back\n");
            return 1;
        }
        while (fscanf(f, "%u,%u,%u,%u,%u,%u,%u,%lld,%lld,%lld,%lld\n", &l.id, &l.first, &l.nv, &l.ne, &l.ends, &l.flags, &l.shell, &l.len, &l.a[0], &l.a[1], &l.a[2]) == 11)
            loops.push_back(l);
        fclose(f);
        for (int k = 0; k < 5 && !loops.empty(); k++) {  // the five longest, longest first
            size_t best = 0;
            for (size_t i = 1; i < loops.size(); i++)
                if (loops[i].len > loops[best].len) best = i;
            const Loop& b = loops[best];
            printf("mesh topology: loop %u: %u edges, length %.6f m, vector area (%.6f, %.6f, %.6f) m^2, %s%s, shell %u\n", b.id, b.ne, (double)b.len * 0x1p-32,
                   (double)b.a[0] * 0x1p-28, (double)b.a[1] * 0x1p-28, (double)b.a[2] * 0x1p-28, (b.flags & HFPF_TOPOLOGY_LOOP_CLOSED) ? "closed" : "open",
                   (b.flags & HFPF_TOPOLOGY_LOOP_BRANCHED) ? ", branched" : "", b.shell);
            loops.erase(loops.begin() + (long)best);
        }
    }
    if (section) {  // section_summary.csv: one line per plane
        FILE* f = fopen((dir + "/section_summary.csv").c_str(), "r");
        if (!f || fscanf(f, "%*[^\n]\n") != 0) {
            fprintf(stderr, "section_summary.csv: cannot read it back\n");
            return 1;
        }
        unsigned v[9];
        long long len, area;
        while (fscanf(f, "%u,%u,%u,%u,%u,%u,%u,%u,%u,%lld,%lld\n", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &len, &area) == 11)
            printf("section: plane %u: %u segments in %u contours (%u closed, %u branched), length %.6f m, closed area %.6f m^2\n", v[0], v[2], v[6], v[7], v[8],
                   (double)len * 0x1p-32, (double)area * 0x1p-28);
        fclose(f);
    }
    if (reference && coverage) {  // the value line of coverage_summary.csv
        unsigned long long v[11] = {0};
        FILE* f = fopen((dir + "/coverage_summary.csv").c_str(), "r");
        const bool ok = f && fscanf(f, "%*[^\n]\n%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7],
                                    &v[8], &v[9], &v[10]) == 11;
        if (f) fclose(f);
        if (!ok) {
            fprintf(stderr, "coverage_summary.csv: cannot read it back\n");
            return 1;
        }
        const double area = ((double)v[8] * 0x1p32 + (double)v[7]) * 0x1p-40, covered = ((double)v[10] * 0x1p32 + (double)v[9]) * 0x1p-40;
        printf("coverage: %.6f of %.6f m^2 covered (%.1f %%), %llu of %llu samples (%.1f %%), %llu valid / %llu invalid / %llu huge triangles\n", covered, area,
               area > 0 ? 100.0 * covered / area : 0.0, v[5], v[3], v[3] ? 100.0 * (double)v[5] / (double)v[3] : 0.0, v[0], v[1], v[2]);
    }
    if (reference && plan) {  // view_plan.csv: the selected views in rank order
        struct Line { unsigned view; int rank; unsigned long long visible, gain, samples; };
        std::vector<Line> sel;
        FILE* f = fopen((dir + "/view_plan.csv").c_str(), "r");
        if (!f || fscanf(f, "%*[^\n]\n") != 0) {
            fprintf(stderr, "view_plan.csv: cannot read it back\n");
            return 1;
        }
        Line l;
        unsigned a, b, c;
        while (fscanf(f, "%u,%d,%u,%u,%u,%llu,%llu,%llu\n", &l.view, &l.rank, &a, &b, &c, &l.visible, &l.gain, &l.samples) == 8)
            if (l.rank >= 0) sel.push_back(l);
        fclose(f);
        for (int k = 0; k < (int)sel.size(); k++)
            for (const Line& x : sel)
                if (x.rank == k)
                    printf("plan: rank %d = view %u, adds %.6f m^2 (%llu samples) of %.6f m^2 it sees\n", k, x.view, (double)x.gain * 0x1p-40, x.samples,
                           (double)x.visible * 0x1p-40);
        if (sel.empty()) printf("plan: no candidate view adds anything\n");
    }
    hfpf_node_destroy(node);
    return 0;
}
