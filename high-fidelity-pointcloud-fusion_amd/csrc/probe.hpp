// csrc/probe.hpp -- leaf probes (include/hfpf_probe.h; tests only): kernels that run the device functions of the hot path's kernels
// on given inputs, and the hfpf_probe_* entries that launch them.  hfpf.hip includes it once, at its end.
#pragma once

#include "../../include/hfpf_probe.h"
#include "kernels.hpp"

namespace hfpf {

// One depth image, pixel by pixel, through the loads and the back-projection of k_integrate's DEPTH form.
__global__ void k_probe_depth(const DepthLayout L, const uint8_t* __restrict__ dimg, const uint32_t n, float* __restrict__ xyz_out,
                              uint32_t* __restrict__ rgb_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const vf4 r = depth_fetch<true>(dimg, L.color, L, i);
    const F3 c = depth_point(L, r);
    xyz_out[3 * (uint64_t)i] = c.x;
    xyz_out[3 * (uint64_t)i + 1] = c.y;
    xyz_out[3 * (uint64_t)i + 2] = c.z;
    rgb_out[i] = __float_as_uint(r.y);
}

__global__ void k_probe_points(const GridParams g, const double* __restrict__ pose, const float* __restrict__ xyz, const uint64_t n,
                               float* __restrict__ q_out, int32_t* __restrict__ idx_out, uint8_t* __restrict__ flags_out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double T[12];
    for (int k = 0; k < 12; k++) T[k] = pose[k];
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const F3 q = transform_point(T, x, y, z);
    int32_t ix, iy, iz;
    voxel_coords(g, q, ix, iy, iz);
    q_out[3 * i] = q.x;
    q_out[3 * i + 1] = q.y;
    q_out[3 * i + 2] = q.z;
    idx_out[3 * i] = ix;
    idx_out[3 * i + 1] = iy;
    idx_out[3 * i + 2] = iz;
    flags_out[i] = (zclip_pass(g, z) ? 1 : 0) | (valid_point(g, q) ? 2 : 0);
}

__global__ void k_probe_normals(const GridParams g, const uint64_t n, const int32_t* __restrict__ cells, const uint8_t* __restrict__ occ,
                                const float* __restrict__ vps, float* __restrict__ normals_out, int32_t* __restrict__ totals_out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t x = cells[3 * i], y = cells[3 * i + 1], z = cells[3 * i + 2];
    Moments m;
    m.clear();
    int total = 0;
    for (int d = 0; d < 125; d++) {
        const int a = d / 25 - 2, b = (d / 5) % 5 - 2, c = d % 5 - 2;
        if (!occ[125 * i + d] || !valid_coord(g, x + a, y + b, z + c)) continue;
        m.add(voxel_center(g, x + a, y + b, z + c), g.cov_shifted != 0);
        total++;
    }
    totals_out[i] = total;
    F3 nrm = {0, 0, 0};
    if (total >= 3) {
        nrm = m.normal(total);
        nrm = orient_normal(nrm, F3{vps[3 * i], vps[3 * i + 1], vps[3 * i + 2]}, voxel_center(g, x, y, z));
    }
    normals_out[3 * i] = nrm.x;
    normals_out[3 * i + 1] = nrm.y;
    normals_out[3 * i + 2] = nrm.z;
}

__global__ void k_probe_project(const GridParams g, const uint64_t n, const float* __restrict__ pts, const float* __restrict__ centres,
                                const float* __restrict__ normals, float* __restrict__ proj_out, double* __restrict__ dist_out,
                                uint8_t* __restrict__ member_out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F3 proj;
    double dist;
    const bool mem = cylinder_member(g, F3{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]}, F3{centres[3 * i], centres[3 * i + 1], centres[3 * i + 2]},
                                     F3{normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]}, proj, dist);
    proj_out[3 * i] = proj.x;
    proj_out[3 * i + 1] = proj.y;
    proj_out[3 * i + 2] = proj.z;
    dist_out[i] = dist;
    F3 a, ab;
    float dd, sp, distf;
    line_of(g, F3{centres[3 * i], centres[3 * i + 1], centres[3 * i + 2]}, F3{normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]}, a, ab, dd);
    const bool mem2 = line_member(g, F3{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]}, a, ab, dd, sp, distf);  // the kernels' form
    float sp3, distf3;  // the form with the hoisted division (k_update_cells): must agree bit for bit
    const bool mem3 = line_member_hoisted(g, F3{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]}, a, ab, line_div_of(dd), sp3, distf3);
    const bool same = mem3 == mem2 && __float_as_uint(sp3) == __float_as_uint(sp) && __float_as_uint(distf3) == __float_as_uint(distf);
    member_out[i] = (mem ? 1 : 0) | (mem2 ? 2 : 0) | (same ? 4 : 0);
}

__global__ void k_probe_trig(const uint64_t n, const float* __restrict__ y, const float* __restrict__ x, float* __restrict__ a_out,
                             float* __restrict__ c_out, float* __restrict__ s_out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    a_out[i] = det_atan2f(y[i], x[i]);
    c_out[i] = det_cosf(x[i]);
    s_out[i] = det_sinf(x[i]);
}

}  // namespace hfpf

// An input of a probe: `count` T from host memory into buf (*d), enqueued.  An output is a scratch_n and a probe_down.
template <typename T>
static int probe_up(hfpf_handle* h, DevBuf& buf, const T* src, uint64_t count, T** d)
{
    if (int rc = scratch_n(h, buf, count, d)) return rc;
    HIPCHK(h, hipMemcpyAsync(*d, src, count * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return HFPF_OK;
}
#define PROBE_DOWN(dst, d, count) HIPCHK(h, hipMemcpyAsync((dst), (d), (count) * sizeof *(d), hipMemcpyDeviceToHost, h->stream));

extern "C" {

int hfpf_probe_points(hfpf_handle* h, const double pose[12], const float* xyz, uint64_t n, float* q_out, int32_t* idx_out, uint8_t* flags_out)
{
    if (!h || !pose || !xyz || !q_out || !idx_out || !flags_out) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (n == 0) return HFPF_OK;
    int rc;
    double* d_pose; float *d_xyz, *d_q;
    int32_t* d_idx; uint8_t* d_flags;
    if ((rc = probe_up(h, h->probe_a, pose, 12, &d_pose)) || (rc = probe_up(h, h->probe_b, xyz, 3 * n, &d_xyz))) return rc;
    if ((rc = scratch_n(h, h->probe_c, 3 * n, &d_q)) || (rc = scratch_n(h, h->probe_d, 3 * n, &d_idx)) || (rc = scratch_n(h, h->probe_e, n, &d_flags))) return rc;
    hipLaunchKernelGGL(k_probe_points, dim3(blocks_for(n, 256)), dim3(256), 0, h->stream, h->g, d_pose, d_xyz, n, d_q, d_idx, d_flags);
    HIPCHK(h, hipGetLastError());
    PROBE_DOWN(q_out, d_q, 3 * n);
    PROBE_DOWN(idx_out, d_idx, 3 * n);
    PROBE_DOWN(flags_out, d_flags, n);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HFPF_OK;
}

int hfpf_probe_normals(hfpf_handle* h, uint64_t n, const int32_t* cells, const uint8_t* occ, const float* vps, float* normals_out, int32_t* totals_out)
{
    if (!h || !cells || !occ || !vps || !normals_out || !totals_out) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (n == 0) return HFPF_OK;
    int rc;
    int32_t *d_cells, *d_totals; uint8_t* d_occ; float *d_vps, *d_normals;
    if ((rc = probe_up(h, h->probe_a, cells, 3 * n, &d_cells)) || (rc = probe_up(h, h->probe_b, occ, 125 * n, &d_occ))) return rc;
    if ((rc = probe_up(h, h->probe_c, vps, 3 * n, &d_vps))) return rc;
    if ((rc = scratch_n(h, h->probe_d, 3 * n, &d_normals)) || (rc = scratch_n(h, h->probe_e, n, &d_totals))) return rc;
    hipLaunchKernelGGL(k_probe_normals, dim3(blocks_for(n, 64)), dim3(64), 0, h->stream, h->g, n, d_cells, d_occ, d_vps, d_normals, d_totals);
    HIPCHK(h, hipGetLastError());
    PROBE_DOWN(normals_out, d_normals, 3 * n);
    PROBE_DOWN(totals_out, d_totals, n);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HFPF_OK;
}

int hfpf_probe_project(hfpf_handle* h, uint64_t n, const float* pts, const float* centres, const float* normals, float* proj_out, double* dist_out,
                       uint8_t* member_out)
{
    if (!h || !pts || !centres || !normals || !proj_out || !dist_out || !member_out) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (n == 0) return HFPF_OK;
    int rc;
    float *d_pts, *d_centres, *d_normals, *d_proj; double* d_dist; uint8_t* d_member;
    if ((rc = probe_up(h, h->probe_a, pts, 3 * n, &d_pts)) || (rc = probe_up(h, h->probe_b, centres, 3 * n, &d_centres))) return rc;
    if ((rc = probe_up(h, h->probe_c, normals, 3 * n, &d_normals))) return rc;
    if ((rc = scratch_n(h, h->probe_d, 3 * n, &d_proj)) || (rc = scratch_n(h, h->probe_e, n, &d_dist)) || (rc = scratch_n(h, h->probe_f, n, &d_member))) return rc;
    hipLaunchKernelGGL(k_probe_project, dim3(blocks_for(n, 256)), dim3(256), 0, h->stream, h->g, n, d_pts, d_centres, d_normals, d_proj, d_dist, d_member);
    HIPCHK(h, hipGetLastError());
    PROBE_DOWN(proj_out, d_proj, 3 * n);
    PROBE_DOWN(dist_out, d_dist, n);
    PROBE_DOWN(member_out, d_member, n);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HFPF_OK;
}

int hfpf_probe_depth(hfpf_handle* h, const hfpf_depth_image* desc, const void* depth, const void* color, float* xyz_out, uint32_t* rgb_out)
{
    if (!h || !xyz_out || !rgb_out) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DepthSpec ds;
    int rc = depth_spec(h, desc, depth, color, &ds);
    if (rc) return rc;
    const uint32_t n = ds.width * ds.height;
    uint8_t *d_depth, *d_color = nullptr;  // (without colour depth_layout() passes no colour image)
    float* d_xyz; uint32_t* d_rgb;
    if ((rc = probe_up(h, h->probe_a, (const uint8_t*)depth, ds.depth_bytes(), &d_depth))) return rc;
    if (ds.color_bpp && (rc = probe_up(h, h->probe_b, (const uint8_t*)color, ds.color_bytes(), &d_color))) return rc;
    if ((rc = scratch_n(h, h->probe_c, 3 * (uint64_t)n, &d_xyz)) || (rc = scratch_n(h, h->probe_d, n, &d_rgb))) return rc;
    hipLaunchKernelGGL(k_probe_depth, dim3(blocks_for(n, 256)), dim3(256), 0, h->stream, depth_layout(ds, d_color, 0), d_depth, n, d_xyz, d_rgb);
    HIPCHK(h, hipGetLastError());
    PROBE_DOWN(xyz_out, d_xyz, 3 * (uint64_t)n);
    PROBE_DOWN(rgb_out, d_rgb, n);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HFPF_OK;
}

int hfpf_probe_trig(hfpf_handle* h, uint64_t n, const float* y, const float* x, float* atan2_out, float* cos_out, float* sin_out)
{
    if (!h || !y || !x || !atan2_out || !cos_out || !sin_out) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (n == 0) return HFPF_OK;
    int rc;
    float *d_y, *d_x, *d_atan2, *d_cos, *d_sin; if ((rc = probe_up(h, h->probe_a, y, n, &d_y)) || (rc = probe_up(h, h->probe_b, x, n, &d_x))) return rc;
    if ((rc = scratch_n(h, h->probe_c, n, &d_atan2)) || (rc = scratch_n(h, h->probe_d, n, &d_cos)) || (rc = scratch_n(h, h->probe_e, n, &d_sin))) return rc;
    hipLaunchKernelGGL(k_probe_trig, dim3(blocks_for(n, 256)), dim3(256), 0, h->stream, n, d_y, d_x, d_atan2, d_cos, d_sin);
    HIPCHK(h, hipGetLastError());
    PROBE_DOWN(atan2_out, d_atan2, n);
    PROBE_DOWN(cos_out, d_cos, n);
    PROBE_DOWN(sin_out, d_sin, n);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HFPF_OK;
}

}  // extern "C"
