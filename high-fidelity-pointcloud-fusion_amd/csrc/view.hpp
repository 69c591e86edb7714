// csrc/view.hpp -- the pinhole view of include/hfpf.h ("render"), in one place: every kernel that looks at the model through a camera
// (render, track's association, plan, depth consistency) and the host code that fills their parameters take the rule from here.  Free
// of HIP, so g++ alone compiles it (tests/view_check.cpp pins its edges against the numpy restatements).
//
//   d  = p - t
//   zc = (T[2]*dx + T[6]*dy) + T[10]*dz          keep iff z_lo < zc < z_far
//   xc = (T[0]*dx + T[4]*dy) + T[8]*dz
//   yc = (T[1]*dx + T[5]*dy) + T[9]*dz
//   u  = (xc/zc)*fx + cx,  v = (yc/zc)*fy + cy    keep iff |u|, |v| < 2^30
//   pu = floor(u + 0.5),  pv = floor(v + 0.5)
//   r  = radius >= 0 ? radius : min(max_radius, floor(r_num / zc))
//
// Every sum is associated as written, every compare is strict and false for a NaN; -ffp-contract=off (csrc/Makefile) keeps a product
// and the sum behind it two roundings.  The projection comes in two halves because a splat tests its back-face cull between them.
#pragma once

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define HFPF_VIEW_FN __host__ __device__ __forceinline__
#else
#define HFPF_VIEW_FN inline
#endif

namespace hfpf {

struct Pinhole {
    double fx, fy, cx, cy, z_near, z_far;
    uint32_t width, height;
};

// The depth half: the offset d of (x, y, z) from the camera T (3x4, row-major, camera -> fusion frame) and its depth zc along the
// optical axis.  z_lo is the caller's: k.z_near, or the occluder_near of plan's occluders.
HFPF_VIEW_FN bool view_depth(const double* T, const Pinhole& k, const double z_lo, const double x, const double y, const double z, double& dx, double& dy,
                             double& dz, double& zc)
{
    dx = x - T[3], dy = y - T[7], dz = z - T[11];
    zc = (T[2] * dx + T[6] * dy) + T[10] * dz;
    return z_lo < zc && zc < k.z_far;
}

// The pixel half: the pixel (pu, pv) that d lands in, set only when both coordinates lie inside +-2^30 (so pu +- 15 does not wrap).
HFPF_VIEW_FN bool view_pixel(const double* T, const Pinhole& k, const double dx, const double dy, const double dz, const double zc, int& pu, int& pv)
{
    const double xc = (T[0] * dx + T[4] * dy) + T[8] * dz;
    const double yc = (T[1] * dx + T[5] * dy) + T[9] * dz;
    const double u = (xc / zc) * k.fx + k.cx;
    const double w = (yc / zc) * k.fy + k.cy;
    // (& and not &&: both compares are evaluated, as the kernels did before the rule moved here.  Behind a && the compiler branches
    // between them, which costs k_track_reduce four VGPRs and its depth form a wave per SIMD.)
    const bool u_in = fabs(u) < 1073741824.0, w_in = fabs(w) < 1073741824.0;
    if (!(u_in & w_in)) return false;
    pu = (int)floor(u + 0.5), pv = (int)floor(w + 0.5);
    return true;
}

// Both halves, for a caller with nothing to test between them.
HFPF_VIEW_FN bool view_project(const double* T, const Pinhole& k, const double z_lo, const double x, const double y, const double z, double& dx, double& dy,
                               double& dz, double& zc, int& pu, int& pv)
{
    return view_depth(T, k, z_lo, x, y, z, dx, dy, dz, zc) && view_pixel(T, k, dx, dy, dz, zc, pu, pv);
}

HFPF_VIEW_FN bool view_inside(const Pinhole& k, const int pu, const int pv) { return pu >= 0 && pu < (int)k.width && pv >= 0 && pv < (int)k.height; }

// The splat radius at depth zc: the fixed one, or (radius < 0) the auto radius with r_num = (0.5 * cell) * max(fx, fy).
HFPF_VIEW_FN int view_radius(const int radius, const int max_radius, const double r_num, const double zc)
{
    if (radius >= 0) return radius;
    const double ra = floor(r_num / zc);
    return ra < (double)max_radius ? (int)ra : max_radius;
}

}  // namespace hfpf
