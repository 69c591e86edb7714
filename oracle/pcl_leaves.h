// oracle/pcl_leaves.h -- TEST INFRASTRUCTURE.  The third-party leaf arithmetic of the reference's plane fit, stated ONCE:
//   pcl::computeMeanAndCovarianceMatrix (float)  (call site grid.hpp:302)
//   pcl::eigen33 / computeRoots / computeRoots2  (call site grid.hpp:289)
//   Eigen's fixed-size-3 reduction order c0 + (c1 + c2)
// restated from the published algorithms of PCL 1.8 / Eigen 3.3, with atan2f/cosf/sinf defined by det_math.h.
//
// Two translation units include this header and nothing else states these leaves:
//   oracle/hfpf_oracle.cpp               the CPU oracle (a restatement of grid.hpp);
//   oracle/ref_shim/ (through pcl/...)   the stand-in Eigen/PCL headers under which the reference's own grid.hpp is compiled
//                                        into oracle/_ref/libhfpf_ref.so (oracle/ref_driver.cpp).
// So when the parity tests compare the oracle with the compiled reference, these leaves are COMMON MODE ON PURPOSE: the
// comparison isolates what it can isolate -- the reference's control flow, state machine, ordering and emit rules -- and says
// nothing about whether this header agrees with the real PCL or Eigen.  A green parity test does not prove more than that.
//
// Plain floats and arrays only, so that neither side needs the other's vector type.  Build with -ffp-contract=off.
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>

#include "det_math.h"

// -DORACLE_USE_LIBM swaps the three deterministic trig leaves for this machine's libm (sensitivity studies only:
// tests/test_oracle_build_variants.py measures how many output rows depend on the last ulp of atan2f/cosf/sinf).
#ifdef ORACLE_USE_LIBM
#define ORACLE_ATAN2F(y, x) atan2f((y), (x))
#define ORACLE_COSF(x) cosf((x))
#define ORACLE_SINF(x) sinf((x))
#else
#define ORACLE_ATAN2F(y, x) odm_atan2f((y), (x))
#define ORACLE_COSF(x) odm_cosf((x))
#define ORACLE_SINF(x) odm_sinf((x))
#endif

namespace hfpf_leaf {

// Eigen fixed-size-3 reduction order: c0 + (c1 + c2).
#ifdef ORACLE_SUM3_LEFT  // sensitivity study only: plain left-to-right order instead of Eigen's redux tree
inline float sum3(float a, float b, float c) { return (a + b) + c; }
#else
inline float sum3(float a, float b, float c) { return a + (b + c); }
#endif

// pcl::computeRoots2 (float)
inline void compute_roots2(float b, float c, float roots[3])
{
    roots[0] = 0.0f;
    float d = (float)((double)(b * b) - 4.0 * (double)c);
    if ((double)d < 0.0) d = 0.0f;
    float sd = sqrtf(d);
    roots[2] = 0.5f * (b + sd);
    roots[1] = 0.5f * (b - sd);
}

// pcl::computeRoots (float, symmetric 3x3 m)
inline void compute_roots(const float m[3][3], float roots[3])
{
    float c0 = m[0][0] * m[1][1] * m[2][2] + 2.0f * m[0][1] * m[0][2] * m[1][2] - m[0][0] * m[1][2] * m[1][2] -
               m[1][1] * m[0][2] * m[0][2] - m[2][2] * m[0][1] * m[0][1];
    float c1 = m[0][0] * m[1][1] - m[0][1] * m[0][1] + m[0][0] * m[2][2] - m[0][2] * m[0][2] + m[1][1] * m[2][2] -
               m[1][2] * m[1][2];
    float c2 = m[0][0] + m[1][1] + m[2][2];

    if (fabsf(c0) < FLT_EPSILON) {
        compute_roots2(c2, c1, roots);
        return;
    }
    const float s_inv3 = (float)(1.0 / 3.0);
    const float s_sqrt3 = sqrtf(3.0f);
    float c2_over_3 = c2 * s_inv3;
    float a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
    if (a_over_3 > 0.0f) a_over_3 = 0.0f;

    float half_b = 0.5f * (c0 + c2_over_3 * (2.0f * c2_over_3 * c2_over_3 - c1));

    float q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
    if (q > 0.0f) q = 0.0f;

    float rho = sqrtf(-a_over_3);
    float theta = ORACLE_ATAN2F(sqrtf(-q), half_b) * s_inv3;
    float cos_theta = ORACLE_COSF(theta);
    float sin_theta = ORACLE_SINF(theta);
    roots[0] = c2_over_3 + 2.0f * rho * cos_theta;
    roots[1] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
    roots[2] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);

    if (roots[0] >= roots[1]) std::swap(roots[0], roots[1]);
    if (roots[1] >= roots[2]) {
        std::swap(roots[1], roots[2]);
        if (roots[0] >= roots[1]) std::swap(roots[0], roots[1]);
    }
    if (roots[0] <= 0.0f) compute_roots2(c2, c1, roots);
}

inline void cross3(const float a[3], const float b[3], float out[3])
{
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

// pcl::eigen33(mat, eigenvalue, eigenvector): the smallest eigenvalue and its eigenvector.
inline void eigen33_smallest(const float mat[3][3], float& eigenvalue, float vec[3])
{
    float scale = 0.0f;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) scale = std::max(scale, fabsf(mat[i][j]));
    if (scale <= FLT_MIN) scale = 1.0f;
    float s[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) s[i][j] = mat[i][j] / scale;
    float ev[3];
    compute_roots(s, ev);
    eigenvalue = ev[0] * scale;
    s[0][0] -= ev[0];
    s[1][1] -= ev[0];
    s[2][2] -= ev[0];
    float vec1[3], vec2[3], vec3[3];
    cross3(s[0], s[1], vec1);
    cross3(s[0], s[2], vec2);
    cross3(s[1], s[2], vec3);
    float len1 = sum3(vec1[0] * vec1[0], vec1[1] * vec1[1], vec1[2] * vec1[2]);
    float len2 = sum3(vec2[0] * vec2[0], vec2[1] * vec2[1], vec2[2] * vec2[2]);
    float len3 = sum3(vec3[0] * vec3[0], vec3[1] * vec3[1], vec3[2] * vec3[2]);
    const float* best = vec3;
    float len = len3;
    if (len1 >= len2 && len1 >= len3) {
        best = vec1;
        len = len1;
    } else if (len2 >= len1 && len2 >= len3) {
        best = vec2;
        len = len2;
    }
    const float r = sqrtf(len);
    vec[0] = best[0] / r;
    vec[1] = best[1] / r;
    vec[2] = best[2] / r;
}

// pcl::computeMeanAndCovarianceMatrix (float) of a dense cloud: single-pass float moments, accumulated in cloud order.  xyz points
// at the first point's x; the points are `stride` floats apart.  Returns the number of points (0: nothing written).
// PCL >= 1.11 accumulates the moments of (p - K), K = first point; PCL <= 1.10 (assumed for the reference) uses K = 0.
inline unsigned mean_and_covariance(const float* xyz, size_t stride, size_t n, bool shifted, float cov[3][3], float mean[3])
{
    if (n == 0) return 0;
    float accu[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#ifdef ORACLE_PCL_SHIFTED
    shifted = true;
#endif
    const float Kx = shifted ? xyz[0] : 0.f, Ky = shifted ? xyz[1] : 0.f, Kz = shifted ? xyz[2] : 0.f;
    for (size_t i = 0; i < n; i++) {
        const float* p = xyz + i * stride;
        const float px = p[0] - Kx, py = p[1] - Ky, pz = p[2] - Kz;
        accu[0] += px * px;
        accu[1] += px * py;
        accu[2] += px * pz;
        accu[3] += py * py;
        accu[4] += py * pz;
        accu[5] += pz * pz;
        accu[6] += px;
        accu[7] += py;
        accu[8] += pz;
    }
    const float fn = (float)n;
    for (int j = 0; j < 9; j++) accu[j] /= fn;
    mean[0] = accu[6] + Kx;
    mean[1] = accu[7] + Ky;
    mean[2] = accu[8] + Kz;
    cov[0][0] = accu[0] - accu[6] * accu[6];
    cov[0][1] = accu[1] - accu[6] * accu[7];
    cov[0][2] = accu[2] - accu[6] * accu[8];
    cov[1][1] = accu[3] - accu[7] * accu[7];
    cov[1][2] = accu[4] - accu[7] * accu[8];
    cov[2][2] = accu[5] - accu[8] * accu[8];
    cov[1][0] = cov[0][1];
    cov[2][0] = cov[0][2];
    cov[2][1] = cov[1][2];
    return (unsigned)n;
}

}  // namespace hfpf_leaf
