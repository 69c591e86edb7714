// oracle/ref_shim/pcl/common/transforms.h -- TEST INFRASTRUCTURE.  Stand-in for the PCL 1.8 headers that OccupancyGrid.hpp reaches
// through this include and uses at grid.hpp:289,302: pcl::eigen33 and pcl::computeMeanAndCovarianceMatrix.  Both forward to
// oracle/pcl_leaves.h, the ONE statement of these leaves that the oracle uses as well: common mode on purpose (see that header).
#pragma once

#include "../../Eigen/Core"
#include "../point_cloud.h"

namespace pcl {

// pcl::eigen33(mat, eigenvalue, eigenvector): the smallest eigenvalue of a symmetric 3 x 3 and its eigenvector
template <typename MatrixT, typename VectorT>
inline void eigen33(const MatrixT& mat, typename MatrixT::Scalar& eigenvalue, VectorT& eigenvector)
{
    float m[3][3], v[3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) m[i][j] = mat(i, j);
    hfpf_leaf::eigen33_smallest(m, eigenvalue, v);
    for (int i = 0; i < 3; i++) eigenvector[i] = v[i];
}

// pcl::computeMeanAndCovarianceMatrix(cloud, covariance, centroid): the PCL <= 1.10 single-pass form over a dense cloud
template <typename PointT>
inline unsigned int computeMeanAndCovarianceMatrix(const PointCloud<PointT>& cloud, Eigen::Matrix<float, 3, 3>& covariance_matrix,
                                                   Eigen::Matrix<float, 4, 1>& centroid)
{
    if (cloud.points.empty()) return 0;
    static_assert(sizeof(PointT) % sizeof(float) == 0, "points are whole floats apart");
    float c[3][3], mean[3];
    const unsigned int n = hfpf_leaf::mean_and_covariance(&cloud.points[0].x, sizeof(PointT) / sizeof(float), cloud.points.size(),
                                                          false, c, mean);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) covariance_matrix(i, j) = c[i][j];
    centroid[0] = mean[0], centroid[1] = mean[1], centroid[2] = mean[2], centroid[3] = 1.f;
    return n;
}

}  // namespace pcl
