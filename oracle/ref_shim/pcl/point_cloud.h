// oracle/ref_shim/pcl/point_cloud.h -- TEST INFRASTRUCTURE.  Stand-in for PCL 1.8's PointCloud<T>, as far as the reference's
// OccupancyGrid.hpp uses it: ::Ptr, .points, size(), width, height (see Eigen/Core in this directory).  Own text.
#pragma once

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../Eigen/Core"
#include "point_types.h"

namespace pcl {

template <typename PointT>
class PointCloud {
public:
    typedef std::shared_ptr<PointCloud<PointT>> Ptr;
    typedef std::shared_ptr<const PointCloud<PointT>> ConstPtr;
    std::vector<PointT> points;
    std::uint32_t width = 0, height = 0;
    bool is_dense = true;
    std::size_t size() const { return points.size(); }
};

namespace io {
// grid.hpp:485 (downloadData) hands the emitted cloud to this writer.  The stand-in only declares it: oracle/ref_driver.cpp
// defines it and keeps the cloud instead of writing a file, which is how the driver reads the reference's own emit path.
template <typename PointT>
int savePCDFileASCII(const std::string& file_name, const PointCloud<PointT>& cloud);
}  // namespace io

}  // namespace pcl
