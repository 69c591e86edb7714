// oracle/ref_shim/pcl/point_types.h -- TEST INFRASTRUCTURE.  Stand-in for PCL 1.8's point types, as far as the reference's
// OccupancyGrid.hpp uses them (see Eigen/Core in this directory for what the stand-ins are and what they decide).  Own text.
// The three point types carry the members grid.hpp names; PCL's padding and unions are not needed and not restated.
#pragma once

#include <cstdint>

namespace pcl {

struct PointXYZ {
    float x = 0.f, y = 0.f, z = 0.f;
    float pad_ = 1.f;  // PCL keeps xyz in four floats
};

struct PointXYZRGB {
    float x = 0.f, y = 0.f, z = 0.f;
    float pad_ = 1.f;
    std::uint8_t b = 0, g = 0, r = 0, a = 255;
};

struct PointXYZRGBNormal {
    float x = 0.f, y = 0.f, z = 0.f;
    float pad_ = 1.f;
    float normal[3] = {0.f, 0.f, 0.f};
    float pad_n_ = 0.f;
    std::uint8_t b = 0, g = 0, r = 0, a = 255;
    float curvature = 0.f;
};

}  // namespace pcl
