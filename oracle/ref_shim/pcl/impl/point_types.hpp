// oracle/ref_shim/pcl/impl/point_types.hpp -- TEST INFRASTRUCTURE.  Stand-in: the point types are complete in pcl/point_types.h.
#pragma once
#include "../point_types.h"
