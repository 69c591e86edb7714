// oracle/ref_driver.cpp -- TEST INFRASTRUCTURE.  A small C ABI over the REFERENCE'S OWN class OccupancyGrid
// (include/utilities/OccupancyGrid.hpp of the reference tree, "grid.hpp"), compiled unmodified against the stand-in Eigen/PCL
// headers of oracle/ref_shim into oracle/_ref/libhfpf_ref.so (oracle/Makefile, target ref).  Nothing of the reference is copied
// here: the header is taken from the reference tree at build time (-I$(HFPF_REFERENCE)/...), and oracle/_ref/ stays out of git.
// The reference's node (pointcloud_fusion_and_filter.cpp) needs ROS and cannot be compiled; the grid can, and it holds every rule
// the oracle restates: insert and buffer, dependant update, the 5x5x5 gate, plane fit, orientation, registration, replay, emit.
//
// What a comparison with this library proves, and what it does not: control flow, state machine, clean order and emit rule are
// the reference's own.  The Eigen/PCL leaf arithmetic is the stand-ins' (oracle/ref_shim/Eigen/Core, oracle/pcl_leaves.h), the
// same statements the oracle uses: common mode on purpose.
//
// Decisions of this driver, none of which touches the reference's text:
//   * VoxelInfo::mean_dist, ::normal, ::viewpoint are left uninitialised by the reference (grid.hpp:74-81) and the oracle defines
//     them as 0.  Here a replacement operator new IN THIS TRANSLATION UNIT zero-fills every block of up to kZeroFillMax bytes
//     (a VoxelInfo is ~120 bytes; larger blocks are vector storage, which is constructed before it is read, and the reference's
//     reserve(1000) per voxel, grid.hpp:228, would otherwise touch 24 kB a voxel).  The link exports href_* alone (ref_exports.map), so the
//     operators serve this library and nothing else in the process; blocks pass to and from libstdc++'s malloc-based
//     operators safely.
//   * clearVoxels (grid.hpp:167-183) is never called: it leaves stale keys behind and has no return.  Destroy and recreate.
//   * setK, clearVoxels, updateThicknessVectors and three download forms are declared bool and fall off their ends; the recipe
//     builds at an optimisation setting where that is well-behaved (oracle/Makefile).
//   * The reference prints to std::cout; the driver silences std::cout for the length of a call.
//   * Rows: set and order come from the reference's own emit path, downloadData (grid.hpp:456-488), whose cloud the stand-in
//     pcl::io::savePCDFileASCII defined below keeps instead of writing; count, sd and the distance moments, which that path only
//     prints as text, are read from VoxelInfo, and x, y, z and the normal of every row are checked against the kept cloud.
//   * Inputs that reach the reference's own undefined behaviour must not be passed: NaN coordinates (grid.hpp:633 -> 203) and a
//     grid with ydim >= 2048 (the int shift of grid.hpp:154); href_create refuses the latter.

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <new>
#include <type_traits>

// ---- zero-filling operator new (see above) ---------------------------------------------------------------------------------------
static constexpr std::size_t kZeroFillMax = 4096;
static void* href_alloc(std::size_t n)
{
    if (n == 0) n = 1;
    void* p = n <= kZeroFillMax ? std::calloc(1, n) : std::malloc(n);
    if (!p) throw std::bad_alloc();
    return p;
}
void* operator new(std::size_t n) { return href_alloc(n); }
void* operator new[](std::size_t n) { return href_alloc(n); }
void operator delete(void* p) noexcept { std::free(p); }
void operator delete[](void* p) noexcept { std::free(p); }
void operator delete(void* p, std::size_t) noexcept { std::free(p); }
void operator delete[](void* p, std::size_t) noexcept { std::free(p); }

#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

// ---- the writer downloadData calls: keep the cloud ---------------------------------------------------------------------------------
static pcl::PointCloud<pcl::PointXYZRGBNormal> g_emitted;
static bool g_emitted_set = false;
namespace pcl {
namespace io {
template <typename PointT>
int savePCDFileASCII(const std::string&, const PointCloud<PointT>& cloud)
{
    if constexpr (std::is_same<PointT, PointXYZRGBNormal>::value) {
        g_emitted = cloud;
        g_emitted_set = true;
    }
    return 0;
}
}  // namespace io
}  // namespace pcl

#include <utilities/OccupancyGrid.hpp>  // the reference's, unmodified

namespace {

struct Row {  // 64 bytes: the oracle's Row (hfpf_oracle.cpp), mirrored by oracle.ROW_DTYPE
    int32_t ix, iy, iz;
    uint32_t count;
    float x, y, z;
    float nx, ny, nz;
    float sdx, sdy, sdz;
    float mean_dist, sd_dist;
    uint32_t rgb;
};

struct Quiet {  // the reference reports on std::cout
    std::streambuf* old;
    Quiet() : old(std::cout.rdbuf(nullptr)) {}
    ~Quiet()
    {
        std::cout.rdbuf(old);
        std::cout.clear();
    }
};

VoxelInfo* info_of(OccupancyGrid* g, int x, int y, int z) { return reinterpret_cast<VoxelInfo*>(g->voxels_[x][y][z].data); }

}  // namespace

extern "C" {

// resolution, bbox (xmin, xmax, ymin, ymax, zmin, zmax), setK(2), construct: the node's own sequence
void* href_create(float resolution, const double* bbox)
{
    Quiet q;
    OccupancyGrid* g = new OccupancyGrid();
    g->setResolution(resolution, resolution, resolution);
    g->setDimensions(bbox[0], bbox[1], bbox[2], bbox[3], bbox[4], bbox[5]);
    g->setK(2);
    g->construct();
    if (g->ydim_ >= 2048) {  // y << 20 in int (grid.hpp:154): the reference's own undefined behaviour
        delete g;
        return nullptr;
    }
    return g;
}

void href_destroy(void* h)
{
    OccupancyGrid* g = (OccupancyGrid*)h;
    if (!g) return;
    for (auto& plane : g->voxels_)
        for (auto& line : plane)
            for (auto& v : line) delete reinterpret_cast<VoxelInfo*>(v.data);
    delete g;
}

void href_dims(void* h, int32_t out[3], double* res_out)
{
    OccupancyGrid* g = (OccupancyGrid*)h;
    out[0] = g->xdim_, out[1] = g->ydim_, out[2] = g->zdim_;
    *res_out = g->xres_;
}

// addPoints<6>(cloud, viewpoint), grid.hpp:185: n world-frame points, xyz packed
int32_t href_add_points(void* h, const float* xyz, uint64_t n, const float* vp)
{
    Quiet q;
    OccupancyGrid* g = (OccupancyGrid*)h;
    pcl::PointCloud<pcl::PointXYZRGB>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZRGB>);
    cloud->points.resize(n);
    for (uint64_t i = 0; i < n; i++) {
        cloud->points[i].x = xyz[3 * i];
        cloud->points[i].y = xyz[3 * i + 1];
        cloud->points[i].z = xyz[3 * i + 2];
    }
    cloud->width = (uint32_t)n, cloud->height = 1;
    Eigen::Vector3f viewpoint(vp[0], vp[1], vp[2]);
    return g->addPoints<6>(cloud, viewpoint) ? 1 : 0;
}

// updateThicknessVectors<6, 3>(), grid.hpp:311
void href_clean(void* h)
{
    Quiet q;
    ((OccupancyGrid*)h)->updateThicknessVectors<6, 3>();
}

int32_t href_is_dirty(void* h) { return ((OccupancyGrid*)h)->state_changed ? 1 : 0; }

// Rows through downloadData (see the header).  Returns the number of rows, or -1 when the kept cloud and the grid disagree.
int64_t href_extract(void* h, void* out_rows, uint64_t cap)
{
    Quiet q;
    OccupancyGrid* g = (OccupancyGrid*)h;
    g_emitted.points.clear();
    g_emitted_set = false;
    g->downloadData("", "/dev/null");
    if (!g_emitted_set) return -1;
    const auto& pts = g_emitted.points;
    Row* out = (Row*)out_rows;
    uint64_t n = 0;
    for (int x = 0; x < g->xdim_; x++)
        for (int y = 0; y < g->ydim_; y++)
            for (int z = 0; z < g->zdim_; z++) {
                if (!g->voxels_[x][y][z].occupied) continue;
                const VoxelInfo* d = info_of(g, x, y, z);
                if (!d->normal_found) continue;
                if (n >= pts.size()) return -1;
                const auto& p = pts[n];
                if (memcmp(&p.x, &d->centroid(0), 4) || memcmp(&p.y, &d->centroid(1), 4) || memcmp(&p.z, &d->centroid(2), 4) ||
                    memcmp(p.normal, d->normal.data(), 12))
                    return -1;
                if (out && n < cap) {
                    Row& r = out[n];
                    r.ix = x, r.iy = y, r.iz = z;
                    r.count = (uint32_t)d->count;
                    r.x = p.x, r.y = p.y, r.z = p.z;
                    r.nx = p.normal[0], r.ny = p.normal[1], r.nz = p.normal[2];
                    r.sdx = d->sd(0), r.sdy = d->sd(1), r.sdz = d->sd(2);
                    r.mean_dist = d->mean_dist;
                    r.sd_dist = d->sd_dist;
                    r.rgb = 0;  // the emit path never writes a colour (grid.hpp:471-479)
                }
                n++;
            }
    if (n != pts.size()) return -1;
    return (int64_t)n;
}

// occupied cells of the whole (dim + 1)^3 storage, ascending (x, y, z); returns their number
uint64_t href_occupied(void* h, int32_t* xyz, uint64_t cap)
{
    OccupancyGrid* g = (OccupancyGrid*)h;
    uint64_t n = 0;
    for (int x = 0; x <= g->xdim_; x++)
        for (int y = 0; y <= g->ydim_; y++)
            for (int z = 0; z <= g->zdim_; z++)
                if (g->voxels_[x][y][z].occupied) {
                    if (xyz && n < cap) xyz[3 * n] = x, xyz[3 * n + 1] = y, xyz[3 * n + 2] = z;
                    n++;
                }
    return n;
}

// one cell's dependants list, in order, decoded with the reference's getVoxelCoords(hash); returns its length
uint64_t href_dependants(void* h, int32_t x, int32_t y, int32_t z, int32_t* xyz, uint64_t cap)
{
    OccupancyGrid* g = (OccupancyGrid*)h;
    if (x < 0 || y < 0 || z < 0 || x > g->xdim_ || y > g->ydim_ || z > g->zdim_) return 0;
    const VoxelInfo* d = info_of(g, x, y, z);
    if (!d) return 0;
    const uint64_t n = d->dependants.size();
    for (uint64_t i = 0; xyz && i < n && i < cap; i++) {
        int xx, yy, zz;
        std::tie(xx, yy, zz) = g->getVoxelCoords(d->dependants[i]);
        xyz[3 * i] = xx, xyz[3 * i + 1] = yy, xyz[3 * i + 2] = zz;
    }
    return n;
}

// the cells that hold a non-empty dependants list, ascending (x, y, z); returns their number
uint64_t href_dependant_cells(void* h, int32_t* xyz, uint64_t cap)
{
    OccupancyGrid* g = (OccupancyGrid*)h;
    uint64_t n = 0;
    for (int x = 0; x <= g->xdim_; x++)
        for (int y = 0; y <= g->ydim_; y++)
            for (int z = 0; z <= g->zdim_; z++) {
                const VoxelInfo* d = info_of(g, x, y, z);
                if (d && !d->dependants.empty()) {
                    if (xyz && n < cap) xyz[3 * n] = x, xyz[3 * n + 1] = y, xyz[3 * n + 2] = z;
                    n++;
                }
            }
    return n;
}

// 1 when a fresh VoxelInfo's three uninitialised members read as 0 (the zero-filling operator new is in effect)
int32_t href_fresh_info_is_zero(void)
{
    void* scratch = operator new(sizeof(VoxelInfo));
    memset(scratch, 0xA5, sizeof(VoxelInfo));
    operator delete(scratch);  // the allocator may hand the same dirty block out again
    VoxelInfo* d = new VoxelInfo();
    const float zero[3] = {0.f, 0.f, 0.f};
    const bool ok = !memcmp(d->normal.data(), zero, 12) && !memcmp(d->viewpoint.data(), zero, 12) && !memcmp(&d->mean_dist, zero, 4);
    delete d;
    return ok ? 1 : 0;
}

uint64_t href_sizeof_row(void) { return sizeof(Row); }

}  // extern "C"
