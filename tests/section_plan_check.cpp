// tests/section_plan_check.cpp -- the host decisions of hfpf_section_mesh* (csrc/host_plan.hpp) as a program of its own: the argument
// checks that need no pointer, the plane check, the packing of point and segment keys and their order, the chunks of planes and the
// grid, and the cap test with its bases.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "host_plan.hpp"

using namespace hfpf;

static int g_fail = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            g_fail++;                                                  \
        }                                                              \
    } while (0)

static void counts()
{
    CHECK(section_counts_fault(0, 0, 0) == nullptr);
    CHECK(section_counts_fault(1ull << 26, 0xFFFFFFFEull, 4096) == nullptr);
    CHECK(section_counts_fault((1ull << 26) + 1, 1, 1) != nullptr);
    CHECK(section_counts_fault(1, 0xFFFFFFFFull, 1) != nullptr);
    CHECK(section_counts_fault(1, 1ull << 40, 1) != nullptr);
    CHECK(section_counts_fault(1, 1, 4097) != nullptr);
    CHECK(kSecMaxPlanes == 1u << 12 && kSecMaxVerts == 1ull << 26);  // 12 + 26 + 26 bits are one key
}

static void planes()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double good[][4] = {{0, 0, 1, 0.25}, {0, 0, -2, -0.5}, {1e-160, 0, 0, 0}, {1e150, 1e150, 1e150, -1e300}, {1, 1, 1, 0}};
    for (const auto& p : good) CHECK(section_plane_ok(p));
    const double bad[][4] = {{0, 0, 0, 1},        {nan, 0, 1, 0}, {0, inf, 1, 0}, {0, 0, 1, nan}, {0, 0, 1, -inf},
                             {1e200, 0, 0, 0},    // nn overflows
                             {1e-170, 0, 0, 0}};  // nn underflows to 0
    for (const auto& p : bad) CHECK(!section_plane_ok(p));
    std::vector<double> list;
    for (int j = 0; j < 5; j++) list.insert(list.end(), good[j], good[j] + 4);
    CHECK(section_first_bad_plane(list.data(), 5) == 5);
    CHECK(section_first_bad_plane(nullptr, 0) == 0);
    list[4 * 3 + 1] = nan;
    CHECK(section_first_bad_plane(list.data(), 5) == 3 && section_first_bad_plane(list.data(), 3) == 3);
}

static void keys()
{
    const uint32_t top_v = (1u << 26) - 1, top_p = kSecMaxPlanes - 1;
    const uint32_t vs[] = {0, 1, 2, 12345, top_v - 1, top_v};
    const uint32_t ps[] = {0, 1, 63, 64, top_p};
    for (uint32_t pl : ps)
        for (uint32_t a : vs)
            for (uint32_t b : vs) {
                if (a == b) continue;
                const uint64_t k = sec_point_key(pl, a, b);
                CHECK(k == sec_point_key(pl, b, a));  // both triangles of an edge name the same point
                CHECK(sec_key_plane(k) == pl && sec_key_va(k) == std::min(a, b) && sec_key_vb(k) == std::max(a, b));
            }
    // ascending keys are ascending (plane, va, vb)
    CHECK(sec_point_key(0, top_v - 1, top_v) < sec_point_key(1, 0, 1));
    CHECK(sec_point_key(3, 5, top_v) < sec_point_key(3, 6, 7));
    CHECK(sec_point_key(3, 5, 6) < sec_point_key(3, 5, 7));
    CHECK(sec_point_key(top_p, top_v - 1, top_v) == ~0ull - (1ull << 26));  // all 64 bits in use, and no valid key is all ones
    const uint32_t ts[] = {0, 1, 0x7FFFFFFFu, 0xFFFFFFFEu};
    for (uint32_t pl : ps)
        for (uint32_t t : ts) {
            const uint64_t k = sec_segment_key(pl, t);
            CHECK(sec_seg_plane(k) == pl && sec_seg_tri(k) == t && k < (1ull << kSecSegKeyBits));
        }
    CHECK(sec_segment_key(0, 0xFFFFFFFEu) < sec_segment_key(1, 0));
    CHECK(kSecPointKeyBits == 64);
}

static void chunks()
{
    const uint32_t ns[] = {0, 1, 63, 64, 65, 128, 129, 4095, 4096};
    for (uint32_t n : ns) {
        const uint32_t nc = section_chunks(n);
        CHECK(nc >= 1 && nc == std::max(1u, (n + 63) / 64));
        std::vector<uint8_t> seen(n, 0);
        for (uint32_t c = 0; c < nc; c++) {
            const uint32_t np = section_chunk_planes(n, c);
            CHECK(np <= kSecChunkPlanes && (np >= 1 || n == 0));
            for (uint32_t j = 0; j < np; j++) {
                CHECK(c * kSecChunkPlanes + j < n);
                if (c * kSecChunkPlanes + j < n) seen[c * kSecChunkPlanes + j]++;
            }
        }
        for (uint32_t j = 0; j < n; j++) CHECK(seen[j] == 1);
        CHECK(section_chunk_planes(n, nc) == 0);
    }
    CHECK(kSecChunkPlanes * 4 * sizeof(double) == 2048);  // the chunk's planes in LDS
    CHECK(section_grid(0) == 1 && section_grid(1) == 1 && section_grid(256) == 1 && section_grid(257) == 2);
    CHECK(section_grid(0xFFFFFFFEull) == 0x1000000u);
}

static void cap()
{
    const uint32_t full = (uint32_t)kSecPlaneCap;
    {
        const uint32_t c[] = {3, 0, full, 7};
        uint64_t first[5];
        const SecCapFault f = section_cap_test(c, 4, first);
        CHECK(!f.over && f.count == 10ull + full);
        CHECK(first[0] == 0 && first[1] == 3 && first[2] == 3 && first[3] == 3ull + full && first[4] == 10ull + full);
    }
    {
        const uint32_t c[] = {3, full + 1, full + 2};
        const SecCapFault f = section_cap_test(c, 3, nullptr);
        CHECK(f.over && f.plane == 1 && f.count == (uint64_t)full + 1);  // the first plane beyond the cap, and its count
    }
    {
        const SecCapFault f = section_cap_test(nullptr, 0, nullptr);
        CHECK(!f.over && f.count == 0);
    }
    {  // the total: 4096 planes at the cap are 2^32 segments
        std::vector<uint32_t> c(4096, full);
        std::vector<uint64_t> first(4097);
        SecCapFault f = section_cap_test(c.data(), 4096, first.data());
        CHECK(f.over && f.plane == 4096 && f.count == 1ull << 32 && first[4096] == 1ull << 32);
        f = section_cap_test(c.data(), 2047, first.data());
        CHECK(!f.over && f.count == 2047ull << 20 && f.count <= kSecTotalCap);
        f = section_cap_test(c.data(), 2048, first.data());
        CHECK(f.over && f.plane == 2048 && f.count == 1ull << 31);
    }
    // the headroom sentence of the contract: 2^20 segments of less than 2^7 m (q32) and terms of less than 2^13 m^2 (q28) stay below 2^62
    CHECK(std::ldexp(1.0, 20 + 7 + 32) < std::ldexp(1.0, 62) && std::ldexp(1.0, 20 + 13 + 28) < std::ldexp(1.0, 62));
    // in-range coordinates: a cube of 64 m has a diagonal below 2^7 m, and half the square of that is below 2^13 m^2
    CHECK(64.0 * std::sqrt(3.0) < 128.0 && 0.5 * (64.0 * std::sqrt(3.0)) * (64.0 * std::sqrt(3.0)) < 8192.0);
}

int main()
{
    counts();
    planes();
    keys();
    chunks();
    cap();
    if (g_fail) {
        printf("section_plan: %d checks failed\n", g_fail);
        return 1;
    }
    printf("section_plan ok\n");
    return 0;
}
