// Stand-alone evaluation of csrc/view.hpp (driven by tests/test_view.py, built with -ffp-contract=off and -fsanitize=address,undefined).
//
// Reads one case per line from stdin: 21 words in hex, the bits of T[12], fx, fy, cx, cy, z_lo, z_far, x, y, z (f64); then width,
// height, radius, max_radius in decimal and the bits of r_num in hex.  Prints per case
//   depth_ok pixel_ok bits(dx) bits(dy) bits(dz) bits(zc) pu pv inside r
// with pu, pv, inside and r as 0 where the projection fails (the callers read none of them then).  The two halves and the
// whole-projection convenience must agree; the expected values are the test's, from the numpy restatements.
#include "view.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>

namespace {

double from_bits(uint64_t b)
{
    double d;
    std::memcpy(&d, &b, sizeof d);
    return d;
}
uint64_t bits_of(double d)
{
    uint64_t b;
    std::memcpy(&b, &d, sizeof b);
    return b;
}

}  // namespace

int main()
{
    using namespace hfpf;
    uint64_t w[21];
    int n = 0, mismatches = 0;
    for (;;) {
        int got = 0;
        for (int i = 0; i < 21; i++) got += std::scanf("%" SCNx64, &w[i]) == 1;
        if (got == 0) break;
        Pinhole k{};
        int radius, max_radius;
        uint64_t r_num_bits;
        if (got != 21 || std::scanf("%" SCNu32 " %" SCNu32 " %d %d %" SCNx64, &k.width, &k.height, &radius, &max_radius, &r_num_bits) != 5) {
            std::fprintf(stderr, "case %d: short input\n", n);
            return 2;
        }
        double T[12];
        for (int i = 0; i < 12; i++) T[i] = from_bits(w[i]);
        k.fx = from_bits(w[12]), k.fy = from_bits(w[13]), k.cx = from_bits(w[14]), k.cy = from_bits(w[15]);
        const double z_lo = from_bits(w[16]);
        k.z_near = z_lo, k.z_far = from_bits(w[17]);
        const double x = from_bits(w[18]), y = from_bits(w[19]), z = from_bits(w[20]);

        double dx, dy, dz, zc;
        int pu = 0, pv = 0;
        const bool depth_ok = view_depth(T, k, z_lo, x, y, z, dx, dy, dz, zc);
        const bool pixel_ok = depth_ok && view_pixel(T, k, dx, dy, dz, zc, pu, pv);
        const bool inside = pixel_ok && view_inside(k, pu, pv);
        const int r = pixel_ok ? view_radius(radius, max_radius, from_bits(r_num_bits), zc) : 0;

        double ex, ey, ez, ec;
        int qu = 0, qv = 0;
        const bool whole = view_project(T, k, z_lo, x, y, z, ex, ey, ez, ec, qu, qv);
        if (whole != pixel_ok || bits_of(ex) != bits_of(dx) || bits_of(ey) != bits_of(dy) || bits_of(ez) != bits_of(dz) || bits_of(ec) != bits_of(zc) ||
            (whole && (qu != pu || qv != pv))) {
            std::fprintf(stderr, "case %d: view_project disagrees with its halves\n", n);
            mismatches++;
        }
        std::printf("%d %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %d %d %d %d\n", (int)depth_ok, (int)pixel_ok, bits_of(dx), bits_of(dy),
                    bits_of(dz), bits_of(zc), pixel_ok ? pu : 0, pixel_ok ? pv : 0, (int)inside, r);
        n++;
    }
    std::printf("view ok %d\n", n);
    return mismatches ? 1 : 0;
}
