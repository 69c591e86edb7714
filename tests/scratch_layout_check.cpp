// Stand-alone check of csrc/scratch_layout.hpp (driven by tests/test_scratch_layout.py, built with -fsanitize=address,undefined).
//
// Every layout the engine cuts out of one buffer is declared here with stand-in element types of the same size, for a range of
// counts.  For each: the total equals the byte formula the engine used before it had the helper, the slices are aligned, in
// declaration order and disjoint, and -- in a malloc of exactly the total -- every byte of every slice can be written and keeps
// its value.  For a count of 2^32 + 1 only the totals are compared, in 64-bit arithmetic.
#include "scratch_layout.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

namespace {

template <int N, typename Word>
struct Rec {
    Word w[N / sizeof(Word)];
};
using B1 = uint8_t;
using B4 = uint32_t;
using B8 = uint64_t;
using B12 = Rec<12, uint32_t>;   // three indices of a triangle
using B16 = Rec<16, uint64_t>;
using B48 = Rec<48, uint64_t>;   // a component record
using B64 = Rec<64, uint64_t>;   // a row, a hit
using B96 = Rec<96, double>;     // compare's triangle record; its counters and summary
using B104 = Rec<104, uint64_t>; // cover's summary and total
using B112 = Rec<112, double>;   // cover's triangle record
static_assert(sizeof(B12) == 12 && sizeof(B16) == 16 && sizeof(B48) == 48 && sizeof(B96) == 96 && sizeof(B104) == 104 && sizeof(B112) == 112, "stand-in sizes");

int g_failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            g_failures++;                                 \
            std::fprintf(stderr, "FAIL %s: ", what);      \
            std::fprintf(stderr, __VA_ARGS__);            \
            std::fprintf(stderr, " (%s)\n", #cond);       \
        }                                                 \
    } while (0)

struct Case {
    struct Slice {
        std::function<char*()> at;
        uint64_t elem, align, count, round_to;
    };
    hfpf::ScratchLayout lay;
    std::vector<Slice> slices;
    uint64_t skipped = 0;
    template <typename T>
    Case& add(T** p, uint64_t count, uint64_t round_to = 1)
    {
        lay.add(p, count, round_to);
        slices.push_back(Slice{[p] { return reinterpret_cast<char*>(*p); }, sizeof(T), alignof(T), count, round_to});
        return *this;
    }
    Case& skip(uint64_t bytes)
    {
        lay.skip(bytes);
        skipped += bytes;
        return *this;
    }
};

uint64_t up(uint64_t v, uint64_t to) { return (v + to - 1) / to * to; }

// expect: the byte formula of the code before the helper.  allocate = false: totals only.
void check(const char* what, Case& c, uint64_t expect, bool allocate = true)
{
    const uint64_t total = c.lay.bytes();
    CHECK(c.lay.fits(), "%zu slices", c.slices.size());
    CHECK(total == expect, "total %llu, formula %llu", (unsigned long long)total, (unsigned long long)expect);
    if (!allocate) return;
    char* base = static_cast<char*>(std::malloc(total ? total : 1));
    if (!base) {
        std::fprintf(stderr, "malloc of %llu bytes failed\n", (unsigned long long)total);
        std::exit(2);
    }
    c.lay.place(base);
    char* end_of_previous = base;
    for (size_t i = 0; i < c.slices.size(); i++) {
        const Case::Slice& s = c.slices[i];
        char* p = s.at();
        const uint64_t room = up(s.count * s.elem, s.round_to);
        CHECK(p >= end_of_previous, "slice %zu starts %td bytes before the end of slice %zu", i, end_of_previous - p, i - 1);
        CHECK(p < end_of_previous + s.align, "slice %zu leaves a gap of %td bytes", i, p - end_of_previous);
        CHECK(reinterpret_cast<uintptr_t>(p) % s.align == 0, "slice %zu is not aligned to %llu", i, (unsigned long long)s.align);
        CHECK(p + room <= base + total, "slice %zu ends %td bytes past the total", i, (p + room) - (base + total));
        std::memset(p, (int)(0x11 * (i + 1)), room);  // every byte of the slice, its rounding included
        end_of_previous = p + room;
    }
    CHECK(end_of_previous + c.skipped == base + total, "the total is %td bytes more than the slices need", (base + total) - end_of_previous - (ptrdiff_t)c.skipped);
    for (size_t i = 0; i < c.slices.size(); i++) {  // disjoint: no later slice wrote into this one
        const Case::Slice& s = c.slices[i];
        const char* p = s.at();
        const uint64_t room = up(s.count * s.elem, s.round_to);
        uint64_t bad = 0;
        for (uint64_t k = 0; k < room; k++) bad += (unsigned char)p[k] != (unsigned char)(0x11 * (i + 1));
        CHECK(bad == 0, "%llu bytes of slice %zu were overwritten", (unsigned long long)bad, i);
    }
    std::free(base);
}

// The engine's layouts for a model of n rows / corners / components / vertices and m triangles / cubes.
void engine_layouts(uint64_t n, uint64_t m, bool allocate)
{
    const uint64_t n1 = n + 1, m1 = m + 1;
    {  // mesh_kdata: per corner the sample, the nearest row, the marks, the vertex count and its scan
        float* s;
        B4 *nid, *marks, *vcount, *vbase;
        Case c;
        c.add(&s, n1).add(&nid, n1).add(&marks, n1).add(&vcount, n1).add(&vbase, n1);
        check("mesh_kdata", c, n1 * 20, allocate);
    }
    {  // mesh_cdata
        B4 *tcount, *tbase;
        Case c;
        c.add(&tcount, m1).add(&tbase, m1);
        check("mesh_cdata", c, m1 * 8, allocate);
    }
    {  // mesh_ctr: the unique count and the miss word behind it
        B8* count;
        B4* miss;
        Case c;
        c.add(&count, 1).add(&miss, 2);
        check("mesh_ctr", c, 16, allocate);
    }
    {  // comp_rows: six arrays of n + 1
        B4* a[6];
        Case c;
        for (auto& p : a) c.add(&p, n1);
        check("comp_rows", c, n1 * 24, allocate);
    }
    {  // comp_recs: the records, then keep flags and their scan
        B48* recs;
        B4 *keep, *kbase;
        Case c;
        c.add(&recs, m).add(&keep, m1).add(&kbase, m1);
        check("comp_recs", c, m * 48 + m1 * 8, allocate);
    }
    {  // dev_bins: brick keys, counters + summary (4 * 8 + 64), flag, base, ub_start, the triangle ranges
        B8* ub_key;
        B96* counters;
        B4 *flag, *base, *ub_start, *trange;
        Case c;
        c.add(&ub_key, n).add(&counters, 1).add(&flag, n1).add(&base, n1).add(&ub_start, n1).add(&trange, 2 * n);
        check("dev_bins", c, n * 8 + 4 * 8 + 64 + (3 * n1 + 2 * n) * 4, allocate);
    }
    {  // dev_tri: the transformed vertices, then compare's or cover's triangle records
        double* v;
        B96* dev;
        B112* cov;
        Case a, b;
        a.add(&v, 3 * (n ? n : 1)).add(&dev, m);
        b.add(&v, 3 * (n ? n : 1)).add(&cov, m);
        check("dev_tri (compare)", a, (n ? n : 1) * 24 + m * 96, allocate);
        check("dev_tri (cover)", b, (n ? n : 1) * 24 + m * 112, allocate);
    }
    {  // dev_pairs: as emitted, then sorted
        B8 *in, *sorted;
        Case c;
        c.add(&in, m).add(&sorted, m);
        check("dev_pairs", c, m * 16, allocate);
    }
    for (uint64_t stride : {12u, 20u, 32u}) {  // dev_mesh: the vertices as they are, the indices at a 16-byte boundary, 16 spare bytes
        const uint64_t v_bytes = n ? (n - 1) * stride + 12 : 0;
        B1* verts;
        B4* tris;
        Case c;
        c.add(&verts, v_bytes, 16).add(&tris, 3 * m).skip(16);
        check("dev_mesh", c, ((v_bytes + 15) & ~15ull) + m * 12 + 16, allocate);
        if (allocate && c.lay.bytes()) {
            char* base = static_cast<char*>(std::malloc(c.lay.bytes()));
            c.lay.place(base);
            const char* what = "dev_mesh";
            CHECK((reinterpret_cast<char*>(tris) - base) % 16 == 0, "indices at offset %td", reinterpret_cast<char*>(tris) - base);
            std::free(base);
        }
    }
    {  // cov_bins: summary + total (96 + 8), the sample counts and their scan
        B104* ctr;
        B4 *count, *offset;
        Case c;
        c.add(&ctr, 1).add(&count, m1).add(&offset, m1);
        check("cov_bins", c, 96 + 8 + 2 * m1 * 4, allocate);
    }
    {  // ray_map: "has a row" and three levels of maps, each in whole 256-byte lines
        const uint64_t cells[3] = {n, (n + 3) / 4, (n + 15) / 16};
        B1 *has, *maps[3];
        Case c;
        c.add(&has, cells[0], 256);
        uint64_t expect = (cells[0] + 255) & ~255ull;
        for (int l = 0; l < 3; l++) {
            c.add(&maps[l], cells[l], 256);
            expect += (cells[l] + 255) & ~255ull;
        }
        check("ray_map", c, expect, allocate);
    }
    {  // query_out: the hits, then (optionally) the rows
        B64 *hits, *rows;
        Case a, b;
        a.add(&hits, n);
        b.add(&hits, n).add(&rows, n);
        check("query_out (hits)", a, n * 64, allocate);
        check("query_out (hits + rows)", b, n * 128, allocate);
    }
    {  // result_out: up to three arrays of bytes, each in whole 16-byte units
        const uint64_t bytes[3] = {n * 64, n * 4, m * 48};
        B1* p[3];
        Case c;
        uint64_t expect = 0;
        for (int i = 0; i < 3; i++) {
            c.add(&p[i], bytes[i], 16);
            expect += (bytes[i] + 15) & ~15ull;
        }
        check("result_out", c, expect, allocate);
    }
    {  // render_out: the requested planes of a view of n pixels, each 256-byte aligned
        float *depth, *normal;
        B4 *rgb, *count;
        int32_t* voxel;
        Case c;
        c.add(&depth, n, 256).add(&normal, 3 * n, 256).add(&rgb, n, 256).add(&count, n, 256).add(&voxel, 3 * n, 256);
        const uint64_t r4 = (4 * n + 255) & ~255ull, r12 = (12 * n + 255) & ~255ull;
        check("render_out", c, 3 * r4 + 2 * r12, allocate);
    }
    {  // ex_counts: one status word per rank, then this rank's own
        B8 *all, *mine;
        Case c;
        c.add(&all, n).add(&mine, 1);
        check("ex_counts", c, n1 * 8, allocate);
    }
}

// Not a layout of the engine: small elements in front of larger ones, where alignment has to add padding.
void padded_layouts(uint64_t n)
{
    const char* what = "padded";
    B1 *bytes, *tail;
    B8* words;
    B12* tri;
    B16* wide;
    Case c;
    c.add(&bytes, n).add(&words, n).add(&tri, n).add(&wide, n).add(&tail, n, 64);
    const uint64_t a = up(n, 8), b = a + 8 * n, d = up(b + 12 * n, 8), e = d + 16 * n;
    check(what, c, e + up(n, 64));
    CHECK(c.lay.bytes() <= n * (1 + 8 + 12 + 16) + up(n, 64) + 2 * 7, "padding of more than alignment - 1 per slice");
}

}  // namespace

int main()
{
    const uint64_t counts[] = {0, 1, 2, 3, 255, 256, 257};
    for (uint64_t n : counts)
        for (uint64_t m : counts) engine_layouts(n, m, true);
    for (uint64_t n : counts) padded_layouts(n);
    const uint64_t big = (1ull << 32) + 1;  // totals only: nothing of this size is allocated
    engine_layouts(big, big, false);
    engine_layouts(big, 3, false);
    engine_layouts(3, big, false);
    {  // more arrays than a layout holds: reported, and place() stays inside what was declared
        const char* what = "too many slices";
        B4* p[9];
        hfpf::ScratchLayout lay;
        for (auto& q : p) lay.add(&q, 1);
        CHECK(!lay.fits(), "nine slices fit");
    }
    if (g_failures) {
        std::fprintf(stderr, "%d checks failed\n", g_failures);
        return 1;
    }
    std::printf("scratch_layout ok\n");
    return 0;
}
