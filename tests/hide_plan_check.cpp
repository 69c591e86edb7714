// tests/hide_plan_check.cpp -- the pure functions of hfpf_hide_* (csrc/host_plan.hpp) as a program of its own: the checks of opts,
// strides and lists, the word op against sets of cells written out, the clipping of a box against the dims, the split of a host list
// into uploads (every entry once, no span past the chunk, no read behind the last entry) and "does the snapshot carry the section".
#include <climits>
#include <cstdio>
#include <set>
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

static std::set<int> bits(uint64_t w)
{
    std::set<int> s;
    for (int b = 0; b < 64; b++)
        if (w >> b & 1) s.insert(b);
    return s;
}

// the contract's set algebra on one plane word, cell by cell
static void word_op(uint64_t old, uint64_t mark, uint64_t found)
{
    const std::set<int> H = bits(old), F = bits(found);
    std::set<int> M;
    for (int b : bits(mark))
        if (F.count(b)) M.insert(b);
    std::set<int> hide = H, show, others = H;
    for (int b : M) hide.insert(b);
    for (int b : H)
        if (!M.count(b)) show.insert(b);
    for (int b : F)
        if (!M.count(b)) others.insert(b);
    CHECK(bits(hide_word_op(kHideOpHide, old, mark, found)) == hide);
    CHECK(bits(hide_word_op(kHideOpShow, old, mark, found)) == show);
    CHECK(bits(hide_word_op(kHideOpOthers, old, mark, found)) == others);
    // H inside F stays inside F; HIDE then SHOW of the same mark restores a disjoint H; HIDE_OTHERS never shows
    for (uint32_t op : {kHideOpHide, kHideOpShow, kHideOpOthers}) CHECK((hide_word_op(op, old, mark, found) & ~found) == 0);
    if ((old & mark) == 0) CHECK(hide_word_op(kHideOpShow, hide_word_op(kHideOpHide, old, mark, found), mark, found) == old);
    CHECK((hide_word_op(kHideOpOthers, old, mark, found) & old) == old);
    CHECK(hide_word_op(kHideOpOthers, old, 0, found) == found);  // n = 0 hides everything
}

static void clip(const int32_t lo[3], const int32_t hi[3], const int32_t dim[3])
{
    const HideBox b = clip_hide_box(lo, hi, dim);
    // against the definition: voxel v (0 <= v < dim) is in the box iff lo <= v <= hi; checked on the corners and their neighbours
    bool any = true;
    for (int a = 0; a < 3; a++) {
        const int64_t l = std::max<int64_t>(lo[a], 0), h = std::min<int64_t>(hi[a], (int64_t)dim[a] - 1);
        if (l > h) any = false;
    }
    CHECK(b.empty == !any);
    if (b.empty) return;
    for (int a = 0; a < 3; a++) {
        CHECK(0 <= b.lo[a] && b.lo[a] <= b.hi[a] && b.hi[a] <= dim[a] - 1);
        CHECK(b.lo[a] >= lo[a] && b.hi[a] <= hi[a]);
        CHECK(b.lo[a] == 0 || b.lo[a] == lo[a]);
        CHECK(b.hi[a] == dim[a] - 1 || b.hi[a] == hi[a]);
    }
}

static void uploads(uint64_t n, uint32_t vs, bool sel, uint32_t ss, uint64_t chunk)
{
    const uint64_t per = hide_entries_per_upload(vs, sel, ss, chunk);
    CHECK(per >= 1);
    std::vector<uint8_t> seen(n, 0);
    for (uint64_t i0 = 0; i0 < n; i0 += per) {
        const uint64_t ne = std::min(per, n - i0);
        CHECK(ne >= 1);
        const uint64_t vb = hide_span_bytes(ne, vs, kHideVoxelBytes);
        CHECK(i0 * vs + vb <= hide_span_bytes(n, vs, kHideVoxelBytes));  // nothing behind the last entry's voxel
        CHECK(vb <= std::max<uint64_t>(chunk, vs));                      // one entry may exceed a tiny chunk, never more
        if (sel) {
            const uint64_t sb = hide_span_bytes(ne, ss, kHideSelectBytes);
            CHECK(i0 * ss + sb <= hide_span_bytes(n, ss, kHideSelectBytes));
            CHECK(sb <= std::max<uint64_t>(chunk, ss));
        }
        for (uint64_t i = i0; i < i0 + ne; i++) seen[i]++;
    }
    for (uint64_t i = 0; i < n; i++) CHECK(seen[i] == 1);
}

int main()
{
    // opts
    CHECK(hide_opts_ok(24, 24, kHideOpHide, 0, 0) && hide_opts_ok(24, 24, kHideOpShow, 0, 0) && hide_opts_ok(24, 24, kHideOpOthers, 0, 0));
    CHECK(!hide_opts_ok(20, 24, kHideOpHide, 0, 0) && !hide_opts_ok(0, 24, kHideOpHide, 0, 0));
    CHECK(!hide_opts_ok(24, 24, 0, 0, 0) && !hide_opts_ok(24, 24, 4, 0, 0) && !hide_opts_ok(24, 24, 0xFFFFFFFFu, 0, 0));
    CHECK(!hide_opts_ok(24, 24, kHideOpHide, 1, 0) && !hide_opts_ok(24, 24, kHideOpHide, 0, 1));
    CHECK(!hide_op_ok(0) && hide_op_ok(1) && hide_op_ok(2) && hide_op_ok(3) && !hide_op_ok(4));
    // strides and lists
    CHECK(hide_stride_ok(12, 12) && hide_stride_ok(16, 12) && hide_stride_ok(64, 12) && hide_stride_ok(4, 4) && hide_stride_ok(32, 4));
    CHECK(!hide_stride_ok(0, 12) && !hide_stride_ok(8, 12) && !hide_stride_ok(13, 12) && !hide_stride_ok(14, 12) && !hide_stride_ok(0, 4) && !hide_stride_ok(6, 4));
    CHECK(hide_stride_ok(0xFFFFFFFCu, 12) && !hide_stride_ok(0xFFFFFFFFu, 12));
    CHECK(hide_list_ok(true, 5, 12, false, 0) && hide_list_ok(true, 5, 64, true, 32) && hide_list_ok(false, 0, 12, false, 0));
    CHECK(hide_list_ok(true, 5, 12, false, 3));    // the select stride counts only with a selector
    CHECK(!hide_list_ok(false, 1, 12, false, 0));  // NULL voxels with n > 0
    CHECK(!hide_list_ok(true, 5, 8, false, 0) && !hide_list_ok(true, 5, 12, true, 0) && !hide_list_ok(true, 5, 12, true, 6) && !hide_list_ok(true, 0, 10, false, 0));
    CHECK(hide_device_aligned(0x1000, 0) && hide_device_aligned(0x1004, 0x2008) && !hide_device_aligned(0x1002, 0) && !hide_device_aligned(0x1000, 0x2001));
    // the word op: corner words and a pseudo-random walk
    const uint64_t words[] = {0, 1, 1ull << 63, ~0ull, 0x8000000000000001ull, 0x00FF00FF00FF00FFull, 0x0123456789ABCDEFull};
    for (uint64_t f : words)
        for (uint64_t m : words)
            for (uint64_t o : words) word_op(o & f, m, f);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < 2000; i++) {
        uint64_t w[3];
        for (uint64_t& v : w) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            v = x;
        }
        word_op(w[0] & w[2], w[1], w[2]);
    }
    // the box
    const int32_t dims[][3] = {{104, 72, 88}, {1, 1, 1}, {2097150, 72, 88}, {12630, 12630, 12630}};
    const int32_t vals[] = {INT_MIN, -1, 0, 1, 50, 71, 72, 87, 88, 103, 104, 12629, 12630, 2097149, 2097150, INT_MAX};
    for (const auto& d : dims)
        for (int32_t l : vals)
            for (int32_t h : vals) {
                const int32_t lo[3] = {l, 0, INT_MIN}, hi[3] = {h, INT_MAX, 5};
                clip(lo, hi, d);
                const int32_t lo2[3] = {0, l, l}, hi2[3] = {d[0] - 1, h, h};
                clip(lo2, hi2, d);
            }
    {
        const int32_t lo[3] = {-5, 10, 80}, hi[3] = {3, 200, 87}, d[3] = {104, 72, 88};
        const HideBox b = clip_hide_box(lo, hi, d);
        CHECK(!b.empty && b.lo[0] == 0 && b.hi[0] == 3 && b.lo[1] == 10 && b.hi[1] == 71 && b.lo[2] == 80 && b.hi[2] == 87);
        const int32_t lo1[3] = {5, 0, 0}, hi1[3] = {4, 71, 87};
        CHECK(clip_hide_box(lo1, hi1, d).empty);  // lo > hi
        const int32_t lo3[3] = {104, 0, 0}, hi3[3] = {200, 71, 87};
        CHECK(clip_hide_box(lo3, hi3, d).empty);  // index == dim holds no row
    }
    // the uploads of a host list
    const uint64_t ns[] = {0, 1, 2, 63, 64, 1000, 1001};
    const uint32_t strides[] = {12, 16, 64, 4096};
    const uint64_t chunks[] = {1, 12, 64, 100, 4096, 16u << 20};
    for (uint64_t n : ns)
        for (uint32_t vs : strides)
            for (uint64_t c : chunks) {
                uploads(n, vs, false, 0, c);
                uploads(n, vs, true, 4, c);
                uploads(n, vs, true, 32, c);
                uploads(n, vs, true, 8192, c);
            }
    CHECK(hide_entries_per_upload(12, false, 0, 16u << 20) == (16u << 20) / 12 && hide_entries_per_upload(64, true, 32, 16u << 20) == (16u << 20) / 64);
    CHECK(hide_entries_per_upload(12, true, 32, 16u << 20) == (16u << 20) / 32);
    CHECK(hide_span_bytes(1, 64, 12) == 12 && hide_span_bytes(3, 64, 12) == 140 && hide_span_bytes(3, 32, 4) == 68);
    // the snapshot
    CHECK(!snapshot_carries_hidden(0) && snapshot_carries_hidden(1) && snapshot_carries_hidden(~0ull));
    if (g_fail) return 1;
    printf("hide_plan ok\n");
    return 0;
}
