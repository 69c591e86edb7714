// Stand-alone check of csrc/host_plan.hpp (driven by tests/test_host_plan.py, built with -fsanitize=address,undefined).
//
// The decisions of an integrate call and of a clean pass at the thresholds no device test reaches in seconds.  Every expected value
// is a literal worked out by hand from the rule in words, not recomputed with the expression under test.
#include "host_plan.hpp"

#include <cstdio>

namespace {

using namespace hfpf;
static_assert(kProbeFrames == 8, "the probe cases below are worked out for the default of 8 frames");

int g_failures = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            g_failures++;                                                      \
            std::fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #cond);       \
        }                                                                      \
    } while (0)

constexpr uint64_t kBig = 1ull << 40;  // a capacity that never binds

// A pass of n_in new cells and nothing else: no pending list, nothing registered, room for everything.  K = 3: 7 cells per candidate.
CleanPlan fresh_pass(uint64_t n_in, bool early, bool nowait_knob, bool replay_knob)
{
    return plan_clean(CleanHead{n_in, 0, 0, 0, 0, 0}, kBig, kBig, kBig, 0, false, 3, early, nowait_knob, replay_knob);
}

void small_pass()
{
    CleanPlan p = fresh_pass(299593, false, true, true);
    CHECK(p.n_in == 299593 && p.reg_ub == 2097151 && !p.full && p.no_wait);
    p = fresh_pass(299594, false, true, true);
    CHECK(p.n_in == 299594 && p.reg_ub == 2097158 && !p.full && !p.no_wait);
    CHECK(!fresh_pass(299593, false, false, true).no_wait);
    CHECK(!fresh_pass(1, false, false, true).no_wait);
    CHECK(fresh_pass(1, false, true, true).reg_ub == 7);
    CHECK(plan_clean(CleanHead{1, 0, 0, 0, 0, 0}, kBig, kBig, kBig, 0, false, 1, false, true, true).reg_ub == 3);  // K = 1: 3 cells
}

void compaction()
{
    // 10 new cells + 5 pending = 15 candidates, 105 registrations at most; 100 registrations + 20 pre-dependants live.
    // dep[] may grow by 2 * 120 + 2 * 105 + 10 = 460 entries.
    auto pass = [](unsigned long long dep, uint64_t max_dep, bool early, bool nowait_knob, bool replay_knob) {
        return plan_clean(CleanHead{10, 33, 5, 100, 20, dep}, kBig, 1000, max_dep, 0, true, 3, early, nowait_knob, replay_knob);
    };
    CleanPlan p = pass(1000, 1460, true, true, true);
    CHECK(p.n_occ == 10 && p.n_normals == 33 && p.n_pend == 5 && p.n_new_occ == 10 && p.n_in == 15 && p.reg_ub == 105 && p.reg_first == 100);
    CHECK(!p.full && p.overlap && p.no_wait && p.replay_early);
    p = pass(1001, 1460, true, true, true);  // one entry more
    CHECK(p.full && !p.overlap && !p.no_wait && !p.replay_early);
    CHECK(pass(1000, 1459, true, true, true).full);
    // replay_early needs all three
    p = pass(1000, 1460, false, true, true);  // not overlapped
    CHECK(!p.full && !p.overlap && p.no_wait && !p.replay_early);
    p = pass(1000, 1460, true, false, true);  // waited
    CHECK(!p.full && p.overlap && !p.no_wait && !p.replay_early);
    p = pass(1000, 1460, true, true, false);  // knob off
    CHECK(!p.full && p.overlap && p.no_wait && !p.replay_early);
    p = fresh_pass(299594, true, true, true);  // waited because it is large
    CHECK(p.overlap && !p.no_wait && !p.replay_early);
}

void clamps()
{
    CleanPlan p = plan_clean(CleanHead{50, 0, 0, 0, 0, 0}, 40, kBig, kBig, 0, false, 3, false, true, true);
    CHECK(p.n_occ == 40 && p.n_new_occ == 40 && p.n_in == 40);
    // 10 new cells, 70 registrations at most: 2 * 70 + 10 = 150 entries besides twice the live ones, each kind cut to max_reg = 1000
    p = plan_clean(CleanHead{10, 0, 0, 5000, 0, 0}, kBig, 1000, 2150, 0, false, 3, false, true, true);
    CHECK(p.reg_first == 1000 && !p.full);
    CHECK(plan_clean(CleanHead{10, 0, 0, 5000, 0, 0}, kBig, 1000, 2149, 0, false, 3, false, true, true).full);
    p = plan_clean(CleanHead{10, 0, 0, 0, 5000, 0}, kBig, 1000, 2150, 0, false, 3, false, true, true);
    CHECK(p.reg_first == 0 && !p.full);
    CHECK(plan_clean(CleanHead{10, 0, 0, 0, 5000, 0}, kBig, 1000, 2149, 0, false, 3, false, true, true).full);
    p = plan_clean(CleanHead{10, 0, 0, 5000, 5000, 0}, kBig, 1000, 4150, 0, false, 3, false, true, true);
    CHECK(!p.full);
    CHECK(plan_clean(CleanHead{10, 0, 0, 5000, 5000, 0}, kBig, 1000, 4149, 0, false, 3, false, true, true).full);
    // the gate has examined more cells than are occupied (after the clamp): no new ones
    p = plan_clean(CleanHead{50, 0, 7, 0, 0, 0}, 40, kBig, kBig, 60, true, 3, false, true, true);
    CHECK(p.n_occ == 40 && p.n_new_occ == 0 && p.n_pend == 7 && p.n_in == 7);
    p = plan_clean(CleanHead{50, 0, 7, 0, 0, 0}, kBig, kBig, kBig, 20, true, 3, false, true, true);
    CHECK(p.n_new_occ == 30 && p.n_in == 37);
    // no valid pending list: its counter is ignored, and with no new cell either there is nothing to do
    p = plan_clean(CleanHead{50, 0, 7, 0, 0, 0}, kBig, kBig, kBig, 50, false, 3, false, true, true);
    CHECK(p.n_pend == 0 && p.n_in == 0 && p.reg_ub == 0);
    p = plan_clean(CleanHead{0, 0, 0, 0, 0, 0}, kBig, kBig, kBig, 0, false, 3, true, true, true);
    CHECK(p.n_occ == 0 && p.n_in == 0);
}

void early_start()
{
    CHECK(clean_starts_early(true, false, true, true, 7, 6));
    CHECK(!clean_starts_early(false, false, true, true, 7, 6));  // knob
    CHECK(!clean_starts_early(true, true, true, true, 7, 6));    // more than one rank
    CHECK(!clean_starts_early(true, false, false, true, 7, 6));  // un-binned
    CHECK(!clean_starts_early(true, false, true, false, 7, 6));  // no mailbox
    CHECK(!clean_starts_early(true, false, true, true, 0, 6));   // the final publish is no longer current
    CHECK(!clean_starts_early(true, false, true, true, 7, 0));   // the call left no early publish
}

void replay()
{
    ReplayPlan r = plan_replay(100000, 65535, false, true, true, 100);
    CHECK(!r.stream && r.walked == 100000 && !r.sort_walked && r.use_marks == 1);
    r = plan_replay(100000, 65536, false, true, true, 100);
    CHECK(r.stream && r.walked == 34464 && r.use_marks == 1);
    r = plan_replay(70000, 200000, false, true, true, 100);  // the single-run count is cut to the touched cells
    CHECK(r.stream && r.walked == 0);
    r = plan_replay(100000, 65536, true, true, true, 100);  // a compacting rebuild
    CHECK(!r.stream && r.walked == 100000 && r.use_marks == 0);
    CHECK(!plan_replay(100000, 65536, false, false, true, 100).stream);  // un-binned
    CHECK(!plan_replay(100000, 65536, false, true, false, 100).stream);  // knob off
    r = plan_replay(0, 0, false, true, true, 100);
    CHECK(!r.stream && r.walked == 0);
    CHECK(!plan_replay(262143, 0, false, true, true, 100).sort_walked);
    CHECK(plan_replay(262144, 0, false, true, true, 100).sort_walked);
    CHECK(plan_replay(262144, 0, true, true, true, 100).sort_walked);
    r = plan_replay(327680, 65536, false, true, true, 100);  // 262144 cells left to walk beside the streamed ones
    CHECK(r.stream && r.walked == 262144 && r.sort_walked);
    r = plan_replay(327680, 65537, false, true, true, 100);
    CHECK(r.stream && r.walked == 262143 && !r.sort_walked);
    // slots = (bricks + 2) * 512: 1024, 1536, 4096, 4608
    CHECK(plan_replay(1, 0, false, true, true, 0).slot_bits == 10);
    CHECK(plan_replay(1, 0, false, true, true, 1).slot_bits == 11);
    CHECK(plan_replay(1, 0, false, true, true, 6).slot_bits == 12);
    CHECK(plan_replay(1, 0, false, true, true, 7).slot_bits == 13);
    CHECK(plan_replay(1, 0, false, true, true, 1ull << 23).slot_bits == 32);  // a 32-bit key at the most
    CHECK(plan_replay(1, 0, false, true, true, 1ull << 30).slot_bits == 32);
}

// The sizes at which a clean pass changes its form: the defaults are pinned, and each field decides at limit - 1 / limit, at its
// default and lowered (what tests/test_gpu_clean_forms.py sets on the device).
static_assert(CleanLimits{}.stream_min_single == 65536, "default of stream_min_single");
static_assert(CleanLimits{}.sort_min_walked == 262144, "default of sort_min_walked");
static_assert(CleanLimits{}.reg_large_min == 262144, "default of reg_large_min");
static_assert(CleanLimits{}.gate4_min == 1048576, "default of gate4_min");
static_assert(CleanLimits{}.nowait_max_reg == 2097152, "default of nowait_max_reg");

void limits()
{
    const CleanLimits def{};
    CleanLimits low{};
    low.stream_min_single = 256;
    low.sort_min_walked = 1024;
    low.reg_large_min = 1024;
    low.gate4_min = 4096;
    low.nowait_max_reg = 700;

    // k_gate: four tiles from gate4_min cells on
    CHECK(gate_tiles(1048575) == 1 && gate_tiles(1048576) == 4 && gate_tiles(0) == 1);
    CHECK(gate_tiles(1048575, def) == 1 && gate_tiles(1048576, def) == 4);
    CHECK(gate_tiles(4095, low) == 1 && gate_tiles(4096, low) == 4);
    // k_register: the large tile count from reg_large_min candidates on
    CHECK(!register_large(262143) && register_large(262144) && !register_large(0));
    CHECK(!register_large(262143, def) && register_large(262144, def));
    CHECK(!register_large(1023, low) && register_large(1024, low));

    // the streaming replay: single-run cells (cut to the touched ones) from stream_min_single on
    ReplayPlan r = plan_replay(100000, 65535, false, true, true, 100, def);
    CHECK(!r.stream && r.walked == 100000);
    r = plan_replay(100000, 65536, false, true, true, 100, def);
    CHECK(r.stream && r.walked == 34464);
    r = plan_replay(1000, 255, false, true, true, 100, low);
    CHECK(!r.stream && r.walked == 1000 && !r.sort_walked);
    r = plan_replay(1000, 256, false, true, true, 100, low);
    CHECK(r.stream && r.walked == 744 && !r.sort_walked && r.use_marks == 1);
    // more single-run cells reported than cells touched: cut, everything streams, nothing is walked or sorted
    r = plan_replay(300, 70000, false, true, true, 100, low);
    CHECK(r.stream && r.walked == 0 && !r.sort_walked);
    r = plan_replay(255, 70000, false, true, true, 100, low);  // ... and the cut count decides
    CHECK(!r.stream && r.walked == 255);
    r = plan_replay(65535, 1ull << 40, false, true, true, 100);
    CHECK(!r.stream && r.walked == 65535);
    r = plan_replay(65536, 1ull << 40, false, true, true, 100);
    CHECK(r.stream && r.walked == 0 && !r.sort_walked);
    // a compacting rebuild never streams and leaves no notes, however many single-run cells and however low the limit
    r = plan_replay(5000, 5000, true, true, true, 100, low);
    CHECK(!r.stream && r.walked == 5000 && r.sort_walked && r.use_marks == 0);
    r = plan_replay(1ull << 20, 1ull << 20, true, true, true, 100);
    CHECK(!r.stream && r.walked == (1ull << 20) && r.sort_walked && r.use_marks == 0);
    CHECK(!plan_replay(5000, 5000, false, false, true, 100, low).stream);  // un-binned
    CHECK(!plan_replay(5000, 5000, false, true, false, 100, low).stream);  // knob off

    // the sorted walk: from sort_min_walked walked cells on, counted behind what streams
    CHECK(!plan_replay(262143, 0, false, true, true, 100, def).sort_walked);
    CHECK(plan_replay(262144, 0, false, true, true, 100, def).sort_walked);
    CHECK(!plan_replay(1023, 0, false, true, true, 100, low).sort_walked);
    CHECK(plan_replay(1024, 0, false, true, true, 100, low).sort_walked);
    r = plan_replay(1280, 256, false, true, true, 100, low);  // 1024 left to walk
    CHECK(r.stream && r.walked == 1024 && r.sort_walked);
    r = plan_replay(1280, 257, false, true, true, 100, low);
    CHECK(r.stream && r.walked == 1023 && !r.sort_walked);
    CHECK(plan_replay(1280, 256, false, true, true, 6, low).slot_bits == 12);  // the key bits do not depend on the limits

    // a SMALL pass: registration bound below nowait_max_reg (K = 3: 7 per candidate)
    auto fresh = [](uint64_t n_in, const CleanLimits& lim) {
        return plan_clean(CleanHead{n_in, 0, 0, 0, 0, 0}, kBig, kBig, kBig, 0, false, 3, true, true, true, lim);
    };
    CleanPlan p = fresh(299593, def);
    CHECK(p.reg_ub == 2097151 && p.no_wait && p.replay_early);
    p = fresh(299594, def);
    CHECK(p.reg_ub == 2097158 && !p.no_wait && !p.replay_early && p.overlap);
    p = fresh(99, low);  // 693 < 700
    CHECK(p.reg_ub == 693 && p.no_wait && p.replay_early);
    p = fresh(100, low);  // 700
    CHECK(p.reg_ub == 700 && !p.no_wait && !p.replay_early && p.overlap && !p.full);
    // the other limits do not enter plan_clean
    CleanLimits other = low;
    other.nowait_max_reg = def.nowait_max_reg;
    CHECK(fresh(299593, other).no_wait && !fresh(299594, other).no_wait);
}

void probe()
{
    CHECK(probe_frames_for(1) == 8 && probe_frames_for(63) == 8);
    CHECK(probe_frames_for(64) == 16 && probe_frames_for(65535) == 16);
    CHECK(!wants_probe(true, false, 8, 8) && wants_probe(true, false, 9, 8));
    CHECK(!wants_probe(true, false, 16, 16) && wants_probe(true, false, 17, 16));
    CHECK(!wants_probe(true, true, 100, 16));   // a plan already
    CHECK(!wants_probe(false, false, 100, 16));  // the un-binned forms
}

void tiles()
{
    CHECK(tile_row_width(640, 640 * 480) == 640);
    CHECK(tile_row_width(636, 636 * 480) == 0);
    CHECK(tile_row_width(640, 640 * 472) == 0);
    CHECK(tile_row_width(640, 640 * 480 + 1) == 0);
    CHECK(tile_row_width(0, 640 * 480) == 0);
    CHECK(tile_row_width(8, 8 * 16) == 0);
    CHECK(tile_row_width(16, 16 * 16) == 16);
}

// binned, a plan from the launch before, `known` bricks of which `before` at the read-back before: slack 2.0, spare regions on
BinState bins(uint64_t known, uint64_t before, uint64_t max_bricks)
{
    return BinState{true, true, false, known, before, max_bricks, 1000000.0, true, 2.0f, 1.0f};
}

void bin_plans()
{
    BinState s = bins(1000, 0, 100000);
    s.have_hist = false;
    BinPlan p = plan_bins(s, 1000000);
    CHECK(!p.have_plan && p.spare == 0 && p.spare_cap == 0 && p.nb_known == 1000 && p.nb == 1000);
    p = plan_bins(bins(0, 0, 100000), 1000000);
    CHECK(!p.have_plan && p.spare == 0 && p.nb == 0 && p.pool == 4125128 && !p.too_large);  // 4.125 per point + 128 per brick and one more
    s = bins(1000, 0, 100000);
    s.bin = false;
    p = plan_bins(s, 1000000);
    CHECK(!p.have_plan && p.pool == 0 && !p.too_large && p.nb == 1000);

    // spare regions: twice the growth, 256 at least, half the known bricks (or 256) at most, and never past max_bricks
    p = plan_bins(bins(10000, 10000, 100000), 1000000);
    CHECK(p.have_plan && p.spare == 256 && p.nb == 10256 && p.nb_known == 10000);
    CHECK(p.spare_cap == 100 && p.pool == 5456328);  // 4125000 + 128 * 10001 + 2 * 256 * 100
    CHECK(plan_bins(bins(10000, 20000, 100000), 1000000).spare == 256);  // (a count that went back: no growth)
    CHECK(plan_bins(bins(10000, 9000, 100000), 1000000).spare == 2000);
    CHECK(plan_bins(bins(10000, 0, 100000), 1000000).spare == 5000);
    CHECK(plan_bins(bins(300, 0, 100000), 1000000).spare == 256);
    CHECK(plan_bins(bins(100, 0, 100000), 1000000).spare == 256);
    CHECK(plan_bins(bins(10000, 0, 10100), 1000000).spare == 100);
    p = plan_bins(bins(10000, 0, 10000), 1000000);
    CHECK(p.have_plan && p.spare == 0 && p.spare_cap == 0 && p.nb == 10000 && p.pool == 5405128);
    CHECK(plan_bins(bins(10000, 0, 9000), 1000000).spare == 0);
    s = bins(10000, 0, 100000);
    s.knob_spare = false;
    p = plan_bins(s, 1000000);
    CHECK(p.have_plan && p.spare == 0 && p.spare_cap == 0 && p.nb == 10000);

    // a spare region: an average brick's share of the batch, 64 at least, 2^15 at most
    CHECK(plan_bins(bins(10000, 10000, 100000), 100000).spare_cap == 64);
    CHECK(plan_bins(bins(10000, 10000, 100000), 639999).spare_cap == 64);
    CHECK(plan_bins(bins(10000, 10000, 100000), 650000).spare_cap == 65);
    CHECK(plan_bins(bins(10000, 10000, 100000), 327680000).spare_cap == 32768);
    CHECK(plan_bins(bins(10000, 10000, 100000), 400000000).spare_cap == 32768);
    // ... and no more than the room under 2^32 - 1 holds: 1040000000 points and one brick take 4290000000 + 256 entries, which leaves
    // 4967039; 256 spare bricks with two regions each get 4967039 / 512 = 9701 entries a region instead of 32768
    p = plan_bins(bins(1, 0, 100000), 1040000000);
    CHECK(p.spare == 256 && p.spare_cap == 9701 && p.pool == 4294967168ull && !p.too_large);

    // the 32-bit pool: 33 entries for 8 points (slack 2.0), 128 per brick and one more; no spare regions
    s = bins(23, 0, 100000);
    s.knob_spare = false;
    p = plan_bins(s, 1041203448);  // 130150431 * 33 + 24 * 128
    CHECK(p.pool == 0xFFFFFFFFull && !p.too_large);
    p = plan_bins(s, 1041203449);  // 4 more
    CHECK(p.pool == 4294967299ull && p.too_large);
    s = bins(32, 0, 100000);
    s.knob_spare = false;
    p = plan_bins(s, 1041203169);  // 130150396 * 33 + 4 + 33 * 128
    CHECK(p.pool == 4294967296ull && p.too_large);

    // the pool counts a slack below 1.5 as 1.5: 3.125 per point
    s = bins(9, 9, 9);
    s.knob_slack = 1.0f;
    CHECK(plan_bins(s, 1000).pool == 3125 + 1280);
    s.knob_slack = 3.0f;
    CHECK(plan_bins(s, 1000).pool == 6125 + 1280);

    // k_bin_plan's slack: the knob, but 1.5 at least for a plan from the dry run's sample
    s = bins(1000, 0, 100000);
    CHECK(plan_bins(s, 1000).slack == 2.0f);
    s.from_probe = true;
    CHECK(plan_bins(s, 1000).slack == 2.0f);
    s.knob_slack = 1.25f;
    CHECK(plan_bins(s, 1000).slack == 1.5f);
    s.from_probe = false;
    CHECK(plan_bins(s, 1000).slack == 1.25f);
    // ... and its scale: this launch's points over the previous launch's (one at least), times the test knob
    s = bins(1000, 0, 100000);
    CHECK(plan_bins(s, 2000000).scale == 2.0f && plan_bins(s, 250000).scale == 0.25f);
    s.test_scale = 0.5f;
    CHECK(plan_bins(s, 2000000).scale == 1.0f);
    s.prev_points = 0.0;
    CHECK(plan_bins(s, 2000).scale == 1000.0f);
}

void order()
{
    CHECK(is_batch(4, true) && !is_batch(3, true) && !is_batch(100, false));
    OrderPlan o = plan_order(5, false, true, true, 4, false);
    CHECK(o.update && o.buffer_first && o.final_publish);
    o = plan_order(0, true, true, true, 4, false);  // the host's record count may lag behind a pass that was not waited for
    CHECK(o.update && o.buffer_first && o.final_publish);
    o = plan_order(0, false, true, true, 4, false);  // no update kernel
    CHECK(!o.update && !o.buffer_first && o.final_publish);
    o = plan_order(5, false, false, true, 4, false);  // knob off
    CHECK(o.update && !o.buffer_first && o.final_publish);
    o = plan_order(5, false, true, false, 4, false);  // no mailbox
    CHECK(o.update && !o.buffer_first && !o.final_publish);
    o = plan_order(5, false, true, true, 3, false);  // three frames
    CHECK(o.update && !o.buffer_first && !o.final_publish);
    o = plan_order(5, false, true, true, 4, true);  // more than one rank
    CHECK(o.update && !o.buffer_first && o.final_publish);
}

void shape()
{
    // a window of 2 misses and 1000 member pairs is exactly one in 500
    CHECK(!update_shape_goes_wide(12, 6000, 10, 5000));
    CHECK(update_shape_goes_wide(13, 6000, 10, 5000));
    CHECK(update_shape_goes_wide(12, 5999, 10, 5000));
    CHECK(!update_shape_goes_wide(10, 5000, 10, 5000));  // an empty window
    CHECK(!update_shape_goes_wide(9, 5000, 10, 5000));
    // after a restore the member count may lie below the one seen: a window of no members
    CHECK(update_shape_goes_wide(11, 100, 10, 5000));
    CHECK(!update_shape_goes_wide(10, 100, 10, 5000));
}

}  // namespace

int main()
{
    small_pass();
    compaction();
    clamps();
    early_start();
    replay();
    limits();
    probe();
    tiles();
    bin_plans();
    order();
    shape();
    if (g_failures) {
        std::fprintf(stderr, "%d checks failed\n", g_failures);
        return 1;
    }
    std::printf("host_plan ok\n");
    return 0;
}
