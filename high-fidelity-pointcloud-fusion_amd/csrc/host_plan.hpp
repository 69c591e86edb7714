// csrc/host_plan.hpp -- what kind of integrate call or clean pass this is.  Host only and free of HIP, so g++ alone compiles it
// (tests/host_plan_check.cpp).
//
// Pure functions over counters, capacities, knobs and session fields: they decide and count, and nothing else.  The two functions that
// enqueue (integrate_device_locked and clean_locked) read a const plan from here; launch geometry stays at the launch
// sites, with the kernels' tile constants.  The defaults of the clean pass's thresholds (CleanLimits) lie far beyond what a test can
// reach in seconds on the device: the plan functions take them as a parameter, tests/host_plan_check.cpp pins the defaults, and a
// device test lowers them (HFPF_TEST_*_MIN) so that frames of test size take the forms behind them (tests/test_gpu_clean_forms.py).
#pragma once

#include <algorithm>
#include <cstdint>

namespace hfpf {

#ifndef HFPF_PROBE_FRAMES
#define HFPF_PROBE_FRAMES 8
#endif
constexpr int kProbeFrames = HFPF_PROBE_FRAMES;  // frames of a plan-less batch that go ahead of the rest to measure the per-brick demand
constexpr uint64_t kSlotsPerBrick = 512;         // = kBrickCells (tables.hpp)

// ---- the clean pass ----

// The sizes at which a clean pass changes its form.  The defaults are what every session runs with; only tests set others.
struct CleanLimits {
    uint64_t stream_min_single = 1ull << 16;  // touched cells in single-run bricks from which the replay streams their runs (plan_replay)
    uint64_t sort_min_walked = 1ull << 18;    // cells of the chain walk from which they are sorted into slot order first (plan_replay)
    uint64_t reg_large_min = 1ull << 18;      // candidates from which k_register takes its large tile count (register_large)
    uint64_t gate4_min = 1ull << 20;          // cells from which k_gate takes four tiles per workgroup (gate_tiles)
    uint64_t nowait_max_reg = 1ull << 21;     // registration bound below which a pass is SMALL (plan_clean)
};

// Tiles per workgroup of k_gate over n cells (pending + new): four only when the input is large enough to fill the device that way.
inline int gate_tiles(uint64_t n, const CleanLimits& lim = CleanLimits{}) { return n >= lim.gate4_min ? 4 : 1; }
// k_register over n_in candidates: kRegTilesLarge tiles per workgroup (kernels.hpp) or kRegTilesSmall.
inline bool register_large(uint64_t n_in, const CleanLimits& lim = CleanLimits{}) { return n_in >= lim.reg_large_min; }

// The pass may take its head-of-pass counters from the early publish of the integrate call before it (evaluated before that read-back).
inline bool clean_starts_early(bool clean_overlap, bool dist_on, bool binned, bool has_mailbox, unsigned long long pub_seq, unsigned long long early_seq)
{
    return clean_overlap && !dist_on && binned && has_mailbox && pub_seq && early_seq;
}

struct CleanHead {  // the counter words as the head-of-pass read-back found them
    unsigned long long occ, normals, pend, reg, prereg, dep;
};
struct CleanPlan {
    uint64_t n_occ, n_normals;
    uint64_t n_pend;     // cells the previous pass left without a normal (pend_a)
    uint64_t n_new_occ;  // cells occupied since the last pass (new tail of occ_list)
    uint64_t n_in;       // candidates = the two together: upper bound of everything this pass can produce per candidate.  0 (or n_occ == 0): nothing to do
    uint64_t reg_ub;     // bound of the pass's registration counts; the kernels read the exact counts on the device
    uint64_t reg_first;  // registrations already present in dep[]: every pass files all of its own, so that is the counter as this pass found it
    bool full;           // a compacting rebuild of the dependant table instead of the incremental update
    bool overlap;        // the front half beside the update kernel
    bool no_wait;        // a SMALL pass: no mid-pass read-back
    bool replay_early;   // the replay too goes beside the update kernel
};
inline CleanPlan plan_clean(const CleanHead& c, uint64_t max_occ, uint64_t max_reg, uint64_t max_dep, uint64_t gate_done, bool pend_valid, int K, bool early,
                            bool clean_small_nowait, bool early_replay, const CleanLimits& lim = CleanLimits{})
{
    CleanPlan p{};
    p.n_occ = std::min<uint64_t>(c.occ, max_occ);
    p.n_normals = c.normals;
    p.n_pend = pend_valid ? c.pend : 0;
    p.n_new_occ = p.n_occ - std::min(p.n_occ, gate_done);
    p.n_in = p.n_pend + p.n_new_occ;
    // The registration counts of this pass are bounded by (2K+1) * n_in; the kernels read the exact counts from the device counters
    // (kCountOnDevice), and the host picks the values up at the read-back after them.
    p.reg_ub = (2ull * (uint64_t)K + 1ull) * p.n_in;
    // Incremental update of the dependant table, or a compacting rebuild?  A conservative space estimate decides (C_DEP as of the
    // head-of-pass read-back: nothing has changed it since).  What one incremental update can take from dep[]: a block of the next
    // power-of-two capacity for every list that outgrows its own (kernels.hpp dep_capacity) -- below twice its new length, i.e.
    // at most twice (all live entries: registrations + filed pre-dependants so far, + the registration bound of this pass) -- and
    // one entry per cell occupied since the last pass (the pre-dependants filed at the head of the pass).
    const uint64_t live_ub = std::min<uint64_t>(c.reg, max_reg) + std::min<uint64_t>(c.prereg, max_reg);
    p.full = c.dep + 2 * live_ub + 2 * p.reg_ub + p.n_new_occ > max_dep;
    p.overlap = early && !p.full;
    p.reg_first = std::min<uint64_t>(c.reg, max_reg);
    // A pass is SMALL when its upper bounds are: then the replay is launched over the bound and reads its count on the device,
    // and the host does not wait for the pass at all (no mid-pass read-back: the GPU is not left idle for a host round trip, and
    // the next integrate call is enqueued behind the pass at once).  The bound above makes sure the pass cannot run out of dep[]
    // half-way (the one overflow the host would have to repair by compacting).
    p.no_wait = !p.full && p.reg_ub < lim.nowait_max_reg && clean_small_nowait;
    p.replay_early = p.overlap && p.no_wait && early_replay;
    return p;
}

// The buffer replay of the inc_touched cells that gained registrants in a waited pass (full: behind a compacting rebuild, planned or not).
struct ReplayPlan {
    bool stream;         // the bricks of one contiguous log run replay by streaming it; the chain walk takes the other cells
    uint64_t walked;     // cells the chain walk has work for (0: no walk)
    bool sort_walked;    // ... in slot order
    unsigned slot_bits;  // key bits of that sort: slot = brick * 512 + cell
    uint32_t use_marks;  // (a compacting rebuild leaves no notes and the lists in no particular order)
};
inline ReplayPlan plan_replay(uint64_t inc_touched, unsigned long long touched_single, bool full, bool binned, bool stream_replay, uint64_t n_bricks_known,
                              const CleanLimits& lim = CleanLimits{})
{
    ReplayPlan r{};
    r.use_marks = full ? 0u : 1u;
    // Bricks whose buffered points are ONE contiguous run of the log (the epoch was handed over in one integrate call, the
    // brick is new in it) replay by streaming that run: worth its launch over every brick when enough of the touched cells
    // lie in such bricks.  The chain walk takes the others.
    const uint64_t single = full ? 0 : std::min<uint64_t>(touched_single, inc_touched);
    r.stream = !full && binned && stream_replay && single >= lim.stream_min_single;
    r.walked = r.stream ? inc_touched - single : inc_touched;
    // a 256-point tile appends consecutive log entries for neighbouring cells, so walking the cells in slot (brick-major)
    // order lets adjacent lanes share cache lines of the log; a short list is not worth the sort's launches
    r.sort_walked = r.walked >= lim.sort_min_walked;
    r.slot_bits = 9;  // the brick count is as of the read-back just ahead of the replay
    while ((1ull << r.slot_bits) < (n_bricks_known + 2) * kSlotsPerBrick && r.slot_bits < 32) r.slot_bits++;
    return r;
}

// ---- the integrate call ----

// frames of the dry run: twice as many for a long batch.  For 150 frames of 640x480 with random poses the first 8 find 46 % of
// the bricks the batch touches and 16 find 50 % (32: 57 %), and the plan made from the larger sample sends 30 % fewer points
// through the overflow list (268 K instead of 382 K per 1000-frame pass): whole job +1.5 %; 32 frames add nothing.
inline uint32_t probe_frames_for(uint32_t n_frames) { return n_frames >= 8u * (uint32_t)kProbeFrames ? 2u * (uint32_t)kProbeFrames : (uint32_t)kProbeFrames; }
// No plan for the per-brick bins yet (first batch of a session): batches of up to probe_frames frames just take the direct forms.
inline bool wants_probe(bool bin, bool bin_have_hist, uint32_t n_frames, uint32_t probe_frames) { return bin && !bin_have_hist && n_frames > probe_frames; }

// 16x16-pixel tiles when the caller told us the image width and the frame tiles exactly (0: none)
inline uint32_t tile_row_width(uint32_t fw, uint32_t n_points) { return (fw >= 16 && fw % 16 == 0 && n_points % fw == 0 && (n_points / fw) % 16 == 0) ? fw : 0u; }

// Entries the bin pool of a launch of `pts` points needs: every brick has two regions, each planned for the brick's whole demand of
// the previous launch x slack (x 1.5 at least when the plan comes from the dry run's sample) + 64.
inline uint64_t bin_pool_entries(float bin_slack, uint64_t pts, uint64_t bricks)
{
    const double per_point = 2.0 * std::max(1.5, (double)bin_slack) + 0.125;
    return (uint64_t)(per_point * (double)pts) + 128ull * (bricks + 1);
}

struct BinState {  // what plan_bins reads of the handle: session fields (as of the dry run's read-back, where there was one), a capacity, knobs
    bool bin, have_hist, from_probe;
    uint64_t n_bricks_known, n_bricks_before, max_bricks;
    double prev_points;
    bool knob_spare;
    float knob_slack, test_scale;
};
struct BinPlan {
    bool have_plan;      // per-brick bin regions sized from the previous launch's demand; without one nothing is parked (direct forms)
    uint32_t nb_known;
    uint32_t spare;      // regions for bricks this launch may discover ...
    uint32_t spare_cap;  // ... of this many entries each
    uint32_t nb;         // bricks the per-brick kernels of this call look at
    uint64_t pool;       // entries for this launch's parked points (+25 % plan slack, +64 per brick)
    bool too_large;      // ... more than a 32-bit index addresses
    float scale, slack;  // k_bin_plan: this launch's points over the previous one's; capacity over demand
};
inline BinPlan plan_bins(const BinState& s, uint64_t pts)
{
    BinPlan p{};
    p.nb_known = (uint32_t)s.n_bricks_known;
    p.have_plan = s.bin && s.have_hist && p.nb_known > 0;
    // Bricks this launch may discover get spare regions of an average brick's size: as many as the session found between its last
    // two counter read-backs (x2), i.e. half the known bricks right after the dry run and a few hundred in the steady state.
    if (p.have_plan && s.knob_spare) {
        const uint64_t grown = s.n_bricks_known - std::min(s.n_bricks_known, s.n_bricks_before);
        p.spare = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(2 * grown, 256), std::max<uint64_t>(p.nb_known / 2, 256));
        p.spare = (uint32_t)std::min<uint64_t>(p.spare, s.max_bricks - std::min<uint64_t>(s.max_bricks, p.nb_known));
    }
    p.nb = p.nb_known + p.spare;
    if (s.bin) {
        p.pool = bin_pool_entries(s.knob_slack, pts, p.nb_known);  // two regions per brick, each sized for the whole brick
        if (p.spare) {  // an average brick's share of the batch, both regions, within what a 32-bit index still addresses
            p.spare_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(pts / std::max(1u, p.nb_known), 64), 1u << 15);
            const uint64_t room = 0xFFFFFFFFull - std::min<uint64_t>(p.pool, 0xFFFFFFFFull);
            if (2ull * p.spare * p.spare_cap > room) p.spare_cap = (uint32_t)(room / (2ull * p.spare));
            p.pool += 2ull * p.spare * p.spare_cap;
        }
    }
    p.too_large = p.pool > 0xFFFFFFFFull;
    p.scale = (float)((double)pts / std::max(1.0, s.prev_points)) * s.test_scale;
    p.slack = s.from_probe ? std::max(1.5f, s.knob_slack) : s.knob_slack;  // a plan from a sample: more slack per region
    return p;
}

// A batch: the next call is probably a clean pass, which starts by reading the counters.
inline bool is_batch(uint32_t n_frames, bool has_mailbox) { return has_mailbox && n_frames >= 4; }

struct OrderPlan {
    bool update;  // a clean pass has run: unoccupied cells may carry a dependant.  Without a normal record no cell has dependants: no update kernel
    // k_buffer ahead of the update kernel (both only read the bins, and they write disjoint tables): everything a clean
    // pass reads at its head is then final while the update kernel -- the longer of the two by far -- still runs, and an
    // early publish + ev_ready let the pass begin beside it (clean_locked).  Only where that can happen: a batch on a
    // single rank with the mailbox; otherwise the order of old.
    bool buffer_first;
    bool final_publish;  // the call ends with a publish of the counters
};
inline OrderPlan plan_order(unsigned long long c_normals, bool normals_possible, bool clean_overlap, bool has_mailbox, uint32_t n_frames, bool dist_on)
{
    OrderPlan o{};
    o.update = c_normals > 0 || normals_possible;
    o.final_publish = is_batch(n_frames, has_mailbox);
    o.buffer_first = o.update && clean_overlap && o.final_publish && !dist_on;
    return o;
}

// k_update_cells leaves its dense shape when the items that found no slot in its table exceed one in 500 member pairs of the window
// since (miss_seen, member_seen).  A member count below member_seen (after a restore) is an empty window.
inline bool update_shape_goes_wide(unsigned long long miss, unsigned long long member, unsigned long long miss_seen, unsigned long long member_seen)
{
    return miss > miss_seen && (miss - miss_seen) * 500ull > member - std::min(member, member_seen);
}

// ---- the depth-consistency read-out ----

constexpr uint32_t kConsChunkFrames = 64;       // frames per chunk at most: their poses sit in LDS (6 KB), as a render's views do
constexpr uint32_t kConsRowTile = 256;          // rows per workgroup of k_consistency
constexpr uint32_t kConsLaunchChunks = 32768;   // chunks per launch at most (grid.y)

// How k_consistency walks `frames` frames for `rows` rows: chunk c of a span holds frames [c * frames_per_chunk, min(frames,
// (c + 1) * frames_per_chunk)), and a launch takes chunks_per_launch chunks (the last launch fewer).  A workgroup is one row tile x
// one chunk.  Few row tiles: shorter chunks, so that tiles x chunks reaches four workgroups per compute unit; many: whole chunks of
// 64, since every chunk costs a row its atomics.  `forced` (HFPF_CONSISTENCY_CHUNK, 1..64; 0 = none) overrides the chunk length.
struct ConsPlan {
    uint32_t frames_per_chunk;   // 1..64 (1 when there are no frames)
    uint32_t n_chunks;           // ceil(frames / frames_per_chunk)
    uint32_t chunks_per_launch;  // 1..kConsLaunchChunks
    bool single;                 // one chunk covers every frame: the records need no atomics
};
inline ConsPlan plan_consistency(uint64_t rows, uint32_t frames, uint32_t compute_units, uint32_t forced = 0)
{
    ConsPlan p{};
    const uint64_t tiles = std::max<uint64_t>(1, (rows + kConsRowTile - 1) / kConsRowTile);
    const uint64_t want_groups = 4ull * std::max(1u, compute_units);
    const uint64_t want_chunks = std::max<uint64_t>(1, (want_groups + tiles - 1) / tiles);
    uint64_t per = (frames + want_chunks - 1) / want_chunks;
    if (forced) per = forced;
    p.frames_per_chunk = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(per, 1), kConsChunkFrames);
    p.n_chunks = (frames + p.frames_per_chunk - 1) / p.frames_per_chunk;
    p.chunks_per_launch = std::min(std::max(p.n_chunks, 1u), kConsLaunchChunks);
    p.single = p.n_chunks <= 1;
    return p;
}

// ---- hidden rows (hfpf_hide_*, include/hfpf.h) ----

constexpr uint32_t kHideOpHide = 1, kHideOpShow = 2, kHideOpOthers = 3;  // = HFPF_HIDE, HFPF_SHOW, HFPF_HIDE_OTHERS
constexpr uint32_t kHideVoxelBytes = 12, kHideSelectBytes = 4;           // what an entry reads at its voxel / its selector word
constexpr uint64_t kHideLaunchEntries = 1ull << 30;                      // entries per launch of the mark kernel at most

inline bool hide_op_ok(uint32_t op) { return op == kHideOpHide || op == kHideOpShow || op == kHideOpOthers; }
// the fields of hfpf_hide_opts (expect = its sizeof)
inline bool hide_opts_ok(uint32_t struct_size, uint32_t expect, uint32_t op, uint32_t flags, uint32_t reserved)
{
    return struct_size == expect && hide_op_ok(op) && flags == 0 && reserved == 0;
}
inline bool hide_stride_ok(uint32_t stride, uint32_t least) { return stride >= least && stride % 4 == 0; }
// the list of a call: the select stride counts only with a selector; a NULL list must be empty
inline bool hide_list_ok(bool have_voxels, uint64_t n, uint32_t voxel_stride, bool have_select, uint32_t select_stride)
{
    if (!hide_stride_ok(voxel_stride, kHideVoxelBytes)) return false;
    if (have_select && !hide_stride_ok(select_stride, kHideSelectBytes)) return false;
    return have_voxels || n == 0;
}
inline bool hide_device_aligned(uint64_t voxels_addr, uint64_t select_addr) { return ((voxels_addr | select_addr) & 3u) == 0; }

// One (brick, x-plane) word of H under an op: old = its HIDDEN bits, mark = the matched cells, found = its normal_found bits (F).
// constexpr, so that the apply kernel and tests/hide_plan_check.cpp run the same line.
constexpr uint64_t hide_word_op(uint32_t op, uint64_t old, uint64_t mark, uint64_t found)
{
    const uint64_t m = mark & found;
    return op == kHideOpHide ? (old | m) : op == kHideOpShow ? (old & ~m) : (old | (found & ~m));
}

// The box of hfpf_hide_box against the grid: inclusive voxel indices, may reach outside 0..dim-1, lo > hi on an axis = empty.
struct HideBox {
    int32_t lo[3], hi[3];  // clipped to 0..dim-1 (meaningless when empty)
    bool empty;
};
inline HideBox clip_hide_box(const int32_t lo[3], const int32_t hi[3], const int32_t dim[3])
{
    HideBox b{};
    for (int a = 0; a < 3; a++) {
        b.lo[a] = std::max<int32_t>(lo[a], 0);
        b.hi[a] = std::min<int32_t>(hi[a], dim[a] - 1);
        if (b.lo[a] > b.hi[a]) b.empty = true;
    }
    return b;
}

// Host lists go up in chunks: entries per upload (one at least), so that neither array's span exceeds chunk_bytes ...
inline uint64_t hide_entries_per_upload(uint32_t voxel_stride, bool have_select, uint32_t select_stride, uint64_t chunk_bytes)
{
    const uint64_t stride = std::max<uint64_t>(voxel_stride, have_select ? select_stride : 0);
    return std::max<uint64_t>(1, chunk_bytes / std::max<uint64_t>(stride, 1));
}
// ... and the bytes n > 0 entries of `stride` span when each reads `item` bytes (nothing behind the last entry's item is read)
inline uint64_t hide_span_bytes(uint64_t n, uint32_t stride, uint32_t item) { return (n - 1) * (uint64_t)stride + item; }

// A snapshot carries the HIDDEN section only when something is hidden: a blob of a handle with H empty is the blob of old.
inline bool snapshot_carries_hidden(uint64_t n_hidden) { return n_hidden != 0; }

// ---- planar sections of a mesh (hfpf_section_mesh*, include/hfpf.h) ----

constexpr uint32_t kSecChunkPlanes = 64;             // planes per launch of k_section: they sit in LDS (2 KB), as a consistency chunk's poses do
constexpr uint32_t kSecMaxPlanes = 4096;             // = HFPF_SECTION_MAX_PLANES: 12 bits of a key
constexpr uint64_t kSecMaxVerts = 1ull << 26;        // 26 bits of a key per vertex index
constexpr uint64_t kSecPlaneCap = 1ull << 20;        // = HFPF_SECTION_MAX_PLANE_SEGMENTS: keeps the q32 and q28 sums below 2^62
constexpr uint64_t kSecTotalCap = (1ull << 31) - 1;  // segments of a call: twice as many points still have 32-bit ids
constexpr uint32_t kSecTriTile = 256;                // triangles per workgroup of k_section
constexpr unsigned kSecSegKeyBits = 44, kSecPointKeyBits = 64;  // what the two sorts compare

// A point's key: plane | va | vb with va < vb, so that ascending keys are ascending (plane, va, vb).  constexpr: the kernels and
// tests/section_plan_check.cpp run the same lines.
constexpr uint64_t sec_point_key(uint32_t plane, uint32_t a, uint32_t b)
{
    return ((uint64_t)plane << 52) | ((uint64_t)(a < b ? a : b) << 26) | (uint64_t)(a < b ? b : a);
}
constexpr uint32_t sec_key_plane(uint64_t key) { return (uint32_t)(key >> 52); }
constexpr uint32_t sec_key_va(uint64_t key) { return (uint32_t)(key >> 26) & 0x3FFFFFFu; }
constexpr uint32_t sec_key_vb(uint64_t key) { return (uint32_t)key & 0x3FFFFFFu; }
// A segment's key: plane | triangle (n_tris < 2^32 - 1); ascending keys are ascending (plane, triangle).
constexpr uint64_t sec_segment_key(uint32_t plane, uint32_t tri) { return ((uint64_t)plane << 32) | tri; }
constexpr uint32_t sec_seg_plane(uint64_t key) { return (uint32_t)(key >> 32); }
constexpr uint32_t sec_seg_tri(uint64_t key) { return (uint32_t)key; }

// The counts of a call that need no pointer: 0 = fine, else the text of the fault.
inline const char* section_counts_fault(uint64_t n_verts, uint64_t n_tris, uint64_t n_planes)
{
    if (n_verts > kSecMaxVerts) return "n_verts must not exceed 2^26";
    if (n_tris >= 0xFFFFFFFFull) return "n_tris must stay below 2^32 - 1";
    if (n_planes > kSecMaxPlanes) return "n_planes must not exceed 4096";
    return nullptr;
}
// One plane (n.x, n.y, n.z, d): all four finite, nn = dot(n, n) finite and > 0, evaluated as the contract writes it.
inline bool section_plane_ok(const double* p)
{
    for (int i = 0; i < 4; i++)
        if (!(p[i] - p[i] == 0.0)) return false;  // false for an infinity and for a NaN
    const double nn = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
    return nn - nn == 0.0 && nn > 0.0;
}
// The first plane of n that fails, or n.
inline uint32_t section_first_bad_plane(const double* planes, uint32_t n)
{
    for (uint32_t j = 0; j < n; j++)
        if (!section_plane_ok(planes + 4ull * j)) return j;
    return n;
}

// How k_section walks the planes: chunk c holds planes [64 c, min(n, 64 (c + 1))); a call without planes still runs one (empty)
// chunk, which counts the triangles.  The grid is one lane per triangle, one workgroup at least.
inline uint32_t section_chunks(uint32_t n_planes) { return std::max(1u, (n_planes + kSecChunkPlanes - 1) / kSecChunkPlanes); }
inline uint32_t section_chunk_planes(uint32_t n_planes, uint32_t chunk)
{
    const uint64_t first = (uint64_t)chunk * kSecChunkPlanes;
    return first >= n_planes ? 0u : (uint32_t)std::min<uint64_t>(kSecChunkPlanes, n_planes - first);
}
inline uint32_t section_grid(uint64_t n_tris) { return (uint32_t)std::max<uint64_t>(1, (n_tris + kSecTriTile - 1) / kSecTriTile); }

// The cap test over the per-plane segment counts: the first plane beyond kSecPlaneCap (and its count), else the total beyond
// kSecTotalCap (plane = n_planes), else fine.  first[] (n_planes + 1 entries, when not NULL) gets the exclusive sums.
struct SecCapFault {
    bool over;
    uint32_t plane;  // n_planes: the total is what exceeds
    uint64_t count;
};
inline SecCapFault section_cap_test(const uint32_t* counts, uint32_t n_planes, uint64_t* first, uint64_t plane_cap = kSecPlaneCap, uint64_t total_cap = kSecTotalCap)
{
    uint64_t total = 0;
    SecCapFault bad{false, 0, 0};
    for (uint32_t j = 0; j < n_planes; j++) {
        if (first) first[j] = total;
        if (!bad.over && counts[j] > plane_cap) bad = SecCapFault{true, j, counts[j]};
        total += counts[j];
    }
    if (first) first[n_planes] = total;
    if (!bad.over && total > total_cap) bad = SecCapFault{true, n_planes, total};
    if (!bad.over) bad.count = total;
    return bad;
}

// ---- open edges of a mesh (hfpf_mesh_topology*, include/hfpf.h) ----

constexpr uint64_t kTopMaxVerts = 1ull << 26;      // = HFPF_TOPOLOGY_MAX_VERTS: 26 bits of an edge key per vertex index
constexpr uint64_t kTopMaxHalfEdges = 1ull << 32;  // 3 n_tris stays below it: a half-edge id is the sort's 32-bit value
constexpr unsigned kTopKeyBits = 52;               // what the sort compares: va | vb
constexpr uint64_t kTopForward = 1ull << 52;       // above the compared bits: the half-edge runs va -> vb
constexpr uint64_t kTopSkipped = ~0ull;            // the key of a skipped triangle's slots: behind every edge (an edge has va < vb)
constexpr uint32_t kTopNone = 0xFFFFFFFFu;         // = HFPF_TOPOLOGY_NONE
constexpr uint32_t kTopBoundary = 1u, kTopNonManifold = 2u, kTopMiswound = 3u;  // hfpf_topology_edge.kind; 0 = INTERIOR, never listed

// A half-edge's key from its two indices in the triangle's order.
constexpr uint64_t top_edge_key(uint32_t from, uint32_t to)
{
    return from < to ? (((uint64_t)from << 26) | (uint64_t)to | kTopForward) : (((uint64_t)to << 26) | (uint64_t)from);
}
constexpr uint32_t top_key_va(uint64_t key) { return (uint32_t)(key >> 26) & 0x3FFFFFFu; }
constexpr uint32_t top_key_vb(uint64_t key) { return (uint32_t)key & 0x3FFFFFFu; }
constexpr bool top_same_edge(uint64_t a, uint64_t b) { return ((a ^ b) & (kTopForward - 1)) == 0; }
// The class of an edge from its exact (or saturated: the classes part below 3) counts.
constexpr uint32_t top_edge_kind(uint32_t n_fwd, uint32_t n_bwd)
{
    return n_fwd + n_bwd == 1 ? kTopBoundary : (n_fwd + n_bwd >= 3 ? kTopNonManifold : (n_fwd == 1 && n_bwd == 1 ? 0u : kTopMiswound));
}
constexpr uint32_t top_edge_uses(uint32_t n_fwd, uint32_t n_bwd) { return (n_fwd < 65535u ? n_fwd : 65535u) | ((n_bwd < 65535u ? n_bwd : 65535u) << 16); }

// The counts of a call that need no pointer: 0 = fine, else the text of the fault.
inline const char* topology_counts_fault(uint64_t n_verts, uint64_t n_tris)
{
    if (n_verts > kTopMaxVerts) return "n_verts must not exceed 2^26";
    if (n_tris >= (kTopMaxHalfEdges + 2) / 3) return "3 * n_tris must stay below 2^32";
    return nullptr;
}

}  // namespace hfpf
