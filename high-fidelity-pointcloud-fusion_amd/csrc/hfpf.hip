// csrc/hfpf.hip -- host side of libhfpf.so: handle, HBM pools, kernel orchestration, C ABI (include/hfpf.h).
//
// One HIP stream per handle; every entry point enqueues on it.  clean/extract are the only calls
// that read device counters back (they are synchronisation points in the reference too: clean holds
// grid_mtx_, node.cpp:305-321).  No CPU fallback exists: without a usable HIP device hfpf_create fails.
#include <hip/hip_runtime.h>

#include <cstring>  // rocprim's texture_cache_iterator.hpp uses memset without including it

#include <rocprim/rocprim.hpp>

#include <dlfcn.h>
#include <sched.h>
#include <sys/mman.h>

#if !defined(__HIP_DEVICE_COMPILE__)
#include <emmintrin.h>
#endif
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hfpf.h"
#include "host_plan.hpp"
#include "kernels.hpp"
#include "scratch_layout.hpp"

using namespace hfpf;

static_assert(sizeof(hfpf_row) == sizeof(Row), "hfpf_row layout");
static_assert(kSlotsPerBrick == (uint64_t)kBrickCells, "host_plan.hpp sizes the slot sort for these bricks");

namespace {

thread_local std::string g_create_error;  // last error of a call that has no handle (create, dist_unique_id)

// A lazily grown device buffer (scratch()).  It registers itself with its handle (hfpf_handle::bufs), which is how hfpf_destroy
// finds it: the handle is never copied or moved, so the address stays good.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    explicit DevBuf(std::vector<DevBuf*>& registry) { registry.push_back(this); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    friend void swap(DevBuf& a, DevBuf& b) { std::swap(a.p, b.p), std::swap(a.bytes, b.bytes); }  // the memory changes hands, the registrations stay
};

struct StageSlot {  // pose / frame-id staging for one in-flight integrate call: n poses (12 doubles each), then n frame ids -- ONE upload
    double* h_pose = nullptr;
    uint32_t* h_ids = nullptr;  // = h_pose + 12 * (frames of the call)
    double* d_pose = nullptr;
    uint32_t* d_ids = nullptr;
    uint32_t cap = 0;
    hipEvent_t done = nullptr;
    bool pending = false;
};

struct FrameSlot {  // host-frame staging: a pinned bounce buffer + one slot of the device ring (hfpf_handle::ring_d)
    void* h = nullptr;       // pinned bounce buffer (hfpf_integrate only; hfpf_integrate_pinned copies from the caller's memory)
    size_t cap_h = 0;
    hipEvent_t done = nullptr;    // main stream: the kernels that read the slot have finished
    hipEvent_t copied = nullptr;  // copy stream: the upload into the slot has finished
    bool pending = false;
};

// Helper threads for the bounce copy of hfpf_integrate (caller's pageable frame -> pinned staging): one core moves ~12 GB/s, the
// link takes 55, so the copy is split over the caller + the helpers.  The helpers spin for a fraction of a millisecond after a
// job (a stream of frames keeps them hot) and sleep on a condition variable otherwise.
// Copy with non-temporal stores (dst 16-byte aligned): the staging buffer is only read by the DMA engine afterwards, so the
// lines need not be fetched for ownership nor kept in the cache -- a third less memory traffic than memcpy below glibc's
// non-temporal threshold (which a 1-2 MB share of a frame does not reach).
#if !defined(__HIP_DEVICE_COMPILE__)
inline void stream_copy(char* dst, const char* src, size_t n)
{
    if (((uintptr_t)dst & 15u) != 0) {
        memcpy(dst, src, n);
        return;
    }
    size_t i = 0;
    for (; i + 64 <= n; i += 64) {
        const __m128i a = _mm_loadu_si128((const __m128i*)(src + i)), b = _mm_loadu_si128((const __m128i*)(src + i + 16));
        const __m128i c = _mm_loadu_si128((const __m128i*)(src + i + 32)), d = _mm_loadu_si128((const __m128i*)(src + i + 48));
        _mm_stream_si128((__m128i*)(dst + i), a);
        _mm_stream_si128((__m128i*)(dst + i + 16), b);
        _mm_stream_si128((__m128i*)(dst + i + 32), c);
        _mm_stream_si128((__m128i*)(dst + i + 48), d);
    }
    _mm_sfence();
    if (i < n) memcpy(dst + i, src + i, n - i);
}
#else
inline void stream_copy(char* dst, const char* src, size_t n) { memcpy(dst, src, n); }
#endif

class StagePool {
  public:
    explicit StagePool(int helpers)
    {
        for (int i = 0; i < helpers; i++) th_.emplace_back([this, i] { run(i + 1); });
    }
    ~StagePool()
    {
        stop_.store(true, std::memory_order_release);
        {
            std::lock_guard<std::mutex> lk(m_);
            cv_.notify_all();
        }
        for (auto& t : th_) t.join();
    }
    void copy(void* dst, const void* src, size_t bytes)
    {
        dst_ = (char*)dst, src_ = (const char*)src, bytes_ = bytes;
        remaining_.store((int)th_.size(), std::memory_order_relaxed);
        gen_.fetch_add(1, std::memory_order_release);
        if (sleepers_.load(std::memory_order_acquire) > 0) {
            std::lock_guard<std::mutex> lk(m_);
            cv_.notify_all();
        }
        part(0);
        while (remaining_.load(std::memory_order_acquire) != 0) __builtin_ia32_pause();
    }

  private:
    void part(int i) const
    {
        const size_t parts = th_.size() + 1;
        const size_t chunk = ((bytes_ + parts - 1) / parts + 4095) & ~(size_t)4095;
        const size_t lo = std::min(bytes_, chunk * (size_t)i), hi = std::min(bytes_, lo + chunk);
        if (hi > lo) stream_copy(dst_ + lo, src_ + lo, hi - lo);
    }
    void run(int i)
    {
        uint64_t seen = 0;
        for (;;) {
            uint64_t g;
            int spins = 0;
            while ((g = gen_.load(std::memory_order_acquire)) == seen && !stop_.load(std::memory_order_acquire)) {
                if (++spins < 20000) {
                    __builtin_ia32_pause();
                } else {
                    std::unique_lock<std::mutex> lk(m_);
                    sleepers_.fetch_add(1, std::memory_order_acq_rel);
                    cv_.wait(lk, [&] { return gen_.load(std::memory_order_acquire) != seen || stop_.load(std::memory_order_acquire); });
                    sleepers_.fetch_sub(1, std::memory_order_acq_rel);
                    spins = 0;
                }
            }
            if (stop_.load(std::memory_order_acquire)) return;
            seen = g;
            part(i);
            remaining_.fetch_sub(1, std::memory_order_acq_rel);
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_;
    std::atomic<uint64_t> gen_{0};
    std::atomic<int> remaining_{0}, sleepers_{0};
    std::atomic<bool> stop_{false};
    char* dst_ = nullptr;
    const char* src_ = nullptr;
    size_t bytes_ = 0;
};

constexpr int kStageSlots = 8;
constexpr size_t kXferChunk = 16u << 20;  // bytes per pinned chunk of extract's row download
constexpr int kFrameSlots = 8;  // uploads run ahead of the kernels by up to this many frames

// A validated hfpf_depth_image as the kernels take it (depth_spec below).  32-bit fields only: two specs are compared with memcmp
// (a batch of waiting host frames must share one).
struct DepthSpec {
    uint32_t width, height, depth_f32, depth_step, color_bpp, color_bgr, color_step;
    float cx, cy, sx, sy, unit;
    uint32_t color_off;  // host frame path: byte offset of the colour image in a ring slot (behind the depth image, 256-aligned)
    size_t depth_bytes() const { return (size_t)(height - 1) * depth_step + (size_t)width * (depth_f32 ? 4u : 2u); }
    size_t color_bytes() const { return color_bpp ? (size_t)(height - 1) * color_step + (size_t)width * color_bpp : 0; }
};
static_assert(sizeof(DepthSpec) == 13 * 4, "DepthSpec is compared bytewise");

DepthLayout depth_layout(const DepthSpec& d, const void* dev_color, uint64_t color_stride)
{
    return DepthLayout{d.color_bpp ? (const uint8_t*)dev_color : nullptr, color_stride, d.width, d.depth_step, d.color_step, d.depth_f32,
                       d.color_bpp, d.color_bgr, d.cx, d.cy, d.sx, d.sy, d.unit};
}

// What the environment overrides (HFPF_*), read once by read_knobs() at hfpf_create.  One exception: HFPF_TEST_SNAPSHOT_WINDOW is
// read by snap_stage_alloc at every call, because a test sets it on a live handle.
struct Knobs {
    int copy_streams = 2;            // HFPF_COPY_STREAMS=1..4: streams the host-frame uploads alternate over
    bool update_cells = true;        // k_update_cells (cell-sorted form); HFPF_UPDATE_FORM=points: k_update (per-point form), A/B and tests
    int host_batch = 4;              // HFPF_HOST_BATCH (1 = every frame launches on its own)
    int upd_shape_forced = -1;       // HFPF_UPD_SHAPE=0|1
    bool trace_shape = false;        // HFPF_TRACE_SHAPE=1: one stderr line per pick_update_shape() window
    bool bin_spare = true;           // HFPF_BIN_SPARE=0: no bin regions for bricks the launch discovers
    bool stream_replay = true;       // HFPF_STREAM_REPLAY=0: every replay walks the chains
    float bin_slack = 2.0f;          // planned capacity of a bin region = the brick's demand in the previous launch x this (HFPF_BIN_SLACK)
    bool clean_small_nowait = true;  // small clean passes run without a mid-pass read-back (HFPF_CLEAN_NOWAIT=0 restores it)
    bool clean_overlap = true;       // HFPF_CLEAN_OVERLAP=0: k_buffer stays behind the update kernel and a clean pass runs on the engine's stream alone
    bool early_replay = true;        // HFPF_EARLY_REPLAY=0: the buffer replay of an overlapped small pass stays behind the dependant-table update (k_replay)
    bool trace_clean = false;        // HFPF_TRACE_CLEAN=1: one stderr line per clean pass that launches kernels: which stream its front half took, which replay; a second one ("clean forms"): which size-gated forms
    float test_bin_scale = 1.f;      // tests only (HFPF_TEST_BIN_SCALE): shrinks the planned bin regions so that they overflow into the direct forms
    bool test_table_skip = false;    // tests only (HFPF_TEST_TABLE_SKIP=1): Tables::test_table_skip
    CleanLimits limits;              // tests only (HFPF_TEST_STREAM_MIN, _SORT_MIN, _REG_LARGE_MIN, _GATE4_MIN, each >= 1): the sizes at which a clean pass changes its form
    bool mailbox = true;             // HFPF_MAILBOX=0: counter read-backs by blit copies + synchronize
    int test_dev_tile = kDevTileDefault;  // tests only (HFPF_TEST_DEV_TILE=8..256): triangles per LDS tile of k_dev_rows
    int cons_chunk = 0;              // HFPF_CONSISTENCY_CHUNK=1..64: frames per chunk of k_consistency (0: plan_consistency decides); tests
    int stage_threads = 0;           // HFPF_STAGE_THREADS: helpers of the StagePool (default half the process's cores - 1, at most 7; 0 = none)
};

// The fusion session: the host mirrors that must follow the device tables.  The initialisers are the values of a fresh or cleared
// handle: reset_state() assigns Session{} and nothing else.  A NEW FIELD GOES HERE, with its note: does a snapshot carry it
// (session_to_header / header_to_session), and if not, what re-creates it after a restore.
struct Session {
    bool dirty = false;                     // snapshot: carried
    uint64_t n_linked[kLogRegions] = {0};   // per log region: entries already chained.  snapshot: carried
    uint64_t gate_done = 0;                 // occ_list entries already examined by a gate pass.  snapshot: carried
    bool pend_valid = false;                // pend_a holds C_PEND cells that a gate pass examined and left without a normal.  snapshot: carried
    uint64_t direct_linked = 0;             // points buffered by k_integrate's direct form (C_BUFFERED) that k_link_log has already chained.  snapshot: carried
    bool normals_possible = false;          // a clean pass has run since the last clear (the host mirror of C_NORMALS may lag behind a no-wait pass).  snapshot: carried
    uint32_t next_frame_id = 0;             // snapshot: carried
    // A capacity / HIP / collective error in the middle of a clean pass leaves the tables half updated: the handle then refuses
    // further work (HFPF_ERR_STATE) until hfpf_clear, instead of silently losing candidates on a retry.
    bool poisoned = false;                  // snapshot: not carried (a failed handle refuses hfpf_snapshot; a restore begins with a clear)
    std::string poison_msg;
    // plan of the binned dependant update.  snapshot: not carried; the next integrate call starts without a plan and records one
    bool bin_have_hist = false;             // bin_fill holds the demand of the previous launch
    bool bin_from_probe = false;            // ... and that launch was the dry run of a session's first frames
    double bin_prev_points = 0;             // points presented by that launch (to scale the plan)
    uint64_t n_bricks_known = 0;            // bricks allocated at the last counter read-back.  snapshot: not carried; the counter read-back of restore
    uint64_t n_bricks_before = 0;           // ... and at the read-back before the count last changed.  snapshot: not carried; restore sets it to n_bricks_known
    // pick_update_shape()'s window.  snapshot: not carried, and nothing re-creates it: the first window after a restore covers the
    // source session's totals
    unsigned long long upd_miss_seen = 0, upd_member_seen = 0;
    unsigned long long pub_seq = 0;         // sequence number of a publish enqueued behind the last integrate call and still current (0: none).  snapshot: not carried; 0 makes the next read-back publish for itself
    // ... and of that call's EARLY publish (second mailbox slot): the counters between k_buffer and the update kernel, with ev_ready
    // recorded behind it; alive only while pub_seq is (0: none).  What lets a clean pass start beside the update kernel (clean_locked).
    // snapshot: not carried; 0 is the plain path
    unsigned long long early_seq = 0;
    // A clean pass that began from the early publish leaves the call's final one unread: pick_update_shape takes the update kernel's
    // words from it (window_from_final) unless a full read-back came first.  snapshot: not carried (0: nothing to take)
    unsigned long long win_seq = 0;
    // Host frames uploaded, not yet launched: slots [pend_first, pend_first + pend_n); everything but pend_n is dead while pend_n == 0.
    // snapshot: not carried (hfpf_snapshot launches them first)
    uint32_t pend_n = 0, pend_first = 0;
    uint32_t pend_pts = 0;
    uint32_t pend_lay[5] = {0, 0, 0, 0, 0};  // point_step, off_x, off_y, off_z, off_rgb of the pending frames
    bool pend_depth = false;                  // ... or: the pending frames are depth images of this spec
    DepthSpec pend_ds{};
    double pend_pose[kFrameSlots * 12] = {0};
    // exchange cursors (multi-GPU, hfpf_epoch_*).  snapshot: not carried; handles that exchange refuse snapshot and restore
    uint64_t occ_exported = 0;              // occ_list entries already exchanged
    uint64_t frames_exported = 0, frames_seen = 0;  // frame_list entries already exchanged / as of the last export
    // |H|, the HIDDEN voxels of hfpf_hide_* (hfpf_handle::hidden_words holds the bits; Tables::hidden points at them while this is not 0).
    // snapshot: carried, as the HIDDEN section (present when this is not 0); restore counts the section's bits
    uint64_t n_hidden = 0;
};

// Kernel timing (hfpf_get_kernel_time): one row per public kernel id.  Ids 0, 1, 5, 6, 7 bracket work with an event pair (Timed
// below) that waits in `pending` until resolve_timing adds it to the sums; ids 2..4 use the rows for their sums only (their events
// are hfpf_handle::ev_detail).
constexpr int kTimeIntegrate = 0, kTimeClean = 1, kTimeDetail = 2, kTimeRaycast = 5, kTimeComponents = 6, kTimeCompare = 7, kTimedIds = 8;
struct TimedId {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double ms = 0;
    uint64_t n = 0;
};

}  // namespace

// Four groups: configuration and knobs, the session, resources, kernel timing.
struct hfpf_handle {
    std::mutex mtx;
    std::string err;

    // ---- configuration: what the caller asked for (setup_params, alloc_tables) and what the environment overrode ----
    hfpf_config cfg;
    GridParams g;
    Knobs knobs;
    bool binned = false;  // two-pass (binned) dependant update (default; HFPF_FLAG_DIRECT_UPDATE switches it off)
    int integrate_grid = 1536;
    int compute_units = 1;  // of the device (plan_consistency)
    size_t dir_entries = 0;
    uint64_t n_slots = 0;
    uint64_t max_touched = 0;

    // ---- the session (reset_state) ... ----
    Session ss;
    // ... and what an hfpf_clear leaves alone
    uint64_t frames_integrated = 0;  // hfpf_get_counters reports it per handle; a restore overwrites it.  Kept to preserve behaviour
    uint64_t clean_passes = 0;       // the same
    uint32_t launch_seq = 0;         // integrate launches so far (rotates the log append regions).  Kept to preserve behaviour
    bool upd_wide = false;           // the 352-slot record table overflowed: k_update_cells takes the 512-slot shape.  Stays: the next session on this handle fuses the same kind of scene
    bool epoch_used = false;         // epoch records or statistic words have left or entered this handle: no snapshot (include/hfpf.h).  Stays: include/hfpf.h says "has exported or imported", ever
    unsigned long long mbox_seq = 0; // never repeats while the mailbox lives: the flag word still holds the last published number
    int stage_next = 0, fslot_next = 0;  // cursors of the stage[] and fslot[] rings: the slots and their events outlive a session

    // ---- resources: streams, pools, scratch, pinned staging ----
    Tables t;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;  // host-frame uploads, overlapped with the kernels of earlier frames
    // ... of ring slots 1, 2, ... modulo knobs.copy_streams: uploads in flight side by side keep the link busy across the gap between
    // two copies of one stream
    hipStream_t copy_more[3] = {nullptr, nullptr, nullptr};
    std::vector<void*> allocs;
    uint64_t device_bytes = 0;
    uint64_t* hidden_words = nullptr;  // the HIDDEN bits, (max_bricks + 1) * 8 words, allocated by the first call that hides a row (hide_words_locked); all zero while Session::n_hidden is 0
    unsigned long long* h_ctr = nullptr;      // pinned mirror of the counters
    unsigned long long* h_log_ctr = nullptr;  // pinned mirror of the region counters
    unsigned long long* mbox = nullptr;       // coherent pinned mailbox k_publish_counters writes (null with HFPF_MAILBOX=0): two slots of kMboxSlotWords
    // The front half of a clean pass (sentinels, gate, candidate sort, k_normal, k_register) runs here beside the update kernel of
    // the integrate call before it: it waits for ev_ready, the engine's stream waits for ev_front behind k_register (clean_locked)
    // and, at the end of the pass, for ev_replay behind the registration-fed replay that follows k_register there
    hipStream_t front_stream = nullptr;
    hipEvent_t ev_ready = nullptr, ev_front = nullptr, ev_replay = nullptr;
    std::vector<DevBuf*> bufs;  // every DevBuf below, in declaration order (DevBuf's constructor): what hfpf_destroy frees
    DevBuf pend_a{bufs}, pend_b{bufs};  // the gate's pending-cell lists (Session::pend_valid)
    StageSlot stage[kStageSlots];
    FrameSlot fslot[kFrameSlots];
    // Device side of the host-frame path: ONE allocation of kFrameSlots slots, ring_cap bytes apart, so that consecutive slots
    // form a batch k_integrate can take in one launch (frame_stride = ring_cap).  Frames that arrive while the engine's stream
    // is still busy with earlier ones are uploaded at once but handed to the kernels together (up to host_batch of them): one
    // bin plan, one k_integrate, one pass of the per-brick kernels for the lot instead of one each.  A frame that finds the
    // stream idle is launched immediately, so a sensor slower than the engine sees no added latency.
    void* ring_d = nullptr;
    size_t ring_cap = 0;
    hipEvent_t busy_ev = nullptr;         // recorded behind the last launch of the host-frame path
    bool busy_pending = false;
    void* xfer_pin[2] = {nullptr, nullptr};  // pinned staging of extract's row download (two chunks in flight)
    hipEvent_t xfer_ev[2] = {nullptr, nullptr};
    StagePool* stage_pool = nullptr;  // created by the first large bounce copy (knobs.stage_threads helpers)
    DevBuf sort_tmp{bufs}, keys_a{bufs}, keys_b{bufs}, vals_a{bufs}, vals_b{bufs}, rows_dev{bufs};
    DevBuf probe_a{bufs}, probe_b{bufs}, probe_c{bufs}, probe_d{bufs}, probe_e{bufs}, probe_f{bufs};
    DevBuf result_out{bufs};  // the host forms of the read-outs that return arrays: the device arrays of one call (result_alloc)
    DevBuf zbuf{bufs}, render_pose{bufs}, render_out{bufs};  // hfpf_render*: z-buffers of one chunk of views, the views' poses, hfpf_render's device planes
    DevBuf track_in{bufs};                                   // hfpf_track*: a host frame's device copy
    DevBuf icp_acc{bufs};                                    // refine_pose (hfpf_track*, hfpf_align_mesh*): the int64 sums of one iteration
    DevBuf query_in{bufs}, query_out{bufs};                  // hfpf_query*: a host cloud chunk or depth image, one chunk's hits and rows
    // hfpf_extract_mesh*: cube and corner keys, per corner s / record / marks / vertex counts and bases, per cube triangle counts and
    // bases, a unique count
    DevBuf mesh_cube{bufs}, mesh_corner{bufs}, mesh_kdata{bufs}, mesh_cdata{bufs}, mesh_ctr{bufs};
    // hfpf_extract_components*: record -> row, the per-row words (parent, root, component, flags and bases), the component records and
    // their keep flags, ranks and bases
    DevBuf comp_index{bufs}, comp_rows{bufs}, comp_recs{bufs};
    // hfpf_compare_mesh*: the host form's mesh, the transformed vertices and triangle records, the bricks' keys / ranges / counters /
    // summary, the (brick, triangle) pairs (unsorted and sorted)
    DevBuf dev_mesh{bufs}, dev_tri{bufs}, dev_bins{bufs}, dev_pairs{bufs};
    DevBuf align_dev{bufs};  // hfpf_align_mesh*: one iteration's deviation records
    DevBuf cov_bins{bufs};   // hfpf_cover_mesh*: the summary, the 64-bit sample total, the triangles' sample counts and their offsets
    // hfpf_plan_views*: the samples' target marks; their scan; the targets (point + triangle, weight); the views' bitsets and the
    // remaining set; the cover records, the scores, the gains and the call's state words
    DevBuf plan_mark{bufs}, plan_scan{bufs}, plan_targets{bufs}, plan_bits{bufs}, plan_ctr{bufs};
    // hfpf_section_mesh*: the counters, the planes, the plane records and the per-plane counts and bases; the segment and point keys
    // (unsorted, sorted, unique) and the sort's values; per point its f64 coordinates, forest, root, flags, scan and degrees.  The
    // transformed vertices lie in dev_tri, a host mesh in dev_mesh
    DevBuf sec_ctr{bufs}, sec_keys{bufs}, sec_data{bufs};
    // hfpf_mesh_topology*: the counters and the per-vertex words (marks, root flags and their scan, degrees); the two forests over the
    // vertices and their roots; the half-edge keys and values (unsorted, sorted) and the per-half-edge words (counts, listed flags and
    // their scan).  The transformed vertices lie in dev_tri, a host mesh in dev_mesh
    DevBuf top_verts{bufs}, top_forest{bufs}, top_keys{bufs};
    // hfpf_depth_consistency*: one upload's frames of the host form, the poses, the records / summary / keep marks and their scan
    DevBuf cons_in{bufs}, cons_pose{bufs}, cons_recs{bufs};
    DevBuf hide_in{bufs}, hide_mark{bufs};  // hfpf_hide_*: one upload's entries of the host form (voxels, then selector words); the mark words and the call's counters
    DevBuf ray_in{bufs}, ray_out{bufs}, ray_map{bufs};  // hfpf_raycast*: a host chunk's rays, a chunk's (or band's) hits, the empty-space maps
    DevBuf snap_stage{bufs}, snap_err{bufs};            // hfpf_snapshot / hfpf_restore: the staging buffer (or one window of it), the range check's error word
    uint64_t bin_pool = 0;           // entries in bin_pt
    DevBuf bin_pt_buf{bufs}, bin_rgb_buf{bufs}, bin_sums{bufs};
    DevBuf ovf_pt_buf{bufs}, ovf_aux_buf{bufs};  // overflow list of one integrate launch (points that found no room in a bin)
    // multi-GPU: RCCL is resolved at run time so a single-GPU user needs no librccl
    bool dist_on = false;
    int rank = 0, world = 1;
    void* rccl_lib = nullptr;
    void* comm = nullptr;  // ncclComm_t
    uint64_t ex_cap_records = 0;  // records the exchange buffers hold per rank; kept EQUAL on every rank (same initial value, same growth rule)
    DevBuf ex_send{bufs}, ex_recv{bufs}, ex_counts{bufs}, stats_total{bufs};
    unsigned long long* h_counts = nullptr;  // pinned, world entries

    // ---- kernel timing ----
    bool timing = false;
    bool timing_detail = false;  // hfpf_kernel_timing(h, 2): also one event pair per kernel of an integrate call (ids 2..4)
    std::vector<hipEvent_t> ev_detail;  // 4 events per call: before k_integrate, after it, after k_update*, after k_buffer (or: after k_buffer, after k_update*)
    std::vector<uint8_t> ev_detail_ran;  // per call: bit k = kernel id 2 + k was launched; bit 3 = k_buffer ran ahead of the update kernel
    // One pair per: integrate launch (id 0), clean pass (1), k_raycast / k_raycast_view launch (5), hfpf_extract_components* call (6),
    // hfpf_compare_mesh* call (7)
    TimedId timed[kTimedIds];
    std::vector<hipEvent_t> ev_free;  // the pool the events come from and go back to
};

namespace {

int fail(hfpf_handle* h, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    else g_create_error = buf;
    return code;
}

int check_usable(hfpf_handle* h)
{
    if (!h->ss.poisoned) return HFPF_OK;
    return fail(h, HFPF_ERR_STATE, "handle failed earlier (%s); hfpf_clear resets it", h->ss.poison_msg.c_str());
}
int poison_on_error(hfpf_handle* h, int rc)
{
    if ((rc == HFPF_ERR_CAPACITY || rc == HFPF_ERR_HIP || rc == HFPF_ERR_DIST) && !h->ss.poisoned) {
        h->ss.poisoned = true;
        h->ss.poison_msg = h->err;
    }
    return rc;
}

#define HIPCHK(h, call)                                                                                        \
    do {                                                                                                       \
        hipError_t e_ = (call);                                                                                \
        if (e_ != hipSuccess) return fail(h, HFPF_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

template <typename T>
int dev_alloc(hfpf_handle* h, T** out, uint64_t count, int memset_byte = 0, bool do_memset = true)
{
    void* p = nullptr;
    const size_t bytes = std::max<uint64_t>(count, 1) * sizeof(T);
    HIPCHK(h, hipMalloc(&p, bytes));
    h->allocs.push_back(p);
    h->device_bytes += bytes;
    if (do_memset) HIPCHK(h, hipMemsetAsync(p, memset_byte, bytes, h->stream));
    *out = (T*)p;
    return HFPF_OK;
}

hipError_t sync_copy_streams(hfpf_handle* h)
{
    hipError_t e = hipStreamSynchronize(h->copy_stream);
    for (hipStream_t cs : h->copy_more)
        if (cs && e == hipSuccess) e = hipStreamSynchronize(cs);
    return e;
}

int scratch(hfpf_handle* h, DevBuf& b, size_t bytes)
{
    if (b.bytes >= bytes && b.p) return HFPF_OK;
    if (b.p) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipFree(b.p));
        h->device_bytes -= b.bytes;
        b.p = nullptr;
        b.bytes = 0;
    }
    const size_t want = std::max<size_t>(bytes + bytes / 4, 4096);
    HIPCHK(h, hipMalloc(&b.p, want));
    b.bytes = want;
    h->device_bytes += want;
    return HFPF_OK;
}

template <typename T>  // one array of `count` T in b: the typed pointer, taken once, after the allocation
int scratch_n(hfpf_handle* h, DevBuf& b, uint64_t count, T** out)
{
    const int rc = scratch(h, b, count * sizeof(T));
    *out = rc ? nullptr : static_cast<T*>(b.p);
    return rc;
}

// Several arrays in b (scratch_layout.hpp): one allocation of the layout's bytes, then every declared pointer is set.
int scratch(hfpf_handle* h, DevBuf& b, const ScratchLayout& lay)
{
    if (!lay.fits()) return fail(h, HFPF_ERR_STATE, "a scratch layout declares too many arrays (internal)");
    if (int rc = scratch(h, b, (size_t)lay.bytes())) return rc;
    lay.place(b.p);
    return HFPF_OK;
}

inline unsigned blocks_for(uint64_t n, unsigned bs) { return (unsigned)std::max<uint64_t>(1, (n + bs - 1) / bs); }

__global__ void k_set_ctr(unsigned long long* ctr, int idx, unsigned long long v) { ctr[idx] = v; }
// up to three counters in one launch (the clean pass resets them in groups; a launch costs ~5 us even for one thread)
__global__ void k_set_ctr3(unsigned long long* ctr, int i0, unsigned long long v0, int i1, unsigned long long v1, int i2, unsigned long long v2)
{
    ctr[i0] = v0;
    ctr[i1] = v1;
    if (i2 >= 0) ctr[i2] = v2;
}

// Counter read-back through a mailbox in coherent pinned host memory: one small kernel copies the counters (and the four
// used words of every region-counter line) over the link and then publishes a sequence number with system-scope release; the
// host spins on that number.  Against two blit copies + hipStreamSynchronize this saves ~20 us per read-back (the interrupt
// and wake-up of the synchronize), and a clean pass needs two of them with the GPU idle meanwhile.  Stream order makes the
// arrival of the number equivalent to a synchronize for everything enqueued before it.
constexpr int kMboxLogWords = 5;  // words 0..4 of each 16-word region-counter line are in use
constexpr int kMboxWords = C_COUNT + kLogRegions * kMboxLogWords;  // + the sequence number in its own 64-byte line
constexpr int kMboxSlotWords = (kMboxWords + 8 + 7) & ~7;  // a slot, whole 64-byte lines; slot 0: every read-back and the publish at the end of an integrate call, slot 1: the early publish
__global__ __launch_bounds__(256) void k_publish_counters(const unsigned long long* __restrict__ ctr, const unsigned long long* __restrict__ log_ctr,
                                                          unsigned long long* mbox, unsigned long long seq)
{
    const unsigned i = threadIdx.x;
    if (i < (unsigned)C_COUNT) mbox[i] = ctr[i];
    for (unsigned w = i; w < (unsigned)(kLogRegions * kMboxLogWords); w += blockDim.x) mbox[C_COUNT + w] = log_ctr[(w / kMboxLogWords) * 16 + (w % kMboxLogWords)];
    __threadfence_system();
    __syncthreads();
    if (i == 0) __hip_atomic_store(&mbox[kMboxWords + 7], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The host's side of a publish: spins until `seq` has arrived in the slot at `box`.
int await_mailbox(hfpf_handle* h, const unsigned long long* box, unsigned long long seq)
{
    const unsigned long long* flag = box + kMboxWords + 7;
    for (uint64_t spins = 1;; spins++) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) break;
        __builtin_ia32_pause();
        if ((spins & 0xFFFF) == 0) {  // every ~1 ms: a failed stream would never publish
            const hipError_t q = hipStreamQuery(h->stream);
            if (q != hipSuccess && q != hipErrorNotReady) HIPCHK(h, q);
            if (q == hipSuccess && __atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq)
                return fail(h, HFPF_ERR_HIP, "counter mailbox: the stream drained without publishing sequence %llu", seq);
        }
    }
    return HFPF_OK;
}

// early: the read-back at the head of a clean pass takes the EARLY publish of the pending integrate call (Session::early_seq;
// the caller has checked that there is one) and leaves the final one to pick_update_shape.
int read_counters(hfpf_handle* h, bool early = false)
{
    if (h->mbox) {
        // An integrate call ends with a publish of its own (nothing has touched the counters since): the snapshot is already on
        // its way, so the host only waits -- no launch of its own behind a stream that has just drained.
        unsigned long long seq = early ? h->ss.early_seq : h->ss.pub_seq;
        const unsigned long long* box = h->mbox + (early ? kMboxSlotWords : 0);
        h->ss.win_seq = early ? h->ss.pub_seq : 0;
        h->ss.pub_seq = 0;
        h->ss.early_seq = 0;
        if (seq == 0) {
            seq = ++h->mbox_seq;
            k_publish_counters<<<1, 256, 0, h->stream>>>(h->t.ctr, h->t.log_ctr, h->mbox, seq);
            HIPCHK(h, hipGetLastError());
        }
        if (int rc = await_mailbox(h, box, seq)) return rc;
        memcpy(h->h_ctr, box, C_COUNT * sizeof(unsigned long long));
        for (int r = 0; r < kLogRegions; r++)
            for (int w = 0; w < kMboxLogWords; w++) h->h_log_ctr[r * 16 + w] = box[C_COUNT + r * kMboxLogWords + w];
    } else {
        HIPCHK(h, hipMemcpyAsync(h->h_ctr, h->t.ctr, C_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->h_log_ctr, h->t.log_ctr, kLogRegions * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    unsigned long long total = 0;
    for (int r = 0; r < kLogRegions; r++) total += std::min<unsigned long long>(h->h_log_ctr[r * 16], h->t.log_region_cap);
    h->h_ctr[C_LOG] = total;
    unsigned long long replayed = 0;  // striped diagnostic counter of k_replay (word 1 of every log_ctr line)
    for (int r = 0; r < kLogRegions; r++) replayed += h->h_log_ctr[r * 16 + 1];
    h->h_ctr[C_REPLAY_MEMBER] = replayed;
    unsigned long long upd_tested = 0, upd_member = 0;  // k_update's striped pair counters (words 2, 3); k_integrate's direct path adds to ctr[]
    for (int r = 0; r < kLogRegions; r++) {
        upd_tested += h->h_log_ctr[r * 16 + 2];
        upd_member += h->h_log_ctr[r * 16 + 3];
    }
    h->h_ctr[C_DEP_TESTED] += upd_tested;
    h->h_ctr[C_DEP_MEMBER] += upd_member;
    unsigned long long single = 0;  // touched cells of the last dependant-table update that lie in single-run bricks (word 4)
    for (int r = 0; r < kLogRegions; r++) single += h->h_log_ctr[r * 16 + 4];
    h->h_ctr[C_TOUCHED_SINGLE] = single;
    {
        const uint64_t nbk = std::min<uint64_t>(h->h_ctr[C_BRICKS], h->t.max_bricks);
        if (nbk != h->ss.n_bricks_known) h->ss.n_bricks_before = h->ss.n_bricks_known;  // how fast the session discovers bricks (spare bin regions)
        h->ss.n_bricks_known = nbk;
    }
    return HFPF_OK;
}

int check_device_errors(hfpf_handle* h)
{
    const unsigned long long e = h->h_ctr[C_ERR];
    if (!e) return HFPF_OK;
    std::string what;
    if (e & E_BRICKS) what += " brick pool (max_bricks)";
    if (e & E_LOG) what += " point log (max_log_points)";
    if (e & E_OCC) what += " occupied list (max_normals*4)";
    if (e & E_NORMALS) what += " normal records (max_normals)";
    if (e & E_REG) what += " registrations (max_normals*7)";
    if (e & E_DEP) what += " dependant table";
    if (e & E_SPIN) what += " brick-claim spin bound";
    if (e & E_DEPCNT) what += " more than 65535 dependants on one cell";
    if (e & E_FRAME) what += " frame id >= max_frames";
    if (e & E_OVF) what += " integrate overflow list";
    if (e & E_CHAIN) what += " point-log chain / run record out of range (internal)";
    return fail(h, HFPF_ERR_CAPACITY, "device pool overflow:%s", what.c_str());
}

// Power-of-two scale that keeps one contribution of magnitude < bound below 2^27 (stats.hpp).
float stat_scale_for(double bound) { return (float)std::ldexp(1.0, 26 - (int)std::floor(std::log2(bound))); }

// The only reader of the environment (but see Knobs): ranges, clamps and defaults of every HFPF_* variable.
Knobs read_knobs()
{
    Knobs k;
    if (const char* cs = getenv("HFPF_COPY_STREAMS")) k.copy_streams = std::max(1, std::min(atoi(cs), 4));
    const char* uf = getenv("HFPF_UPDATE_FORM");
    k.update_cells = !(uf && uf[0] == 'p');
    if (const char* hb = getenv("HFPF_HOST_BATCH")) k.host_batch = std::max(1, std::min(atoi(hb), kFrameSlots));
    if (const char* us = getenv("HFPF_UPD_SHAPE")) k.upd_shape_forced = std::max(0, std::min(atoi(us), 1));
    if (const char* tr = getenv("HFPF_TRACE_SHAPE")) k.trace_shape = tr[0] != '0';
    if (const char* sp = getenv("HFPF_BIN_SPARE")) k.bin_spare = sp[0] != '0';
    if (const char* sr = getenv("HFPF_STREAM_REPLAY")) k.stream_replay = sr[0] != '0';
    if (const char* bs = getenv("HFPF_BIN_SLACK")) k.bin_slack = std::max(1.0f, std::min(4.0f, (float)atof(bs)));
    if (const char* nw = getenv("HFPF_CLEAN_NOWAIT")) k.clean_small_nowait = nw[0] != '0';
    if (const char* co = getenv("HFPF_CLEAN_OVERLAP")) k.clean_overlap = co[0] != '0';
    if (const char* er = getenv("HFPF_EARLY_REPLAY")) k.early_replay = er[0] != '0';
    if (const char* tc = getenv("HFPF_TRACE_CLEAN")) k.trace_clean = tc[0] != '0';    if (const char* bs = getenv("HFPF_TEST_BIN_SCALE")) k.test_bin_scale = std::max(0.f, std::min(1.f, (float)atof(bs)));
    const char* ts = getenv("HFPF_TEST_TABLE_SKIP");
    k.test_table_skip = ts && ts[0] == '1';
    const auto limit = [](const char* name, uint64_t& v) {
        if (const char* e = getenv(name)) v = (uint64_t)std::max(1ll, atoll(e));
    };
    limit("HFPF_TEST_STREAM_MIN", k.limits.stream_min_single);
    limit("HFPF_TEST_SORT_MIN", k.limits.sort_min_walked);
    limit("HFPF_TEST_REG_LARGE_MIN", k.limits.reg_large_min);
    limit("HFPF_TEST_GATE4_MIN", k.limits.gate4_min);
    if (const char* dt = getenv("HFPF_TEST_DEV_TILE")) k.test_dev_tile = std::max(8, std::min(atoi(dt), kDevTileMax));
    if (const char* cc = getenv("HFPF_CONSISTENCY_CHUNK")) k.cons_chunk = std::max(1, std::min(atoi(cc), (int)kConsChunkFrames));
    const char* mb = getenv("HFPF_MAILBOX");
    k.mailbox = !mb || mb[0] != '0';
    int cores = (int)std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) cores = std::min(cores > 0 ? cores : 1 << 20, CPU_COUNT(&set));  // the process's share
    const char* st = getenv("HFPF_STAGE_THREADS");
    k.stage_threads = st ? std::max(0, std::min(atoi(st), 15)) : std::max(0, std::min(7, cores / 2 - 1));
    return k;
}

int setup_params(hfpf_handle* h)
{
    const hfpf_config& c = h->cfg;
    GridParams& g = h->g;
    if (!(c.resolution > 0.f)) return fail(h, HFPF_ERR_BAD_CONFIG, "resolution must be > 0");
    for (int a = 0; a < 3; a++)
        if (!(c.bbox[2 * a + 1] > c.bbox[2 * a])) return fail(h, HFPF_ERR_BAD_CONFIG, "bounding_box axis %d: max <= min", a);
    if (c.k != 2) return fail(h, HFPF_ERR_BAD_CONFIG, "k must be 2 (the reference probes exactly 125 neighbours, OccupancyGrid.hpp:334)");
    if (c.K < 0 || c.K > 16) return fail(h, HFPF_ERR_BAD_CONFIG, "K out of range [0,16]");
    if (!(c.cylinder_radius > 0) || !(c.ball_radius > 0)) return fail(h, HFPF_ERR_BAD_CONFIG, "radii must be > 0");
    g.res = (double)c.resolution;  // float -> double, grid.hpp:614-619
    g.inv_res = 1.0 / g.res;
    for (int a = 0; a < 3; a++) {
        g.min[a] = c.bbox[2 * a];
        g.max[a] = c.bbox[2 * a + 1];
        const double d = (g.max[a] - g.min[a]) / g.res;  // grid.hpp:623-625 (int truncation)
        if (!(d < 2097151.0)) return fail(h, HFPF_ERR_BAD_CONFIG, "axis %d: more than 2^21 cells", a);
        g.dim[a] = (int32_t)d;
        g.bdim[a] = (g.dim[a] + 1 + 7) / 8;  // storage is dim+1 cells, grid.hpp:626
    }
    {
        auto bits_for = [](int32_t dim) {  // bits that hold 0..dim (storage is dim+1 cells per axis, grid.hpp:626)
            uint32_t b = 1;
            while ((1ll << b) <= (long long)dim) b++;
            return b;
        };
        g.key_sy = bits_for(g.dim[2]);
        g.key_sx = g.key_sy + bits_for(g.dim[1]);
        g.key_bits = g.key_sx + bits_for(g.dim[0]);
    }
    g.zclip_min = c.z_clip_min;
    g.zclip_max = c.z_clip_max;
    {   // float neighbours of the double clip constants (geometry.hpp, GridParams::bb_lo): compares in f32 with identical decisions
        auto float_at_or_above = [](double m) {
            float f = (float)m;
            if ((double)f < m) f = nextafterf(f, INFINITY);
            return f;
        };
        auto float_at_or_below = [](double m) {
            float f = (float)m;
            if ((double)f > m) f = nextafterf(f, -INFINITY);
            return f;
        };
        for (int a = 0; a < 3; a++) {
            g.bb_hi[a] = float_at_or_above(g.max[a]);
            g.bb_lo[a] = float_at_or_below(g.min[a]);
        }
        g.zc_hi = float_at_or_above(g.zclip_max);
        g.zc_lo = float_at_or_below(g.zclip_min);
    }
    g.cyl_r = c.cylinder_radius;
    g.ball_r = (float)c.ball_radius;
    g.K = c.K;
    g.gate = c.gate;
    g.cov_shifted = (c.flags & HFPF_FLAG_PCL_SHIFTED_COV) ? 1 : 0;
    // s = 0.5 + t / (2 r) with t the point's offset along the normal from the cell centre: a point updates a voxel only from
    // a cell on that voxel's line, so |t| <= K*res + sqrt(3)*res
    const double Bs = 0.5 + ((double)c.K + 2.0) * g.res / (2.0 * c.ball_radius);
    if (!(Bs < 1.0e6)) return fail(h, HFPF_ERR_BAD_CONFIG, "ball_radius too small for this resolution and K");
    const double Bm = HFPF_CENTERED_MOMENTS ? Bs - 0.5 : Bs;  // bound of the accumulated variable (u = s - 0.5 or s, stats.hpp)
    g.fs_scale = stat_scale_for(Bm);
    g.fss_scale = stat_scale_for(Bm * Bm);
    g.fd_scale = stat_scale_for(g.cyl_r);
    g.fdd_scale = stat_scale_for(g.cyl_r * g.cyl_r);
    {   // largest f32 u with (double)sqrtf(u) < cyl_r (sqrtf is correctly rounded on the host: IEEE 754), by bisection on the bits
        uint32_t lo_b = 0, hi_b = 0x7F800000u;  // invariant: f(lo) passes, f(hi) fails (sqrt(+inf) = inf)
        while (hi_b - lo_b > 1) {
            const uint32_t mid = lo_b + (hi_b - lo_b) / 2;
            float u;
            memcpy(&u, &mid, 4);
            if ((double)sqrtf(u) < g.cyl_r) lo_b = mid;
            else hi_b = mid;
        }
        memcpy(&g.d2_max, &lo_b, 4);
    }
    const double dir_entries = (double)g.bdim[0] * (double)g.bdim[1] * (double)g.bdim[2];
    if (dir_entries > 4.0e9) return fail(h, HFPF_ERR_BAD_CONFIG, "brick directory too large (%.3g entries)", dir_entries);
    h->dir_entries = (size_t)dir_entries;
    return HFPF_OK;
}

// bricks_used / normals_used: how far the session got into the brick pool and the record table (hfpf_clear knows; everything at
// create).  Per-cell and per-brick arrays are indexed by brick id, records by record id, and both are handed out in sequence, so a
// reset only has to cover the prefix the session used: the bench's handle is sized for 300,000 bricks and uses 22,000 -- 7 GB of
// resets become 0.6 GB.
int reset_state(hfpf_handle* h, uint64_t bricks_used = ~0ull, uint64_t normals_used = ~0ull)
{
    Tables& t = h->t;
    hipStream_t s = h->stream;
    const uint64_t nb = std::min<uint64_t>(bricks_used, t.max_bricks);                     // ids 1..nb (+ the unused id 0)
    const uint64_t nsl = std::min<uint64_t>(h->n_slots, (nb + 1) * (uint64_t)kBrickCells);  // their cells
    const uint64_t nn = std::min<uint64_t>(normals_used, t.max_normals);
    // (a clean pass that failed on the host half-way through its front half has not joined front_stream to the engine's stream)
    if (h->front_stream) HIPCHK(h, hipStreamSynchronize(h->front_stream));
    HIPCHK(h, hipMemsetAsync(t.dir, 0, h->dir_entries * 4, s));
    HIPCHK(h, hipMemsetAsync(t.info, 0, nsl * 8, s));
    HIPCHK(h, hipMemsetAsync(t.first_frame, 0xFF, nsl * 4, s));
    HIPCHK(h, hipMemsetAsync(t.buf_head, 0, nsl * 4 * kChains, s));
    HIPCHK(h, hipMemsetAsync(t.stat_id, 0, nsl * 4, s));
    HIPCHK(h, hipMemsetAsync(t.pre_dep, 0, nsl * 4, s));
    HIPCHK(h, hipMemsetAsync(t.dep_tmp, 0, nsl * 4, s));
    HIPCHK(h, hipMemsetAsync(t.occ_mask, 0, (nb + 1) * 8 * 8, s));
    HIPCHK(h, hipMemsetAsync(t.stats, 0, (nn + 1) * kStatWords * 8, s));
    HIPCHK(h, hipMemsetAsync(t.nd_mask, 0, (nb + 1) * 8 * 2 * 8, s));
    if (h->hidden_words) HIPCHK(h, hipMemsetAsync(h->hidden_words, 0, (nb + 1) * 8 * 8, s));
    t.hidden = nullptr;  // H is empty (Session::n_hidden)
    HIPCHK(h, hipMemsetAsync(t.ctr, 0, C_COUNT * 8, s));
    HIPCHK(h, hipMemsetAsync(t.log_ctr, 0, kLogRegions * 16 * 8, s));
    HIPCHK(h, hipMemsetAsync(t.bin_fill, 0, 2 * (t.max_bricks + 2) * 4, s));
    HIPCHK(h, hipMemsetAsync(t.bin_off, 0, 2 * (t.max_bricks + 2) * 4, s));
    HIPCHK(h, hipMemsetAsync(t.bin_capb, 0, 2 * (t.max_bricks + 2) * 4, s));
    HIPCHK(h, hipMemsetAsync(t.run_cnt, 0, (t.max_bricks + 2) * 4, s));
    if (h->h_ctr) memset(h->h_ctr, 0, C_COUNT * sizeof(unsigned long long));  // host mirror follows the device counters
    h->ss = Session{};
    return HFPF_OK;
}

int alloc_tables(hfpf_handle* h)
{
    hfpf_config& c = h->cfg;
    Tables& t = h->t;
    memset(&t, 0, sizeof t);
    if (c.max_bricks == 0) c.max_bricks = 131072;
    if (c.max_log_points == 0) c.max_log_points = 64ull << 20;
    if (c.max_normals == 0) c.max_normals = 8ull << 20;
    if (c.max_frames == 0) c.max_frames = 65536;
    if (c.max_bricks > 8388606ull) return fail(h, HFPF_ERR_BAD_CONFIG, "max_bricks must be < 2^23");
    c.max_log_points = std::max<uint64_t>(c.max_log_points, 64 * kLogRegions);
    if (c.max_log_points > 0x7FFFFFF0ull) return fail(h, HFPF_ERR_BAD_CONFIG, "max_log_points must be < 2^31 (bit 31 of a log link marks an unchained entry)");
    if (c.max_frames > (1ull << 23)) return fail(h, HFPF_ERR_BAD_CONFIG, "max_frames must be <= 2^23 (a parked point carries its frame id in 23 bits)");
    if (c.max_normals > 4294967294ull) return fail(h, HFPF_ERR_BAD_CONFIG, "max_normals must be < 2^32-1");
    t.max_bricks = c.max_bricks;
    t.max_log = c.max_log_points;
    t.max_normals = c.max_normals;
    t.max_occ = c.max_normals * 4;
    t.max_reg = c.max_normals * (2ull * (uint64_t)c.K + 1ull);
    t.max_dep = 2 * t.max_reg;  // room for the lists the incremental update relocates
    if (t.max_dep > 0xFFFFFFF0ull) return fail(h, HFPF_ERR_BAD_CONFIG, "max_normals too large: the dependant table must stay below 2^32 entries");
    t.max_frames = c.max_frames;
    h->n_slots = (t.max_bricks + 1) * (uint64_t)kBrickCells;
    h->max_touched = t.max_reg;
    int rc;
#define ALLOC(field, count, ...)                                         \
    if ((rc = dev_alloc(h, &t.field, (count), ##__VA_ARGS__)) != HFPF_OK) return rc;
    ALLOC(dir, h->dir_entries, 0, false);
    ALLOC(brick_lin, t.max_bricks + 1);
    ALLOC(info, h->n_slots, 0, false);
    ALLOC(first_frame, h->n_slots, 0, false);
    ALLOC(buf_head, h->n_slots * kChains, 0, false);
    ALLOC(stat_id, h->n_slots, 0, false);
    ALLOC(pre_dep, h->n_slots, 0, false);
    ALLOC(dep_tmp, h->n_slots, 0, false);
    ALLOC(occ_mask, (t.max_bricks + 1) * 8, 0, false);
    ALLOC(log_pt, t.max_log + 1, 0, false);
    if (c.flags & HFPF_FLAG_FUSE_COLOR) { ALLOC(log_rgb, t.max_log + 1, 0, false); }
    ALLOC(occ_list, t.max_occ, 0, false);
    ALLOC(nv_key, t.max_normals + 1, 0, false);
    ALLOC(nv_slot, t.max_normals + 1, 0, false);
    ALLOC(nv_c, 3 * (t.max_normals + 1), 0, false);
    ALLOC(nv_n, 3 * (t.max_normals + 1), 0, false);
    ALLOC(stats, (t.max_normals + 1) * kStatWords, 0, false);
    t.color = (c.flags & HFPF_FLAG_FUSE_COLOR) ? 1u : 0u;
    t.test_table_skip = h->knobs.test_table_skip ? 1u : 0u;
    ALLOC(nd_mask, (t.max_bricks + 1) * 8 * 2, 0, false);
    ALLOC(reg_occ, t.max_reg, 0, false);
    ALLOC(dep, t.max_dep + t.max_normals + 1, 0, false);  // dep[] and, behind it, the records' lines (one 32-byte entry each): one entry space
    t.nv_line = reinterpret_cast<float4*>(t.dep + t.max_dep);
    ALLOC(prereg_list, t.max_reg, 0, false);
    ALLOC(touched_list, h->max_touched, 0, false);
    ALLOC(run_start, t.max_bricks + 2, 0, false);
    ALLOC(run_len, t.max_bricks + 2, 0, false);
    ALLOC(run_cnt, t.max_bricks + 2);
    ALLOC(cand_key, t.max_occ, 0, false);
    ALLOC(frame_vp, 3 * t.max_frames);
    ALLOC(frame_list, t.max_frames, 0, false);
    ALLOC(ctr, C_COUNT);
    ALLOC(log_ctr, kLogRegions * 16);
    ALLOC(bin_fill, 2 * (t.max_bricks + 2));
    ALLOC(bin_off, 2 * (t.max_bricks + 2));
    ALLOC(bin_capb, 2 * (t.max_bricks + 2));
    h->binned = (c.flags & HFPF_FLAG_DIRECT_UPDATE) == 0;
#undef ALLOC
    t.log_region_cap = t.max_log / kLogRegions;
    t.ent_base = t.dep;
    t.ent_dep_first = 0;
    t.ent_nv_first = t.max_dep;  // (max_dep < 2^32 and max_normals < 2^32: far inside the 40-bit entry index of k_update_cells)
    return reset_state(h);
}

// (rocPRIM sorts fewer than a million keys by block sort + log2(n / 1024) merge launches -- nine launches, 57 us, for the 74 K candidate
// keys of a steady clean pass.  Forcing its radix path for small inputs, radix_sort_config<..., 8192>, was measured in round 4: a
// histogram, a scan and per 8-bit digit two buffer fills and one sweep, fifteen launches and ~100 us for the same keys: the merge path stays.)
// What does help: blocks of 4,096 sorted keys instead of 1,024 -- two merge launches less for those 74 K keys (clean passes 3.66 -> 3.57 ms
// per 1000-frame run; 8,192-key blocks: 3.64).
#ifndef HFPF_SORT_BLOCK_ITEMS
#define HFPF_SORT_BLOCK_ITEMS 4
#endif
using sort_config = rocprim::radix_sort_config<rocprim::default_config, rocprim::merge_sort_config<512, 1024, HFPF_SORT_BLOCK_ITEMS>, rocprim::default_config>;

// rocPRIM's two-call protocol on h->sort_tmp: fn(tmp, bytes) -> hipError_t is called with tmp = nullptr (it reports the bytes it
// needs), sort_tmp grows to that, and fn runs with the buffer and all of its bytes.
template <typename Fn>
int with_sort_tmp(hfpf_handle* h, Fn&& fn)
{
    size_t bytes = 0;
    HIPCHK(h, fn((void*)nullptr, bytes));
    if (int rc = scratch(h, h->sort_tmp, bytes)) return rc;
    bytes = h->sort_tmp.bytes;
    HIPCHK(h, fn(h->sort_tmp.p, bytes));
    return HFPF_OK;
}

// Cell keys: only the low GridParams::key_bits bits are significant (an all-ones sentinel still sorts behind every valid key:
// a valid cell has x < dim <= 2^bits_x - 1, so its key is never all ones).
// on: the stream the sort runs on (default: the engine's).  sort_tmp is the handle's one buffer: whoever sorts elsewhere sees to it
// that the engine's stream runs no sort, scan or unique meanwhile (clean_locked).
int sort_keys_u64(hfpf_handle* h, uint64_t* in, uint64_t* out, uint64_t n, unsigned bits = 0, hipStream_t on = nullptr)
{
    const unsigned kb = bits ? bits : h->g.key_bits;
    const hipStream_t st = on ? on : h->stream;
    return with_sort_tmp(h, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_keys<sort_config>(tmp, bytes, in, out, (size_t)n, 0, kb, st); });
}

int sort_keys_u32(hfpf_handle* h, uint32_t* in, uint32_t* out, uint64_t n, unsigned bits = 32)
{
    return with_sort_tmp(h, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_keys<sort_config>(tmp, bytes, in, out, (size_t)n, 0, bits, h->stream); });
}

int sort_pairs_u64(hfpf_handle* h, uint64_t* kin, uint64_t* kout, uint32_t* vin, uint32_t* vout, uint64_t n, unsigned bits = 0)
{
    const unsigned kb = bits ? bits : h->g.key_bits;
    return with_sort_tmp(h, [&](void* tmp, size_t& bytes) {
        return rocprim::radix_sort_pairs<sort_config>(tmp, bytes, kin, kout, vin, vout, (size_t)n, 0, kb, h->stream);
    });
}

// out[0..n] = the exclusive sum of the n + 1 words in[0..n] (in[n] = 0, so out[n] is the total, read back into *total).
int scan_counts_locked(hfpf_handle* h, const uint32_t* in, uint32_t* out, uint64_t n, uint64_t* total)
{
    if (int rc = with_sort_tmp(h, [&](void* tmp, size_t& bytes) {
            return rocprim::exclusive_scan(tmp, bytes, in, out, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), h->stream);
        }))
        return rc;
    uint32_t t = 0;
    HIPCHK(h, hipMemcpyAsync(&t, out + n, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *total = t;
    return HFPF_OK;
}

// out = the distinct keys of sorted[0, n) in order; their number lands in the first word of `count` (device) and in *n_out.
int unique_keys_locked(hfpf_handle* h, const uint64_t* sorted, uint64_t n, uint64_t* out, uint64_t* count, uint64_t* n_out)
{
    if (int rc = with_sort_tmp(h, [&](void* tmp, size_t& bytes) {
            return rocprim::unique(tmp, bytes, sorted, out, count, (size_t)n, rocprim::equal_to<uint64_t>(), h->stream);
        }))
        return rc;
    uint64_t cnt = 0;
    HIPCHK(h, hipMemcpyAsync(&cnt, count, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *n_out = cnt;
    return HFPF_OK;
}

int acquire_stage(hfpf_handle* h, uint32_t n_frames, StageSlot** out)
{
    StageSlot& s = h->stage[h->stage_next];
    h->stage_next = (h->stage_next + 1) % kStageSlots;
    if (s.pending) {
        HIPCHK(h, hipEventSynchronize(s.done));
        s.pending = false;
    }
    if (!s.done) HIPCHK(h, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    if (s.cap < n_frames) {
        if (s.h_pose) {
            HIPCHK(h, hipHostFree(s.h_pose));
            HIPCHK(h, hipFree(s.d_pose));
            s.h_pose = nullptr, s.d_pose = nullptr, s.cap = 0;
        }
        const uint32_t cap = std::max<uint32_t>(n_frames, 64);
        const size_t bytes = (size_t)cap * (12 * sizeof(double) + sizeof(uint32_t));
        HIPCHK(h, hipHostMalloc((void**)&s.h_pose, bytes, hipHostMallocDefault));
        HIPCHK(h, hipMalloc((void**)&s.d_pose, bytes));
        s.cap = cap;
    }
    s.h_ids = reinterpret_cast<uint32_t*>(s.h_pose + 12 * (size_t)n_frames);
    s.d_ids = reinterpret_cast<uint32_t*>(s.d_pose + 12 * (size_t)n_frames);
    *out = &s;
    return HFPF_OK;
}

// Which instantiation of k_update_cells a launch takes (kernels.hpp, UpdShape): 0 dense, 1 wide table.  HFPF_UPD_SHAPE=0|1 forces
// one.  Otherwise the dense shape, until the items that found no slot in its table exceed one in 500 member pairs (counted by the
// kernel, seen by the host at its counter read-backs -- every clean pass); then the wide table for the rest of the session.
// The streaming replay of a clean pass is the same kernel with the same table and counts its misses into the same word, so its
// members belong in the denominator too: a caller that reads the counters between a clean pass and the next integrate call
// (hfpf_get_counters, hfpf_get_kernel_time) makes a window that holds the replay alone -- a few hundred misses against no update
// member at all, which used to switch the session to the wide shape (bench.py's per-kernel pass did exactly that).
// The last clean pass began from the early publish of the integrate call before it (Session::win_seq): the words the update kernel
// of that call wrote -- the table misses and the member pairs -- are taken from the call's final publish here, so that the window
// below covers what it covered when the pass read that publish itself.  Nothing else of the final publish is used: it ran beside
// the front half of the pass, which moves other counters.  By now the update kernel has usually long finished; the engine's
// stream holds the back half of the pass and this call's k_integrate meanwhile.
int window_from_final(hfpf_handle* h)
{
    const unsigned long long seq = h->ss.win_seq;
    h->ss.win_seq = 0;
    if (!seq || !h->mbox) return HFPF_OK;
    if (int rc = await_mailbox(h, h->mbox, seq)) return rc;
    unsigned long long member = h->mbox[C_DEP_MEMBER], tested = h->mbox[C_DEP_TESTED];
    for (int r = 0; r < kLogRegions; r++) {
        tested += h->mbox[C_COUNT + r * kMboxLogWords + 2];
        member += h->mbox[C_COUNT + r * kMboxLogWords + 3];
    }
    h->h_ctr[C_DEP_TESTED] = tested;
    h->h_ctr[C_DEP_MEMBER] = member;
    h->h_ctr[C_TABLE_MISS] = h->mbox[C_TABLE_MISS];
    h->h_ctr[C_UPD_ROUNDS] = h->mbox[C_UPD_ROUNDS];
    return HFPF_OK;
}

int pick_update_shape(hfpf_handle* h)
{
    if (h->knobs.upd_shape_forced >= 0) return h->knobs.upd_shape_forced;
    const unsigned long long miss = h->h_ctr[C_TABLE_MISS], member = h->h_ctr[C_DEP_MEMBER] + h->h_ctr[C_REPLAY_MEMBER];
    if (h->knobs.trace_shape)
        fprintf(stderr, "hfpf: update shape window: %llu table misses, %llu members (%llu of them replayed so far), %s\n", miss - std::min(miss, h->ss.upd_miss_seen),
                member - std::min(member, h->ss.upd_member_seen), h->h_ctr[C_REPLAY_MEMBER], h->upd_wide ? "wide" : "dense");
    if (!h->upd_wide && update_shape_goes_wide(miss, member, h->ss.upd_miss_seen, h->ss.upd_member_seen)) h->upd_wide = true;
    h->ss.upd_miss_seen = miss;
    h->ss.upd_member_seen = member;
    return h->upd_wide ? 1 : 0;
}

// A cloud's record layout: x, y, z (and rgb: with_rgb) 4-byte aligned and inside point_step.  what = the entry point named in the
// message.  The base address and the frame stride are the caller's to check.
int check_cloud_layout(hfpf_handle* h, const char* what, const FrameLayout& lay, bool with_rgb)
{
    const uint32_t off_rgb = with_rgb ? lay.off_rgb : 0u;
    if ((lay.point_step & 3) || (lay.off_x & 3) || (lay.off_y & 3) || (lay.off_z & 3) || (off_rgb & 3))
        return fail(h, HFPF_ERR_BAD_ARG, "%s: fields must be 4-byte aligned", what);
    if (std::max({lay.off_x, lay.off_y, lay.off_z, off_rgb}) + 4 > lay.point_step)
        return fail(h, HFPF_ERR_BAD_ARG, "%s: field offset beyond point_step", what);
    return HFPF_OK;
}

// The cloud can take kFormPacked16: x, y, z at 0, 4, 8 of 16-byte records from a 16-byte aligned base.  with_rgb (integrate, which
// takes the colour from the same load) also asks for rgb at 12 and 16-byte aligned frames.
bool packed16(const FrameLayout& lay, const void* base, bool with_rgb, uint64_t frame_stride = 0)
{
    return lay.point_step == 16 && lay.off_x == 0 && lay.off_y == 4 && lay.off_z == 8 && ((uintptr_t)base & 15) == 0 &&
           (!with_rgb || (lay.off_rgb == 12 && (frame_stride & 15) == 0));
}

// A run-time PointForm as a template argument: fn(std::integral_constant<int, FORM>{}).
template <typename Fn>
void with_form(int form, Fn&& fn)
{
    if (form == kFormDepth) fn(std::integral_constant<int, kFormDepth>{});
    else if (form == kFormPacked16) fn(std::integral_constant<int, kFormPacked16>{});
    else fn(std::integral_constant<int, kFormStrided>{});
}

// A run-time colour switch as a template argument: fn(std::true_type{}) or fn(std::false_type{}).
template <typename Fn>
void with_color(bool color, Fn&& fn)
{
    if (color) fn(std::true_type{});
    else fn(std::false_type{});
}

// ... and k_integrate's colour and bin switches with it: fn(form, color, bin), each an integral constant.
template <typename Fn>
void with_form(int form, bool color, bool bin, Fn&& fn)
{
    auto with_bin = [&](auto B) {
        with_form(form, [&](auto F) {
            if (!color) fn(F, std::false_type{}, B);
            else fn(F, std::true_type{}, B);
        });
    };
    if (bin) with_bin(std::true_type{});
    else with_bin(std::false_type{});
}

// One launch of k_update_cells (REPLAY: in its buffer-replay mode) over nb bricks, the run-time colour and table as constants.
template <bool COLOR, bool WIDE>
constexpr UpdShape kUpdShapeOf = COLOR ? (WIDE ? kUpdWideColor : kUpdDenseColor) : (WIDE ? kUpdWide : kUpdDense);
template <bool REPLAY>
void launch_update_cells(bool color, bool wide, hipStream_t s, const GridParams& g, const Tables& t, uint32_t nb)
{
    with_color(color, [&](auto C) {
        auto launch = [&](auto W) {
            constexpr UpdShape S = kUpdShapeOf<C, W>;
            hipLaunchKernelGGL((k_update_cells<C, S.threads, S.cap, S.slots, S.desc, S.waves, REPLAY>), dim3(nb), dim3(S.threads), 0, s, g, t, nb);
        };
        if (wide) launch(std::true_type{});
        else launch(std::false_type{});
    });
}

// The layout argument of a FORM kernel: *dl for depth images, lay for clouds.
template <int FORM>
const PointLayout<FORM>& form_layout(const FrameLayout& lay, const DepthLayout* dl)
{
    if constexpr (FORM == kFormDepth) return *dl;
    else return lay;
}

// Kernel timing.  An event from the handle's pool (resolve_timing gives them back), or a new one.
hipError_t pooled_event(hfpf_handle* h, hipEvent_t* e)
{
    if (h->ev_free.empty()) return hipEventCreate(e);
    *e = h->ev_free.back();
    h->ev_free.pop_back();
    return hipSuccess;
}

// Brackets work on the engine's stream with a pooled event pair when timing is on (with timing off it touches nothing).  The
// constructor takes the pair and records its first event (check `rc`); file(id) records the second and files the pair under the
// id's row, where resolve_timing finds it.  A pair that is never filed -- the call left early -- goes back to the pool.
struct Timed {
    hfpf_handle* h;
    std::pair<hipEvent_t, hipEvent_t> pr{nullptr, nullptr};
    int rc;
    explicit Timed(hfpf_handle* h_) : h(h_), rc(h_->timing ? begin() : HFPF_OK) {}
    Timed(const Timed&) = delete;
    ~Timed()
    {
        if (pr.first) h->ev_free.push_back(pr.first);
        if (pr.second) h->ev_free.push_back(pr.second);
    }
    int file(int id)
    {
        if (!pr.second) return HFPF_OK;
        HIPCHK(h, hipEventRecord(pr.second, h->stream));
        h->timed[id].pending.push_back(pr);
        pr = {nullptr, nullptr};
        return HFPF_OK;
    }

  private:
    int begin()
    {
        HIPCHK(h, pooled_event(h, &pr.first));
        HIPCHK(h, pooled_event(h, &pr.second));
        HIPCHK(h, hipEventRecord(pr.first, h->stream));
        return HFPF_OK;
    }
};
// ... around one kernel launch (the march launches of raycast, kTimeRaycast)
template <typename Launch>
int timed_launch(hfpf_handle* h, int id, Launch&& launch)
{
    Timed timed(h);
    if (timed.rc) return timed.rc;
    launch();
    HIPCHK(h, hipGetLastError());
    return timed.file(id);
}

// dl != nullptr: the frames are depth images (dev_base / frame_stride address the depth images, n_points = width * height, the
// cloud layout is unused); the caller has validated them (depth_spec, plus the device alignment of hfpf_integrate_depth_device).
int integrate_device_locked(hfpf_handle* h, const void* dev_base, uint32_t n_frames, uint64_t frame_stride, uint32_t n_points,
                            uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z, uint32_t off_rgb, const double* poses,
                            const uint32_t* frame_ids, const DepthLayout* dl = nullptr)
{
    if (!dev_base || !poses || n_frames == 0) return fail(h, HFPF_ERR_BAD_ARG, "integrate: null buffer/poses or zero frames");
    if (n_points == 0) return HFPF_OK;
    const FrameLayout lay{point_step, off_x, off_y, off_z, off_rgb};
    if (!dl && (((uintptr_t)dev_base & 3) || (frame_stride & 3))) return fail(h, HFPF_ERR_BAD_ARG, "integrate: fields must be 4-byte aligned");
    int rc;
    if (!dl && (rc = check_cloud_layout(h, "integrate", lay, true))) return rc;
    if (n_frames > 65535) return fail(h, HFPF_ERR_BAD_ARG, "integrate: at most 65535 frames per call");
    h->ss.pub_seq = 0;  // kernels are about to be enqueued: a counter snapshot already on its way is no longer the latest
    h->ss.early_seq = 0;
    StageSlot* s = nullptr;
    if ((rc = acquire_stage(h, n_frames, &s))) return rc;
    memcpy(s->h_pose, poses, (size_t)n_frames * 12 * sizeof(double));
    for (uint32_t f = 0; f < n_frames; f++) {
        const uint32_t id = frame_ids ? frame_ids[f] : h->ss.next_frame_id + f;
        if (id >= h->t.max_frames) return fail(h, HFPF_ERR_CAPACITY, "frame id %u >= max_frames %llu", id, (unsigned long long)h->t.max_frames);
        s->h_ids[f] = id;
    }
    if (!frame_ids) h->ss.next_frame_id += n_frames;
    HIPCHK(h, hipMemcpyAsync(s->d_pose, s->h_pose, (size_t)n_frames * (12 * sizeof(double) + sizeof(uint32_t)), hipMemcpyHostToDevice, h->stream));  // poses + ids

    const int form = dl ? kFormDepth : packed16(lay, dev_base, true, frame_stride) ? kFormPacked16 : kFormStrided;
    const dim3 block(256);
    const uint64_t pts = (uint64_t)n_points * n_frames;
    const uint64_t n_tiles = (uint64_t)blocks_for(n_points, 256) * n_frames;
    // (hfpf_config.frame_width; a depth frame carries its own width)
    const uint32_t row_w = tile_row_width(dl ? dl->width : h->cfg.frame_width, n_points);
    const dim3 grid((unsigned)std::min<uint64_t>(n_tiles, (uint64_t)h->integrate_grid));
    Timed timed(h);
    if (timed.rc) return timed.rc;
    const bool color = h->t.color != 0;
    const bool bin = h->binned;
    // (ahead of the dry run: its read-back cannot change the answer, normal records exist only behind a pass that set normals_possible)
    const OrderPlan order = plan_order(h->h_ctr[C_NORMALS], h->ss.normals_possible, h->knobs.clean_overlap, h->mbox != nullptr, n_frames, h->dist_on);
    // k_integrate on the batch's first launch_frames frames; probe = 1: the dry run
    auto launch_integrate = [&](dim3 grid_, bool bin_, uint32_t launch_frames, uint32_t log_rot, uint32_t probe) {
        with_form(form, color, bin_, [&](auto F, auto C, auto B) {
            hipLaunchKernelGGL((k_integrate<F == kFormPacked16, C, B, F == kFormDepth>), grid_, block, 0, h->stream, IntegrateArgs{h->g, h->t},
                               (const uint8_t*)dev_base, frame_stride, n_points, launch_frames, form_layout<F>(lay, dl), (const double*)s->d_pose,
                               (const uint32_t*)s->d_ids, row_w, log_rot, probe, order.update ? 1u : 0u);
        });
    };
    // no region exists: every lane takes the direct forms (or none, in the dry run) and the demand is recorded
    auto reset_bins = [&]() -> hipError_t {
        hipError_t e = hipMemsetAsync(&h->t.ctr[C_OVF], 0, sizeof(unsigned long long), h->stream);  // (k_bin_place does this where there is a plan)
        if (!e) e = hipMemsetAsync(h->t.bin_fill, 0, 2 * (h->t.max_bricks + 2) * 4, h->stream);
        if (!e) e = hipMemsetAsync(h->t.bin_capb, 0, 2 * (h->t.max_bricks + 2) * 4, h->stream);
        return e;
    };
    const uint32_t probe_frames = probe_frames_for(n_frames);
    if (wants_probe(bin, h->ss.bin_have_hist, n_frames, probe_frames)) {
        // A dry run of the batch's first frames claims their bricks and records the per-region demand, so that the real launch
        // below parks from its first point.  One extra read-back (the brick count), once per session.
        HIPCHK(h, reset_bins());
        const dim3 pgrid((unsigned)std::min<uint64_t>((uint64_t)blocks_for(n_points, 256) * probe_frames, (uint64_t)h->integrate_grid));
        launch_integrate(pgrid, true, probe_frames, 0, 1);
        HIPCHK(h, hipGetLastError());
        int rcp = read_counters(h);  // bricks the dry run claimed
        if (rcp) return rcp;
        h->ss.bin_have_hist = true;
        h->ss.bin_from_probe = true;  // the plan of the launch below comes from a sample: more slack per region
        h->ss.bin_prev_points = (double)n_points * probe_frames;
    }
    const BinPlan bp = plan_bins({bin, h->ss.bin_have_hist, h->ss.bin_from_probe, h->ss.n_bricks_known, h->ss.n_bricks_before, h->t.max_bricks,
                                  h->ss.bin_prev_points, h->knobs.bin_spare, h->knobs.bin_slack, h->knobs.test_bin_scale}, pts);
    const uint32_t nb = bp.nb;
    if (bin) {
        if (bp.too_large) return fail(h, HFPF_ERR_BAD_ARG, "integrate: batch too large for the binned update (split the call)");
        if (h->bin_pool < bp.pool) {
            int rc2 = scratch(h, h->bin_pt_buf, bp.pool * sizeof(float4));
            if (rc2) return rc2;
            if (color && (rc2 = scratch(h, h->bin_rgb_buf, bp.pool * 4))) return rc2;
            h->bin_pool = bp.pool;
        }
        h->t.bin_pt = (float4*)h->bin_pt_buf.p;
        h->t.bin_rgb = (uint32_t*)h->bin_rgb_buf.p;
        // the overflow list holds a whole launch: a batch without a plan, or one that looks at a new part of the scene, parks nothing
        if (h->ovf_pt_buf.bytes < pts * sizeof(float4) || h->ovf_aux_buf.bytes < pts * sizeof(uint2)) {
            int rc2 = scratch(h, h->ovf_pt_buf, pts * sizeof(float4));
            if (!rc2) rc2 = scratch(h, h->ovf_aux_buf, pts * sizeof(uint2));
            if (rc2) return rc2;
        }
        h->t.ovf_pt = (float4*)h->ovf_pt_buf.p;
        h->t.ovf_aux = (uint2*)h->ovf_aux_buf.p;
        h->t.ovf_cap = pts;
        if (bp.have_plan) {
            const uint32_t n_regions = 2u * (bp.nb_known + 1u);  // two per brick: cells with / without a normal
            const uint32_t n_planned = 2u * (nb + 1u);        // ... and the spare ones behind them
            const uint32_t all_regions = 2u * (uint32_t)(h->t.max_bricks + 2);
            int rc2 = scratch(h, h->bin_sums, (size_t)blocks_for(all_regions, kBinPlanTile) * sizeof(uint32_t));
            if (rc2) return rc2;
            hipLaunchKernelGGL(k_bin_plan, dim3(blocks_for(n_planned, kBinPlanTile)), dim3(256), 0, h->stream, h->t, n_regions, n_planned, bp.spare_cap, bp.scale,
                               bp.slack, (uint32_t*)h->bin_sums.p);
            h->ss.bin_from_probe = false;
            hipLaunchKernelGGL(k_bin_place, dim3(blocks_for(all_regions, kBinPlanTile)), dim3(256), 0, h->stream, h->t, n_planned, all_regions, h->bin_pool,
                               (const uint32_t*)h->bin_sums.p);
        } else {  // no plan yet
            HIPCHK(h, reset_bins());
        }
    }
    const uint32_t log_rot = (uint32_t)((h->launch_seq++ * 17u) & (kLogRegions - 1));
    // Detail timing: four events per call and one byte saying which of the three kernels between them ran.  A call that leaves
    // early gives its events back, so the records stay aligned.
    struct DetailGuard {
        hfpf_handle* h;
        size_t first;
        bool done = false;
        ~DetailGuard()
        {
            if (done) return;
            while (h->ev_detail.size() > first) {
                h->ev_free.push_back(h->ev_detail.back());
                h->ev_detail.pop_back();
            }
        }
    } detail_guard{h, h->ev_detail.size()};
    uint8_t detail_ran = 1;  // k_integrate (+ its overflow kernel) always runs
    unsigned long long early_seq = 0;
    auto detail_mark = [&]() -> hipError_t {  // per-kernel boundaries of this call (detail timing only)
        if (!h->timing_detail) return hipSuccess;
        hipEvent_t e = nullptr;
        if (hipError_t r = pooled_event(h, &e)) return r;
        h->ev_detail.push_back(e);
        return hipEventRecord(e, h->stream);
    };
    HIPCHK(h, detail_mark());
    launch_integrate(grid, bin, n_frames, log_rot, 0);
    if (!bin) {
        for (int k = 0; k < 3; k++) HIPCHK(h, detail_mark());
    } else {
        {  // the points that found no room in a bin (usually a few thousand, everything for a batch without a plan): direct forms
            const unsigned ogrid = (unsigned)std::min<uint64_t>(blocks_for(pts, 256), 8ull * 256);
            with_color(color, [&](auto C) { hipLaunchKernelGGL(k_integrate_overflow<C>, dim3(ogrid), dim3(256), 0, h->stream, h->g, h->t, log_rot); });
        }
        HIPCHK(h, detail_mark());
        if (bp.have_plan) {
            auto launch_buffer = [&]() {
                detail_ran |= 4;
                with_color(color, [&](auto C) { hipLaunchKernelGGL(k_buffer<C>, dim3(nb), dim3(256), 0, h->stream, h->g, h->t, nb); });
            };
            if (order.buffer_first) {  // ... ahead of the update kernel (plan_order)
                detail_ran |= 8;  // events 1..2 bracket k_buffer and 2..3 the update kernel (resolve_timing)
                launch_buffer();
                early_seq = ++h->mbox_seq;
                k_publish_counters<<<1, 256, 0, h->stream>>>(h->t.ctr, h->t.log_ctr, h->mbox + kMboxSlotWords, early_seq);
                HIPCHK(h, hipGetLastError());
                HIPCHK(h, hipEventRecord(h->ev_ready, h->stream));
                HIPCHK(h, detail_mark());
            }
            if (order.update) {
                detail_ran |= 2;
                if (h->knobs.update_cells) {
                    if ((rc = window_from_final(h))) return rc;
                    launch_update_cells<false>(color, pick_update_shape(h) == 1, h->stream, h->g, h->t, nb);
                } else {
                    with_color(color, [&](auto C) { hipLaunchKernelGGL(k_update<C>, dim3(nb), dim3(kUpdThreads), 0, h->stream, h->g, h->t, nb); });
                }
            }
            HIPCHK(h, detail_mark());
            if (!order.buffer_first) {
                launch_buffer();
                HIPCHK(h, detail_mark());
            }
        } else {
            HIPCHK(h, detail_mark());
            HIPCHK(h, detail_mark());
        }
        h->ss.bin_have_hist = true;
        h->ss.bin_prev_points = (double)n_points * n_frames;
    }
    HIPCHK(h, hipGetLastError());
    if (h->timing_detail) h->ev_detail_ran.push_back(detail_ran);
    detail_guard.done = true;
    if ((rc = timed.file(kTimeIntegrate))) return rc;
    HIPCHK(h, hipEventRecord(s->done, h->stream));
    s->pending = true;
    h->ss.dirty = true;  // state_changed = true, grid.hpp:189
    h->frames_integrated += n_frames;
    if (order.final_publish) {  // a batch: the next call is probably a clean pass, which starts by reading the counters
        if ((rc = window_from_final(h))) return rc;  // (a final publish nobody has read yet is about to be overwritten)
        h->ss.pub_seq = ++h->mbox_seq;
        k_publish_counters<<<1, 256, 0, h->stream>>>(h->t.ctr, h->t.log_ctr, h->mbox, h->ss.pub_seq);
        HIPCHK(h, hipGetLastError());
        h->ss.early_seq = early_seq;
    } else {
        h->ss.pub_seq = 0;
    }
    return HFPF_OK;
}

int resolve_timing(hfpf_handle* h)
{
    bool pending = !h->ev_detail.empty();
    for (const TimedId& t : h->timed) pending = pending || !t.pending.empty();
    if (!pending) return HFPF_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (TimedId& t : h->timed) {
        for (auto& pr : t.pending) {
            float ms = 0.f;
            HIPCHK(h, hipEventElapsedTime(&ms, pr.first, pr.second));
            t.ms += (double)ms;
            t.n++;
            h->ev_free.push_back(pr.first);
            h->ev_free.push_back(pr.second);
        }
        t.pending.clear();
    }
    for (size_t c = 0; 4 * c + 3 < h->ev_detail.size() && c < h->ev_detail_ran.size(); c++) {
        for (int k = 0; k < 3; k++) {
            if (!(h->ev_detail_ran[c] & (1u << k))) continue;  // not launched in this call (e.g. no dependants yet: no k_update_cells)
            const int at = (k && (h->ev_detail_ran[c] & 8u)) ? 3 - k : k;  // k_buffer ran ahead of the update kernel: their brackets change places
            float ms = 0.f;
            HIPCHK(h, hipEventElapsedTime(&ms, h->ev_detail[4 * c + at], h->ev_detail[4 * c + at + 1]));
            h->timed[kTimeDetail + k].ms += (double)ms;
            h->timed[kTimeDetail + k].n++;
        }
    }
    for (hipEvent_t e : h->ev_detail) h->ev_free.push_back(e);
    h->ev_detail.clear();
    h->ev_detail_ran.clear();
    return HFPF_OK;
}


// ---- RCCL, resolved with dlopen/dlsym ---------------------------------------------------------------
// (same ABI as <rccl/rccl.h>; declared here so libhfpf.so has no link-time dependency on librccl)
typedef struct ncclComm* ncclComm_t_;
typedef struct { char internal[128]; } ncclUniqueId_;
enum { ncclSuccess_ = 0 };
enum { ncclChar_ = 0, ncclUint64_ = 5 };  // ncclInt8/ncclChar = 0, ncclUint64 = 5 (rccl.h ncclDataType_t)
enum { ncclSum_ = 0 };
struct RcclApi {
    int (*GetUniqueId)(ncclUniqueId_*) = nullptr;
    int (*CommInitRank)(ncclComm_t_*, int, ncclUniqueId_, int) = nullptr;
    int (*CommDestroy)(ncclComm_t_) = nullptr;
    int (*CommCount)(const ncclComm_t_, int*) = nullptr;
    int (*CommUserRank)(const ncclComm_t_, int*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, ncclComm_t_, hipStream_t) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, ncclComm_t_, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    void* lib = nullptr;
};
RcclApi g_rccl;
std::mutex g_rccl_mtx;

int load_rccl(std::string& err)
{
    std::lock_guard<std::mutex> lk(g_rccl_mtx);
    if (g_rccl.lib) return 0;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void* lib = nullptr;
    for (const char* n : names)
        if ((lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!lib) {
        err = std::string("cannot load librccl: ") + dlerror();
        return -1;
    }
    RcclApi a;
    a.lib = lib;
    a.GetUniqueId = (decltype(a.GetUniqueId))dlsym(lib, "ncclGetUniqueId");
    a.CommInitRank = (decltype(a.CommInitRank))dlsym(lib, "ncclCommInitRank");
    a.CommDestroy = (decltype(a.CommDestroy))dlsym(lib, "ncclCommDestroy");
    a.CommCount = (decltype(a.CommCount))dlsym(lib, "ncclCommCount");
    a.CommUserRank = (decltype(a.CommUserRank))dlsym(lib, "ncclCommUserRank");
    a.AllGather = (decltype(a.AllGather))dlsym(lib, "ncclAllGather");
    a.AllReduce = (decltype(a.AllReduce))dlsym(lib, "ncclAllReduce");
    a.GetErrorString = (decltype(a.GetErrorString))dlsym(lib, "ncclGetErrorString");
    if (!a.GetUniqueId || !a.CommInitRank || !a.AllGather || !a.AllReduce) {
        err = "librccl lacks a required symbol";
        return -1;
    }
    g_rccl = a;
    return 0;
}

#define NCCLCHK(h, call)                                                                                              \
    do {                                                                                                              \
        int r_ = (call);                                                                                              \
        if (r_ != ncclSuccess_)                                                                                       \
            return fail(h, HFPF_ERR_DIST, "%s failed: %s", #call, g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "?"); \
    } while (0)

// Export the cells this handle occupied since the last exchange into h->ex_send; returns the count.
int epoch_export_locked(hfpf_handle* h, uint64_t* n_out, uint64_t min_capacity_records)
{
    int rc = read_counters(h);
    if (rc) return rc;
    if ((rc = check_device_errors(h))) return rc;
    const uint64_t n_occ = std::min<uint64_t>(h->h_ctr[C_OCC], h->t.max_occ);
    const uint64_t n_cells = n_occ - std::min(n_occ, h->ss.occ_exported);
    const uint64_t n_fr_all = std::min<uint64_t>(h->h_ctr[C_FRAMES], h->t.max_frames);
    const uint64_t n_frames = n_fr_all - std::min(n_fr_all, h->ss.frames_exported);
    const uint64_t n_new = n_cells + 2 * n_frames;  // one record per cell, two per frame (its viewpoint)
    if ((rc = scratch(h, h->ex_send, std::max<uint64_t>(std::max(n_new, min_capacity_records), 1) * sizeof(EpochRec)))) return rc;
    if (n_new) {
        hipLaunchKernelGGL(k_epoch_export, dim3(blocks_for(n_new, 256)), dim3(256), 0, h->stream, h->g, h->t, h->ss.occ_exported, n_cells, h->ss.frames_exported, n_frames,
                           (EpochRec*)h->ex_send.p);
        HIPCHK(h, hipGetLastError());
    }
    h->ss.frames_seen = n_fr_all;  // (the clean pass that follows the exchange marks them exchanged, like the cells)
    *n_out = n_new;
    return HFPF_OK;
}

int epoch_import_locked(hfpf_handle* h, const void* dev_records, uint64_t n)
{
    if (n == 0) return HFPF_OK;
    h->ss.pub_seq = 0;  // the import changes counters behind any snapshot already on its way
    hipLaunchKernelGGL(k_epoch_import, dim3(blocks_for(n, 256 * kImportTiles)), dim3(256), 0, h->stream, h->g, h->t, (const EpochRec*)dev_records, n);
    HIPCHK(h, hipGetLastError());
    return HFPF_OK;
}

// Device records [0, n) of one rank's slice of a gathered exchange buffer -> this handle's tables.  The one place both
// transports (RCCL all-gather below, hfpf_epoch_import for host-staged / virtual ranks) go through.
int import_rank_slice_locked(hfpf_handle* h, const void* dev_buffer, uint64_t slice_stride_bytes, int src_rank, uint64_t n_records)
{
    if (n_records == 0) return HFPF_OK;
    return epoch_import_locked(h, (const char*)dev_buffer + (size_t)src_rank * slice_stride_bytes, n_records);
}

// Every other rank's slice of an all-gathered buffer (world slices of slice_stride_bytes; slice r holds counts[r] records, the
// rest of it is padding that is never read).
int import_gathered_locked(hfpf_handle* h, const void* dev_buffer, uint64_t slice_stride_bytes, int world, int my_rank, const unsigned long long* counts)
{
    for (int r = 0; r < world; r++)  // every count is judged before any slice is imported: a refused call imports nothing
        if (r != my_rank && counts[r] > slice_stride_bytes / sizeof(EpochRec)) return fail(h, HFPF_ERR_BAD_ARG, "gathered slice %d: %llu records do not fit the stride", r, counts[r]);
    for (int r = 0; r < world; r++) {
        if (r == my_rank) continue;
        if (int rc = import_rank_slice_locked(h, dev_buffer, slice_stride_bytes, r, counts[r])) return rc;
    }
    return HFPF_OK;
}

// Failure consensus in front of a data collective: every rank contributes ONE status word (a payload below 2^63, bit 63 = "this
// rank has failed") to an all-gather that it enters whatever happened to it locally -- the status gather itself needs nothing but
// the (world+1)-word buffer allocated by hfpf_dist_init.  Afterwards every rank knows whether any rank failed and all of them
// leave the collective sequence at the same point: the failed rank with its own error, the others with HFPF_ERR_DIST.  Without
// it a rank that returns early (capacity overflow, poisoned handle, failed allocation) leaves its peers blocked in the next
// ncclAllGather / ncclAllReduce for ever.  payloads_out (world entries, may be null) receives every rank's payload.
// h->ex_counts: the status word of every rank, then this rank's own (what it sends into the gather).
ScratchLayout ex_counts_layout(int world, unsigned long long** all, unsigned long long** mine)
{
    return ScratchLayout().add(all, (uint64_t)world).add(mine, 1);
}

int dist_status_gather_locked(hfpf_handle* h, int local_rc, uint64_t payload, const char* where, unsigned long long* payloads_out)
{
    constexpr unsigned long long kFailBit = 1ull << 63;
    const std::string local_err = h->err;  // keep the text of the local failure: the calls below may overwrite it
    if (!h->ex_counts.p || !h->h_counts) return fail(h, HFPF_ERR_DIST, "%s: no status buffer (hfpf_dist_init did not complete)", where);
    unsigned long long *d_counts, *d_mine;
    ex_counts_layout(h->world, &d_counts, &d_mine).place(h->ex_counts.p);  // allocated by hfpf_dist_init alone, never grown
    h->h_counts[h->world] = (payload & ~kFailBit) | (local_rc ? kFailBit : 0ull);
    HIPCHK(h, hipMemcpyAsync(d_mine, h->h_counts + h->world, 8, hipMemcpyHostToDevice, h->stream));
    NCCLCHK(h, g_rccl.AllGather(d_mine, d_counts, 1, ncclUint64_, (ncclComm_t_)h->comm, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->h_counts, d_counts, (size_t)h->world * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    int failed_rank = -1;
    for (int r = 0; r < h->world; r++) {
        if ((h->h_counts[r] & kFailBit) && failed_rank < 0) failed_rank = r;
        h->h_counts[r] &= ~kFailBit;
        if (payloads_out) payloads_out[r] = h->h_counts[r];
    }
    if (local_rc) {
        h->err = local_err;
        return local_rc;
    }
    if (failed_rank >= 0) return fail(h, HFPF_ERR_DIST, "rank %d failed before the %s; the call is abandoned on every rank", failed_rank, where);
    return HFPF_OK;
}

// Exchange buffers for `records` records per rank.  The send buffer keeps its first `keep` records.
int grow_exchange_buffers_locked(hfpf_handle* h, uint64_t records, uint64_t keep)
{
    int rc;
    if (h->ex_send.bytes < records * sizeof(EpochRec)) {
        std::vector<DevBuf*> unregistered;  // (the allocation moves into ex_send below)
        DevBuf bigger(unregistered);
        if ((rc = scratch(h, bigger, records * sizeof(EpochRec)))) return rc;
        if (keep) HIPCHK(h, hipMemcpyAsync(bigger.p, h->ex_send.p, keep * sizeof(EpochRec), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (h->ex_send.p) {
            HIPCHK(h, hipFree(h->ex_send.p));
            h->device_bytes -= h->ex_send.bytes;
        }
        h->ex_send.p = bigger.p, h->ex_send.bytes = bigger.bytes;
    }
    return scratch(h, h->ex_recv, (size_t)h->world * records * sizeof(EpochRec));
}

// RCCL exchange at the head of a clean pass: status gather (with the per-rank record counts as payload), then the all-gather of
// the padded record lists.  pre_rc != 0: this rank failed before the call (poisoned handle); it still takes part in the status
// gather so that its peers return an error instead of waiting for it.  Nothing that can fail sits between two collectives
// without a status gather behind it: the buffers hold ex_cap_records per rank -- the same number on every rank, because it
// starts from the same configuration and grows by the same rule from the same gathered maximum -- so "must grow" is the same
// decision everywhere, and the ranks that grow agree on the outcome before the record gather.
int dist_exchange_locked(hfpf_handle* h, int pre_rc)
{
    uint64_t n_mine = 0;
    int local_rc = pre_rc;
    if (!local_rc) local_rc = epoch_export_locked(h, &n_mine, h->ex_cap_records);
    if (local_rc) n_mine = 0;
    int rc = dist_status_gather_locked(h, local_rc, n_mine, "epoch exchange", nullptr);
    if (rc) return rc;
    uint64_t maxc = 0;
    for (int r = 0; r < h->world; r++) maxc = std::max<uint64_t>(maxc, h->h_counts[r]);
    if (maxc == 0) return HFPF_OK;
    if (maxc > h->ex_cap_records) {
        const uint64_t new_cap = maxc + maxc / 4;
        const int grc = grow_exchange_buffers_locked(h, new_cap, n_mine);
        std::vector<unsigned long long> counts(h->h_counts, h->h_counts + h->world);  // the second gather reuses h_counts
        if ((rc = dist_status_gather_locked(h, grc, new_cap, "growth of the exchange buffers", nullptr))) return rc;
        std::copy(counts.begin(), counts.end(), h->h_counts);
        h->ex_cap_records = new_cap;
    }
    NCCLCHK(h, g_rccl.AllGather(h->ex_send.p, h->ex_recv.p, maxc * sizeof(EpochRec), ncclChar_, (ncclComm_t_)h->comm, h->stream));
    return import_gathered_locked(h, h->ex_recv.p, maxc * sizeof(EpochRec), h->world, h->rank, h->h_counts);
}

// k_gate with four tiles per workgroup only when the input is large enough to fill the chip that way (one reservation per
// list and workgroup; small inputs keep one tile so that the latency-heavy stencil probes spread over as many CUs as possible).
void launch_gate(hfpf_handle* h, hipStream_t s, const uint32_t* cells_a, uint64_t n_a, const uint32_t* cells_b, uint64_t n_b, uint32_t* pend_out)
{
    const uint64_t n = n_a + n_b;
    if (gate_tiles(n, h->knobs.limits) == 4)
        hipLaunchKernelGGL(k_gate<4>, dim3(blocks_for(n, 256 * 4)), dim3(256), 0, s, h->g, h->t, cells_a, n_a, cells_b, n_b, pend_out);
    else
        hipLaunchKernelGGL(k_gate<1>, dim3(blocks_for(n, 256)), dim3(256), 0, s, h->g, h->t, cells_a, n_a, cells_b, n_b, pend_out);
}

// One clean pass.  Two host read-backs: at the start (what the integrate launches since the last pass produced) and after the
// dependant-table update (how many cells to replay, overflow bits).  Everything between them is sized from upper bounds on the
// host and reads its exact counts from the device counters.
//
// The front half -- sentinels, gate, candidate sort, k_normal, k_register: a chain of small launches over a few ten thousand
// candidates -- reads nothing the update kernel of the integrate call before it writes (the statistic sums and its pair counters),
// and writes nothing that kernel reads for the cells it is written for (cand_key, the pending lists, the records of NEW ids and
// their lines, stat_id, bit 1 of an info word and the nd_mask bit of a candidate, pre_dep of UNOCCUPIED cells, reg_occ, dep_tmp,
// touched_list, directory entries of bricks beyond the call's; the update reads the list bits of info words, pre_dep of occupied
// cells, dep[] and the lines of older records).  So when that call is still pending and left an early publish (integrate_device_locked), the pass takes its
// head-of-pass counters from it and runs the front half on front_stream beside the update kernel: front_stream waits for
// ev_ready, the engine's stream for ev_front, and the back half -- the filing of pre-dependants (it rewrites info words the
// update reads: k_clean_file), the dependant-table update, the replays -- follows on the engine's stream as ever.  Scratch: pend_b,
// keys_a and sort_tmp are the front half's alone until ev_front; the engine's stream holds only the update kernel and a publish.
// A small (no-wait) overlapped pass also replays there, behind k_register (k_replay_reg, HFPF_EARLY_REPLAY=0 switches it off).  It
// READS reg_occ from the pass's first registration on, nv_line of the new records, buf_head and the log -- chains and log are final
// behind k_integrate_overflow and k_buffer, ahead of ev_ready, and the update kernel appends to neither -- and WRITES integer atomic
// adds into the statistics of the NEW records (no list names them yet, so the update kernel adds to none of them) and into the
// striped replay counter (word 1 of the log_ctr lines; the update kernel's are words 2 and 3).  It touches neither info, dep[] nor
// dep_tmp, so the back half -- file, offsets, fill -- runs beside it; k_depinc_fill then leaves no note, and the engine's stream
// waits for ev_replay at the end of the pass, ahead of whatever appends to the log, publishes or reads next.
// The early publish cannot show an error bit the update kernel raises: like the errors of a no-wait pass it surfaces at the next
// read-back and poisons the handle there.  Everything else -- no call pending, a read-back since (hfpf_sync, hfpf_get_counters),
// a distributed session, the un-binned forms, a compacting pass, HFPF_CLEAN_OVERLAP=0 -- is the plain sequence on one stream.
// Who decides (host_plan.hpp): clean_starts_early whether the head-of-pass counters come from the early publish; plan_clean, from
// those counters, whether the pass compacts, overlaps, waits, replays early; plan_replay the replay of a waited pass.  This function
// enqueues what they say, and changes one answer only: a pass whose incremental update ran out of dep[] compacts after all.
int clean_locked(hfpf_handle* h, int pre_rc)
{
    Tables& t = h->t;
    int rc;
    // collective: every rank cleans at the same schedule point; a rank that is already unusable (pre_rc) still says so to its peers
    if (h->dist_on && (rc = dist_exchange_locked(h, pre_rc))) return rc;
    if (pre_rc) return pre_rc;
    const bool early = clean_starts_early(h->knobs.clean_overlap, h->dist_on, h->binned, h->mbox != nullptr, h->ss.pub_seq, h->ss.early_seq);
    if ((rc = read_counters(h, early))) return rc;
    if ((rc = check_device_errors(h))) return rc;
    const unsigned long long* c = h->h_ctr;
    const CleanPlan p = plan_clean({c[C_OCC], c[C_NORMALS], c[C_PEND], c[C_REG], c[C_PREREG], c[C_DEP]}, t.max_occ, t.max_reg, t.max_dep, h->ss.gate_done,
                                   h->ss.pend_valid, h->g.K, early, h->knobs.clean_small_nowait, h->knobs.early_replay, h->knobs.limits);
    const uint64_t n_occ = p.n_occ, n_normals = p.n_normals, n_pend = p.n_pend, n_new_occ = p.n_new_occ, n_in = p.n_in, reg_ub = p.reg_ub;
    h->ss.occ_exported = n_occ;  // everything occupied so far (locally or imported) has been exchanged
    h->ss.frames_exported = std::max(h->ss.frames_exported, h->ss.frames_seen);  // ... and the viewpoints of the frames the last export covered
    h->ss.dirty = false;  // state_changed = false, grid.hpp:313
    h->clean_passes++;

    {
        LinkRanges lr;
        uint64_t max_new = 0;
        for (int r = 0; r < kLogRegions; r++) {
            const uint64_t n_r = std::min<uint64_t>(h->h_log_ctr[r * 16], t.log_region_cap);
            const uint64_t base = (uint64_t)r * t.log_region_cap;
            lr.first[r] = (uint32_t)(base + h->ss.n_linked[r] + 1);
            lr.last[r] = (uint32_t)(base + n_r);
            max_new = std::max(max_new, n_r - h->ss.n_linked[r]);
            h->ss.n_linked[r] = n_r;
        }
        // entries appended by k_buffer arrive chained; only k_integrate's direct form leaves marked entries behind
        if (max_new && !h->binned && h->h_ctr[C_BUFFERED] != h->ss.direct_linked) {  // (the binned form chains its few direct appends itself)
            hipLaunchKernelGGL(k_link_log, dim3(blocks_for(max_new, 256), kLogRegions), dim3(256), 0, h->stream, t, lr);
            HIPCHK(h, hipGetLastError());
        }
        h->ss.direct_linked = h->h_ctr[C_BUFFERED];
    }
    if (n_occ == 0 || n_in == 0) return HFPF_OK;  // no candidates: nothing to do

    if ((rc = scratch(h, h->pend_b, n_in * 4))) return rc;
    if ((rc = scratch(h, h->keys_a, n_in * 8))) return rc;
    const uint32_t* new_cells = (const uint32_t*)(t.occ_list + h->ss.gate_done);
    if (h->knobs.trace_clean)
        fprintf(stderr, "hfpf: clean pass %llu: %llu candidates, front half %s, replay %s\n", (unsigned long long)h->clean_passes, (unsigned long long)n_in,
                p.overlap ? "beside the update kernel" : "on the engine's stream", p.replay_early ? "fed from the registrations" : "behind the dependant-table update");
    // ... and a second line with the size-gated forms the pass takes (CleanLimits): a no-wait pass knows them here, a waited one ahead of its replay
    const auto trace_forms = [&](const ReplayPlan* rp, uint64_t touched, const char* compacting) {
        if (!h->knobs.trace_clean) return;
        char tail[160];
        if (rp)
            snprintf(tail, sizeof tail, "waited: single %llu, walked %llu, %s, use_marks %u", (unsigned long long)(touched - rp->walked), (unsigned long long)rp->walked,
                     rp->walked && rp->sort_walked ? "sorted" : "unsorted", rp->use_marks);
        else
            snprintf(tail, sizeof tail, "no-wait");
        fprintf(stderr, "hfpf: clean forms %llu: gate tiles %d (%llu pending + %llu new), register %s, compacting %s, %s\n", (unsigned long long)h->clean_passes,
                gate_tiles(n_in, h->knobs.limits), (unsigned long long)n_pend, (unsigned long long)n_new_occ, register_large(n_in, h->knobs.limits) ? "large" : "small", compacting, tail);
    };
    if (p.no_wait) trace_forms(nullptr, 0, "no");
    // the front half: beside the update kernel on a stream of its own, or on the engine's like everything behind k_register
    const hipStream_t front = p.overlap ? h->front_stream : h->stream;
    if (p.overlap) {
        HIPCHK(h, hipStreamWaitEvent(front, h->ev_ready, 0));
        hipLaunchKernelGGL(k_clean_front, dim3(blocks_for(n_in, 256)), dim3(256), 0, front, t, n_in);
    } else {
        // sentinels + the pass's list counters + the pre-dependants of the cells occupied since the last pass become their lists
        hipLaunchKernelGGL(k_clean_begin, dim3(blocks_for(n_in, 256)), dim3(256), 0, front, t, n_in, new_cells, n_new_occ, p.full ? 1u : 0u);
    }
    launch_gate(h, front, (const uint32_t*)h->pend_a.p, n_pend, new_cells, n_new_occ, (uint32_t*)h->pend_b.p);
    HIPCHK(h, hipGetLastError());
    h->ss.gate_done = n_occ;
    h->ss.normals_possible = true;
    swap(h->pend_a, h->pend_b);  // cells that got a normal in this pass are dropped by the next gate's kNormal test
    h->ss.pend_valid = true;             // C_PEND now counts pend_a; the host reads it at the start of the next pass

    // canonical order: ascending (x,y,z) key; record id = n_normals + rank + 1
    // (with HFPF_MORTON_IDS the candidate keys are Z-order codes: three interleaved axes of the widest axis' bits)
    const unsigned cand_bits = HFPF_MORTON_IDS ? 3u * std::max(h->g.key_sy, std::max(h->g.key_sx - h->g.key_sy, h->g.key_bits - h->g.key_sx)) : h->g.key_bits;
    if ((rc = sort_keys_u64(h, t.cand_key, (uint64_t*)h->keys_a.p, n_in, cand_bits, front))) return rc;
    hipLaunchKernelGGL(k_normal, dim3(blocks_for(n_in, 128)), dim3(128), 0, front, h->g, t, (const uint64_t*)h->keys_a.p, kCountOnDevice, n_normals);
    const bool reg_small = !register_large(n_in, h->knobs.limits);  // tiles per workgroup: kernels.hpp k_register
    const uint64_t reg_tile = 256ull * (reg_small ? kRegTilesSmall : kRegTilesLarge);  // step-major, whole workgroups per step
    const uint64_t reg_blocks = ((n_in + reg_tile - 1) / reg_tile) * (2ull * (uint64_t)h->g.K + 1ull);
    const uint32_t count_deps = p.full ? 0u : 1u;  // (the compacting rebuild counts for itself, from zero)
    if (reg_small) hipLaunchKernelGGL(k_register<kRegTilesSmall>, dim3((unsigned)std::max<uint64_t>(reg_blocks, 1)), dim3(256), 0, front, h->g, t, kCountOnDevice, n_normals, count_deps);
    else hipLaunchKernelGGL(k_register<kRegTilesLarge>, dim3((unsigned)std::max<uint64_t>(reg_blocks, 1)), dim3(256), 0, front, h->g, t, kCountOnDevice, n_normals, count_deps);
    HIPCHK(h, hipGetLastError());
    if (p.overlap) {
        HIPCHK(h, hipEventRecord(h->ev_front, front));
        if (p.replay_early) {  // still beside the update kernel; the engine's stream joins it at the end of the pass (ev_replay)
            with_color(t.color, [&](auto C) {
                hipLaunchKernelGGL(k_replay_reg<C>, dim3(blocks_for(reg_ub * kChains, 256)), dim3(256), 0, front, h->g, t, p.reg_first, kCountOnDevice);
            });
            HIPCHK(h, hipGetLastError());
            HIPCHK(h, hipEventRecord(h->ev_replay, front));
        }
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_front, 0));
        if (n_new_occ) hipLaunchKernelGGL(k_clean_file, dim3(blocks_for(n_new_occ, 256)), dim3(256), 0, h->stream, t, new_cells, n_new_occ);
    }
    // the back half, on the engine's stream
    uint64_t n_reg = 0, n_pre = 0, inc_touched = 0;
    bool full = p.full;  // the one mode a pass may change: dep[] ran out under an incremental update (a reaction to the read-back below, not a plan)
    if (!p.full) {
        hipLaunchKernelGGL(k_depinc_offsets, dim3(blocks_for(reg_ub, 256 * kListTiles)), dim3(256), 0, h->stream, t, kCountOnDevice);
        hipLaunchKernelGGL(k_depinc_fill, dim3(blocks_for(reg_ub, 256)), dim3(256), 0, h->stream, t, p.reg_first, kCountOnDevice, p.replay_early ? 0u : 1u);
        HIPCHK(h, hipGetLastError());
        if (p.replay_early) {  // nothing that appends to the log or the chains, or publishes the counters, gets ahead of the replay
            HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_replay, 0));
            return HFPF_OK;
        }
        if (p.no_wait) {  // errors of this pass (capacity) surface at the next read-back and poison the handle there
            with_color(t.color, [&](auto C) {
                hipLaunchKernelGGL(k_replay<C>, dim3(blocks_for(reg_ub * kChains, 256)), dim3(256), 0, h->stream, h->g, t, (const uint32_t*)t.touched_list, 1u, 0u,
                                   kCountOnDevice, n_normals);
            });
            HIPCHK(h, hipGetLastError());
            return HFPF_OK;
        }
        if ((rc = read_counters(h))) return rc;
        n_reg = std::min<uint64_t>(h->h_ctr[C_REG], t.max_reg);
        n_pre = std::min<uint64_t>(h->h_ctr[C_PREREG], t.max_reg);
        inc_touched = h->h_ctr[C_TOUCHED];
        if (h->h_ctr[C_ERR] == (unsigned long long)E_DEP) {  // dep[] ran out mid-way: compact
            hipLaunchKernelGGL(k_set_ctr, dim3(1), dim3(1), 0, h->stream, t.ctr, (int)C_ERR, 0ull);
            if (inc_touched) hipLaunchKernelGGL(k_dep_reset, dim3(blocks_for(inc_touched, 256)), dim3(256), 0, h->stream, t, inc_touched);  // poisoned cursors
            full = true;
        } else if ((rc = check_device_errors(h))) {
            return rc;
        }
    } else {
        if ((rc = read_counters(h))) return rc;
        if ((rc = check_device_errors(h))) return rc;
        n_reg = std::min<uint64_t>(h->h_ctr[C_REG], t.max_reg);
        n_pre = std::min<uint64_t>(h->h_ctr[C_PREREG], t.max_reg);
    }
    if (full) {
        const uint64_t n_all = n_reg + n_pre;
        if (2 * n_all > t.max_dep)  // (lists own power-of-two blocks: below twice their length)
            return fail(h, HFPF_ERR_CAPACITY, "dependant table: %llu entries do not fit %llu with their blocks", (unsigned long long)n_all, (unsigned long long)t.max_dep);
        // touched_list holds one entry per distinct cell among the n_all registrations: every normal record registers on at most
        // 2K+1 cells, so n_reg + n_pre <= max_normals * (2K+1) = max_reg = max_touched
        if (n_all > h->max_touched) return fail(h, HFPF_ERR_CAPACITY, "registrations: %llu > %llu", (unsigned long long)n_all, (unsigned long long)h->max_touched);
        hipLaunchKernelGGL(k_set_ctr3, dim3(1), dim3(1), 0, h->stream, t.ctr, (int)C_DEP, 0ull, (int)C_TOUCHED, 0ull, -1, 0ull);
        if (n_all) {
            hipLaunchKernelGGL(k_dep_count, dim3(blocks_for(n_all, 256)), dim3(256), 0, h->stream, t, n_reg, n_pre);
            HIPCHK(h, hipGetLastError());
            if ((rc = read_counters(h))) return rc;
            const uint64_t n_touched = h->h_ctr[C_TOUCHED];
            hipLaunchKernelGGL(k_dep_offsets, dim3(blocks_for(n_touched, 256)), dim3(256), 0, h->stream, t, n_touched);
            hipLaunchKernelGGL(k_dep_fill, dim3(blocks_for(n_all, 256)), dim3(256), 0, h->stream, t, n_reg, n_pre);
            hipLaunchKernelGGL(k_dep_reset, dim3(blocks_for(n_touched, 256)), dim3(256), 0, h->stream, t, n_touched);
            HIPCHK(h, hipGetLastError());
            inc_touched = n_touched;  // superset of the cells touched by this pass; k_replay filters by record id
        }
        if ((rc = read_counters(h))) return rc;
        if ((rc = check_device_errors(h))) return rc;
    }
    // buffer replay of the cells that gained registrants in this pass (touched_list is still intact)
    const ReplayPlan rp = plan_replay(inc_touched, h->h_ctr[C_TOUCHED_SINGLE], full, h->binned, h->knobs.stream_replay, h->ss.n_bricks_known, h->knobs.limits);
    trace_forms(&rp, inc_touched, !full ? "no" : p.full ? "planned" : "after the incremental update ran out");
    if (rp.stream) {
        const uint32_t nbk = (uint32_t)h->ss.n_bricks_known;
        const bool wide = h->knobs.upd_shape_forced >= 0 ? h->knobs.upd_shape_forced == 1 : h->upd_wide;  // the shape the dependant updates of this session take
        launch_update_cells<true>(t.color, wide, h->stream, h->g, t, nbk);
        HIPCHK(h, hipGetLastError());
    }
    if (rp.walked) {
        const uint32_t* cells = t.touched_list;
        if (rp.sort_walked) {
            if ((rc = scratch(h, h->vals_a, inc_touched * 4))) return rc;
            if ((rc = sort_keys_u32(h, t.touched_list, (uint32_t*)h->vals_a.p, inc_touched, rp.slot_bits))) return rc;
            cells = (const uint32_t*)h->vals_a.p;
        }
        with_color(t.color, [&](auto C) {
            hipLaunchKernelGGL(k_replay<C>, dim3(blocks_for(inc_touched * kChains, 256)), dim3(256), 0, h->stream, h->g, t, cells, rp.use_marks, rp.stream ? 1u : 0u, inc_touched,
                               n_normals);
        });
        HIPCHK(h, hipGetLastError());
    }
    return HFPF_OK;
}

}  // namespace

// ================================================================================================
extern "C" {

int hfpf_abi_version(void) { return HFPF_ABI_VERSION; }

void hfpf_default_config(hfpf_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof *c;
    c->resolution = 0.005f;  // kResolution node.cpp:91
    const double box[6] = {-0.80, 1.80, -1.5, 1.5, 0.0, 1.0};  // launch file line 7
    memcpy(c->bbox, box, sizeof box);
    c->k = 2;                    // node.cpp:163
    c->K = 3;                    // node.cpp:311
    c->gate = 20;                // grid.hpp:352
    c->cylinder_radius = 0.001;  // grid.hpp:36
    c->ball_radius = 0.015;      // grid.hpp:35
    c->z_clip_min = 0.28;        // node.cpp:92
    c->z_clip_max = 0.6;         // node.cpp:93
    c->device = 0;
}

const char* hfpf_last_error(const hfpf_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int hfpf_create(const hfpf_config* cfg, hfpf_handle** out)
{
    if (!cfg || !out) return fail(nullptr, HFPF_ERR_BAD_ARG, "hfpf_create: null argument");
    if (cfg->struct_size != sizeof(hfpf_config)) return fail(nullptr, HFPF_ERR_BAD_CONFIG, "hfpf_config.struct_size mismatch (ABI %d)", HFPF_ABI_VERSION);
    *out = nullptr;
    hfpf_handle* h = new hfpf_handle();
    h->cfg = *cfg;
    h->knobs = read_knobs();
    auto bail = [&](int rc) {
        g_create_error = h->err;
        for (void* p : h->allocs) (void)hipFree(p);
        for (DevBuf* b : h->bufs)
            if (b->p) (void)hipFree(b->p);
        if (h->h_ctr) (void)hipHostFree(h->h_ctr);
        if (h->h_log_ctr) (void)hipHostFree(h->h_log_ctr);
        if (h->mbox) (void)hipHostFree(h->mbox);
        if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
        for (hipStream_t cs : h->copy_more)
            if (cs) (void)hipStreamDestroy(cs);
        if (h->ev_ready) (void)hipEventDestroy(h->ev_ready);
        if (h->ev_front) (void)hipEventDestroy(h->ev_front);
        if (h->ev_replay) (void)hipEventDestroy(h->ev_replay);
        if (h->front_stream) (void)hipStreamDestroy(h->front_stream);
        if (h->stream) (void)hipStreamDestroy(h->stream);
        delete h;
        return rc;
    };
    int rc = setup_params(h);
    if (rc) return bail(rc);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return bail(fail(h, HFPF_ERR_HIP, "no HIP device available (%s); this engine has no CPU path", hipGetErrorString(e)));
    if (cfg->device < 0 || cfg->device >= ndev) return bail(fail(h, HFPF_ERR_BAD_CONFIG, "device %d out of range (%d devices)", cfg->device, ndev));
    if ((e = hipSetDevice(cfg->device)) != hipSuccess) return bail(fail(h, HFPF_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e)));
    if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) return bail(fail(h, HFPF_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)));
    if ((e = hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking)) != hipSuccess) return bail(fail(h, HFPF_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)));
    for (int k = 0; k + 1 < h->knobs.copy_streams; k++)
        if ((e = hipStreamCreateWithFlags(&h->copy_more[k], hipStreamNonBlocking)) != hipSuccess) return bail(fail(h, HFPF_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)));
    if ((e = hipStreamCreateWithFlags(&h->front_stream, hipStreamNonBlocking)) != hipSuccess) return bail(fail(h, HFPF_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)));
    if ((e = hipEventCreateWithFlags(&h->ev_ready, hipEventDisableTiming)) != hipSuccess || (e = hipEventCreateWithFlags(&h->ev_front, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&h->ev_replay, hipEventDisableTiming)) != hipSuccess)
        return bail(fail(h, HFPF_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(e)));
    if ((e = hipHostMalloc((void**)&h->h_ctr, C_COUNT * sizeof(unsigned long long), hipHostMallocDefault)) != hipSuccess)
        return bail(fail(h, HFPF_ERR_HIP, "hipHostMalloc: %s", hipGetErrorString(e)));
    memset(h->h_ctr, 0, C_COUNT * sizeof(unsigned long long));
    if ((e = hipHostMalloc((void**)&h->h_log_ctr, kLogRegions * 16 * sizeof(unsigned long long), hipHostMallocDefault)) != hipSuccess)
        return bail(fail(h, HFPF_ERR_HIP, "hipHostMalloc: %s", hipGetErrorString(e)));
    memset(h->h_log_ctr, 0, kLogRegions * 16 * sizeof(unsigned long long));
    if (h->knobs.mailbox) {
        if ((e = hipHostMalloc((void**)&h->mbox, 2 * kMboxSlotWords * sizeof(unsigned long long), hipHostMallocCoherent | hipHostMallocMapped)) != hipSuccess)
            return bail(fail(h, HFPF_ERR_HIP, "hipHostMalloc (mailbox): %s", hipGetErrorString(e)));
        memset(h->mbox, 0, 2 * kMboxSlotWords * sizeof(unsigned long long));
    }
    {
        int per_cu = 0, cus = 0;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess) cus = prop.multiProcessorCount;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, h->binned ? k_integrate<true, false, true> : k_integrate<true, false, false>, 256, 0) != hipSuccess) per_cu = 4;
        h->integrate_grid = std::max(1, per_cu) * std::max(1, cus);
        h->compute_units = std::max(1, cus);
    }
    if ((rc = alloc_tables(h))) return bail(rc);
    {
        // Work buffers that would otherwise grow on first use are sized here like the pools: the clean
        // passes' key / value / sort scratch from max_normals, the per-call brick bins from max_call_points when given.
        const uint64_t n0 = h->cfg.max_normals;
        if ((rc = scratch(h, h->keys_a, n0 * 8)) || (rc = scratch(h, h->keys_b, n0 * 8)) || (rc = scratch(h, h->vals_a, n0 * 4)) ||
            (rc = scratch(h, h->vals_b, n0 * 4)) || (rc = scratch(h, h->pend_b, n0 * 4)) || (rc = scratch(h, h->sort_tmp, n0 * 16)))
            return bail(rc);
        if (h->cfg.max_call_points && h->binned) {
            const uint64_t pts = h->cfg.max_call_points;
            const uint64_t pool = std::min<uint64_t>(bin_pool_entries(h->knobs.bin_slack, pts, h->cfg.max_bricks), 0xFFFFFFFFull);
            if ((rc = scratch(h, h->bin_pt_buf, pool * sizeof(float4)))) return bail(rc);
            if (h->t.color && (rc = scratch(h, h->bin_rgb_buf, pool * 4))) return bail(rc);
            h->bin_pool = pool;
            if ((rc = scratch(h, h->ovf_pt_buf, pts * sizeof(float4))) || (rc = scratch(h, h->ovf_aux_buf, pts * sizeof(uint2)))) return bail(rc);
        }
    }
    for (int k = 0; k < 2; k++) {  // (a failure here only costs speed: extract then copies straight into pageable memory)
        if (hipHostMalloc(&h->xfer_pin[k], kXferChunk, hipHostMallocDefault) != hipSuccess || hipEventCreateWithFlags(&h->xfer_ev[k], hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            if (h->xfer_pin[0]) (void)hipHostFree(h->xfer_pin[0]);
            h->xfer_pin[0] = nullptr;
            break;
        }
    }
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return bail(fail(h, HFPF_ERR_HIP, "sync after init: %s", hipGetErrorString(e)));
    *out = h;
    return HFPF_OK;
}

int hfpf_destroy(hfpf_handle* h)
{
    if (!h) return HFPF_OK;
    (void)hipSetDevice(h->cfg.device);
    (void)hipStreamSynchronize(h->stream);
    if (h->front_stream) (void)hipStreamSynchronize(h->front_stream);
    for (void* p : h->allocs) (void)hipFree(p);
    for (DevBuf* b : h->bufs)
        if (b->p) (void)hipFree(b->p);
    if (h->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy((ncclComm_t_)h->comm);
    if (h->h_counts) (void)hipHostFree(h->h_counts);
    for (auto& s : h->stage) {
        if (s.h_pose) (void)hipHostFree(s.h_pose);
        if (s.d_pose) (void)hipFree(s.d_pose);
        if (s.done) (void)hipEventDestroy(s.done);
    }
    delete h->stage_pool;
    h->stage_pool = nullptr;
    for (int k = 0; k < 2; k++) {
        if (h->xfer_pin[k]) (void)hipHostFree(h->xfer_pin[k]);
        if (h->xfer_ev[k]) (void)hipEventDestroy(h->xfer_ev[k]);
    }
    for (auto& f : h->fslot) {
        if (f.h) (void)hipHostFree(f.h);
        if (f.done) (void)hipEventDestroy(f.done);
        if (f.copied) (void)hipEventDestroy(f.copied);
    }
    if (h->ring_d) (void)hipFree(h->ring_d);
    if (h->busy_ev) (void)hipEventDestroy(h->busy_ev);
    if (h->copy_stream) {
        (void)hipStreamSynchronize(h->copy_stream);
        (void)hipStreamDestroy(h->copy_stream);
    }
    for (hipStream_t cs : h->copy_more)
        if (cs) {
            (void)hipStreamSynchronize(cs);
            (void)hipStreamDestroy(cs);
        }
    for (TimedId& t : h->timed)
        for (auto& pr : t.pending) {
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
    for (auto e : h->ev_detail) (void)hipEventDestroy(e);
    for (auto e : h->ev_free) (void)hipEventDestroy(e);
    if (h->h_ctr) (void)hipHostFree(h->h_ctr);
    if (h->h_log_ctr) (void)hipHostFree(h->h_log_ctr);
    if (h->mbox) (void)hipHostFree(h->mbox);
    if (h->ev_ready) (void)hipEventDestroy(h->ev_ready);
    if (h->ev_front) (void)hipEventDestroy(h->ev_front);
    if (h->ev_replay) (void)hipEventDestroy(h->ev_replay);
    if (h->front_stream) (void)hipStreamDestroy(h->front_stream);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return HFPF_OK;
}

int hfpf_get_dims(const hfpf_handle* h, int32_t dims[3], double* resolution)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    if (dims) memcpy(dims, h->g.dim, 3 * sizeof(int32_t));
    if (resolution) *resolution = h->g.res;
    return HFPF_OK;
}

static int flush_pending_locked(hfpf_handle* h);

int hfpf_integrate_device(hfpf_handle* h, const void* dev_base, uint32_t n_frames, uint64_t frame_stride, uint32_t n_points, uint32_t point_step,
                          uint32_t off_x, uint32_t off_y, uint32_t off_z, uint32_t off_rgb, const double* poses, const uint32_t* frame_ids)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rcf = flush_pending_locked(h)) return rcf;  // host frames still waiting for their launch
    if (int rc = check_usable(h)) return rc;
    return integrate_device_locked(h, dev_base, n_frames, frame_stride, n_points, point_step, off_x, off_y, off_z, off_rgb, poses, frame_ids);
}

// Large host-to-host copies (the bounce copy of hfpf_integrate, the row download of extract) are split over the caller and the
// helper threads of the handle's StagePool (Knobs::stage_threads).
static void host_copy(hfpf_handle* h, void* dst, const void* src, size_t bytes)
{
    if (h->knobs.stage_threads > 0 && bytes >= (1u << 20)) {
        if (!h->stage_pool) h->stage_pool = new StagePool(h->knobs.stage_threads);
        h->stage_pool->copy(dst, src, bytes);
    } else {
        stream_copy((char*)dst, (const char*)src, bytes);
    }
}

// Hand the uploaded-but-not-launched host frames to the kernels: one integrate launch for the batch.
static int flush_pending_locked(hfpf_handle* h)
{
    if (h->ss.pend_n == 0) return HFPF_OK;
    const uint32_t first = h->ss.pend_first, n = h->ss.pend_n;
    h->ss.pend_n = 0;
    // the handle refuses work until hfpf_clear: frames accepted before the failure surfaced are dropped, and the caller is told
    if (h->ss.poisoned) return fail(h, HFPF_ERR_STATE, "%u accepted host frame(s) dropped: handle failed earlier (%s); hfpf_clear resets it", n, h->ss.poison_msg.c_str());
    // The slots of a batch alternate over the copy streams (slot % knobs.copy_streams): the kernels wait for the LAST upload of every
    // stream that carried one of them -- a stream is in order, so its earlier uploads are done too.  (f.done, recorded behind the
    // kernels below, then also means "this slot's upload has left its pinned bounce buffer".)
    for (uint32_t k = n, seen = 0; k-- > 0;) {
        const uint32_t which = (first + k) % (uint32_t)h->knobs.copy_streams;
        if (seen & (1u << which)) continue;
        seen |= 1u << which;
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->fslot[first + k].copied, 0));
    }
    const char* ring = (const char*)h->ring_d + (size_t)first * h->ring_cap;
    const DepthLayout dl = depth_layout(h->ss.pend_ds, ring + h->ss.pend_ds.color_off, h->ring_cap);
    int rc = integrate_device_locked(h, ring, n, h->ring_cap, h->ss.pend_pts, h->ss.pend_lay[0], h->ss.pend_lay[1], h->ss.pend_lay[2], h->ss.pend_lay[3],
                                     h->ss.pend_lay[4], h->ss.pend_pose, nullptr, h->ss.pend_depth ? &dl : nullptr);
    // frames that were accepted with HFPF_OK are lost: whichever entry point found them waiting, the handle stops until hfpf_clear
    if (rc) return poison_on_error(h, rc);
    for (uint32_t k = 0; k < n; k++) {
        FrameSlot& f = h->fslot[first + k];
        HIPCHK(h, hipEventRecord(f.done, h->stream));
        f.pending = true;
    }
    if (!h->busy_ev) HIPCHK(h, hipEventCreateWithFlags(&h->busy_ev, hipEventDisableTiming));
    HIPCHK(h, hipEventRecord(h->busy_ev, h->stream));
    h->busy_pending = true;
    return HFPF_OK;
}

// What a call that reads the fused model does first: select the device, launch the host frames still waiting (a failure there
// poisons the handle), refuse a failed handle, read the counters, surface deferred device errors (which poison it too).  Used by
// extract_filtered, snapshot and -- behind their refusal of distributed handles -- render, track, query, raycast and mesh.
// Entry points whose sequence DIFFERS keep their own, because aligning them would change what a failed handle returns:
// hfpf_extract_with_stats (no usability check, no poisoning), hfpf_sync (no usability check; only its error check poisons),
// hfpf_get_counters and hfpf_get_occupied (flush and read-back only), hfpf_stats_export (its flush does not poison),
// hfpf_epoch_export (no poisoning), hfpf_epoch_import* (flush only; the gathered form adds the usability check).
static int read_prologue_locked(hfpf_handle* h)
{
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc = poison_on_error(h, flush_pending_locked(h));
    if (!rc) rc = check_usable(h);
    if (!rc) rc = read_counters(h);
    if (!rc) rc = poison_on_error(h, check_device_errors(h));
    return rc;
}

// One host frame: upload on the copy stream into the next slot of the device ring; launch it -- together with the frames still
// waiting in front of it -- when the engine's stream is idle or the batch is full, otherwise leave it pending (the next frame,
// or any other call on the handle, launches it).  The upload of frame k+1 overlaps the kernels of frame k; `bounce` = copy the
// caller's (pageable) buffer into the slot's pinned buffer first, so that the caller's memory is free again when the call returns.
// ds != nullptr: a depth frame (validated by depth_spec): `base` is its depth image, `color` its colour image (or nullptr), both go
// into the slot (colour at ds->color_off), n_points = width * height, the cloud layout is unused.
static int integrate_host_locked(hfpf_handle* h, const void* base, bool bounce, uint32_t n_points, uint32_t point_step, uint32_t off_x,
                                 uint32_t off_y, uint32_t off_z, uint32_t off_rgb, const double pose[12], const DepthSpec* ds = nullptr,
                                 const void* color = nullptr)
{
    if (!base || !pose) return fail(h, HFPF_ERR_BAD_ARG, "integrate: null buffer or pose");
    if (int rc0 = check_usable(h)) return rc0;
    int rc;
    if (n_points == 0 && !ds) {
        if ((rc = flush_pending_locked(h))) return rc;  // frame ids stay in arrival order
        h->ss.next_frame_id++;
        h->frames_integrated++;
        h->ss.dirty = true;
        return HFPF_OK;
    }
    if (!ds && (rc = check_cloud_layout(h, "integrate", FrameLayout{point_step, off_x, off_y, off_z, off_rgb}, true))) return rc;
    const uint32_t lay[5] = {ds ? 0u : point_step, ds ? 0u : off_x, ds ? 0u : off_y, ds ? 0u : off_z, ds ? 0u : off_rgb};
    const size_t bytes = ds ? (ds->color_bpp ? ds->color_off + ds->color_bytes() : ds->depth_bytes()) : (size_t)n_points * point_step;
    // a frame of another kind or shape (depth frames: size, formats, intrinsics), or a slot that is not the batch's neighbour
    // (ring wrap), closes the pending batch
    const bool kind_differs = h->ss.pend_depth != (ds != nullptr) || (ds && memcmp(&h->ss.pend_ds, ds, sizeof *ds) != 0);
    if (h->ss.pend_n && (kind_differs || h->ss.pend_pts != n_points || memcmp(h->ss.pend_lay, lay, sizeof lay) != 0 ||
                      (uint32_t)h->fslot_next != h->ss.pend_first + h->ss.pend_n)) {
        if ((rc = flush_pending_locked(h))) return rc;
    }
    if (h->ring_cap < bytes) {  // (re)size the ring: nothing may be in flight in it
        if ((rc = flush_pending_locked(h))) return rc;
        HIPCHK(h, sync_copy_streams(h));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (auto& f : h->fslot) f.pending = false;
        if (h->ring_d) {
            HIPCHK(h, hipFree(h->ring_d));
            h->device_bytes -= h->ring_cap * kFrameSlots;
        }
        h->ring_d = nullptr;
        h->ring_cap = 0;
        const size_t cap = (bytes + 4095) & ~(size_t)4095;
        HIPCHK(h, hipMalloc(&h->ring_d, cap * kFrameSlots));
        h->ring_cap = cap;
        h->device_bytes += cap * kFrameSlots;
        h->fslot_next = 0;
    }
    const uint32_t slot = (uint32_t)h->fslot_next;
    FrameSlot& f = h->fslot[slot];
    h->fslot_next = (h->fslot_next + 1) % kFrameSlots;
    if (f.pending) {  // the kernels that read this slot (kFrameSlots frames ago)
        HIPCHK(h, hipEventSynchronize(f.done));
        f.pending = false;
    }
    if (!f.done) HIPCHK(h, hipEventCreateWithFlags(&f.done, hipEventDisableTiming));
    if (!f.copied) HIPCHK(h, hipEventCreateWithFlags(&f.copied, hipEventDisableTiming));
    const void* src = base;
    if (bounce) {
        if (f.cap_h < bytes) {
            if (f.h) HIPCHK(h, hipHostFree(f.h));
            f.h = nullptr;
            HIPCHK(h, hipHostMalloc(&f.h, h->ring_cap, hipHostMallocDefault));
            f.cap_h = h->ring_cap;
        }
        // the caller's buffer is free again when this call returns
        if (ds) {  // depth image, then the colour image at its offset (the gap between them is uploaded but never read)
            host_copy(h, f.h, base, ds->depth_bytes());
            if (ds->color_bpp) host_copy(h, (char*)f.h + ds->color_off, color, ds->color_bytes());
        } else {
            host_copy(h, f.h, base, bytes);
        }
        src = f.h;
    }
    const uint32_t which = slot % (uint32_t)h->knobs.copy_streams;
    hipStream_t cs = which ? h->copy_more[which - 1] : h->copy_stream;
    char* dst = (char*)h->ring_d + (size_t)slot * h->ring_cap;
    if (ds && !bounce) {  // two page-locked buffers of the caller: two uploads
        HIPCHK(h, hipMemcpyAsync(dst, base, ds->depth_bytes(), hipMemcpyHostToDevice, cs));
        if (ds->color_bpp) HIPCHK(h, hipMemcpyAsync(dst + ds->color_off, color, ds->color_bytes(), hipMemcpyHostToDevice, cs));
    } else {
        HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, cs));
    }
    HIPCHK(h, hipEventRecord(f.copied, cs));
    if (h->ss.pend_n == 0) {
        h->ss.pend_first = slot;
        h->ss.pend_pts = n_points;
        memcpy(h->ss.pend_lay, lay, sizeof lay);
        h->ss.pend_depth = ds != nullptr;
        if (ds) h->ss.pend_ds = *ds;
    }
    memcpy(h->ss.pend_pose + 12 * h->ss.pend_n, pose, 12 * sizeof(double));
    h->ss.pend_n++;
    h->ss.dirty = true;  // state_changed = true, grid.hpp:189 (the frame is accepted; its kernels follow)
    bool launch = h->ss.pend_n >= (uint32_t)std::max(1, h->knobs.host_batch) || h->fslot_next == 0;  // batch full, or the ring wraps next
    if (!launch) {
        if (!h->busy_pending) {
            launch = true;
        } else {
            const hipError_t q = hipEventQuery(h->busy_ev);
            if (q == hipSuccess) h->busy_pending = false, launch = true;
            else if (q != hipErrorNotReady) HIPCHK(h, q);
        }
    }
    return launch ? flush_pending_locked(h) : HFPF_OK;
}

int hfpf_integrate(hfpf_handle* h, const void* base, uint32_t n_points, uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z,
                   uint32_t off_rgb, const double pose[12])
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return integrate_host_locked(h, base, true, n_points, point_step, off_x, off_y, off_z, off_rgb, pose);
}

int hfpf_integrate_pinned(hfpf_handle* h, const void* pinned_base, uint32_t n_points, uint32_t point_step, uint32_t off_x, uint32_t off_y,
                          uint32_t off_z, uint32_t off_rgb, const double pose[12])
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (pinned_base) {
        hipPointerAttribute_t attr;
        const hipError_t e = hipPointerGetAttributes(&attr, pinned_base);
        if (e != hipSuccess || attr.type != hipMemoryTypeHost) {
            (void)hipGetLastError();
            return fail(h, HFPF_ERR_BAD_ARG, "integrate_pinned: the buffer is not page-locked host memory (hfpf_host_alloc / hipHostRegister); use hfpf_integrate");
        }
    }
    return integrate_host_locked(h, pinned_base, false, n_points, point_step, off_x, off_y, off_z, off_rgb, pose);
}

// hfpf_depth_image -> DepthSpec, with every check include/hfpf.h lists (HFPF_ERR_BAD_ARG; nothing on the handle changes).
static int depth_spec(hfpf_handle* h, const hfpf_depth_image* d, const void* depth, const void* color, DepthSpec* out)
{
    if (!d) return fail(h, HFPF_ERR_BAD_ARG, "depth image: null descriptor");
    if (d->struct_size != sizeof(hfpf_depth_image) || d->reserved != 0)
        return fail(h, HFPF_ERR_BAD_ARG, "depth image: struct_size must be %zu and reserved 0", sizeof(hfpf_depth_image));
    if (!depth) return fail(h, HFPF_ERR_BAD_ARG, "depth image: null depth buffer");
    const uint64_t n = (uint64_t)d->width * d->height;
    if (n == 0 || n > (1ull << 31)) return fail(h, HFPF_ERR_BAD_ARG, "depth image: %u x %u pixels", d->width, d->height);
    uint32_t dbpp = 0, cbpp = 0;
    if (d->depth_format == HFPF_DEPTH_U16) dbpp = 2;
    else if (d->depth_format == HFPF_DEPTH_F32) dbpp = 4;
    else return fail(h, HFPF_ERR_BAD_ARG, "depth image: unknown depth_format %u", d->depth_format);
    if (d->color_format == HFPF_COLOR_RGB8 || d->color_format == HFPF_COLOR_BGR8) cbpp = 3;
    else if (d->color_format == HFPF_COLOR_RGBA8 || d->color_format == HFPF_COLOR_BGRA8) cbpp = 4;
    else if (d->color_format != HFPF_COLOR_NONE) return fail(h, HFPF_ERR_BAD_ARG, "depth image: unknown color_format %u", d->color_format);
    if ((uint64_t)d->depth_step < (uint64_t)d->width * dbpp || d->depth_step % dbpp)
        return fail(h, HFPF_ERR_BAD_ARG, "depth image: depth_step %u (width %u, %u-byte samples)", d->depth_step, d->width, dbpp);
    if (cbpp && ((uint64_t)d->color_step < (uint64_t)d->width * cbpp || (cbpp == 4 && d->color_step % 4)))
        return fail(h, HFPF_ERR_BAD_ARG, "depth image: color_step %u (width %u, %u bytes per pixel)", d->color_step, d->width, cbpp);
    if (!cbpp && color) return fail(h, HFPF_ERR_BAD_ARG, "depth image: a colour buffer given with HFPF_COLOR_NONE");
    if (cbpp && !color) return fail(h, HFPF_ERR_BAD_ARG, "depth image: null colour buffer for color_format %u", d->color_format);
    if (!(std::isfinite(d->fx) && d->fx > 0) || !(std::isfinite(d->fy) && d->fy > 0) || !std::isfinite(d->cx) || !std::isfinite(d->cy))
        return fail(h, HFPF_ERR_BAD_ARG, "depth image: intrinsics fx %g fy %g cx %g cy %g", d->fx, d->fy, d->cx, d->cy);
    const bool f32 = d->depth_format == HFPF_DEPTH_F32;
    if (!f32 && !(std::isfinite(d->depth_scale) && d->depth_scale > 0))
        return fail(h, HFPF_ERR_BAD_ARG, "depth image: depth_scale %g", (double)d->depth_scale);
    DepthSpec ds{};
    ds.width = d->width;
    ds.height = d->height;
    ds.depth_f32 = f32 ? 1u : 0u;
    ds.depth_step = d->depth_step;
    ds.color_bpp = cbpp;
    ds.color_bgr = (d->color_format == HFPF_COLOR_BGR8 || d->color_format == HFPF_COLOR_BGRA8) ? 1u : 0u;
    ds.color_step = cbpp ? d->color_step : 0u;
    // the rounding of the contract (include/hfpf.h): each constant from its double, once, here
    ds.cx = (float)d->cx;
    ds.cy = (float)d->cy;
    ds.unit = f32 ? 1.0f : d->depth_scale;
    ds.sx = f32 ? (float)(1.0 / d->fx) : (float)((double)d->depth_scale / d->fx);
    ds.sy = f32 ? (float)(1.0 / d->fy) : (float)((double)d->depth_scale / d->fy);
    const size_t coff = cbpp ? (ds.depth_bytes() + 255) & ~(size_t)255 : 0;
    if (coff > 0xFFFFFFFFull) return fail(h, HFPF_ERR_BAD_ARG, "depth image: %zu bytes", ds.depth_bytes());
    ds.color_off = (uint32_t)coff;
    *out = ds;
    return HFPF_OK;
}

static bool is_pinned_host(const void* p)
{
    hipPointerAttribute_t attr;
    const hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess && attr.type == hipMemoryTypeHost;
}

int hfpf_integrate_depth(hfpf_handle* h, const hfpf_depth_image* desc, const void* depth, const void* color, const double pose[12])
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DepthSpec ds;
    if (int rc = depth_spec(h, desc, depth, color, &ds)) return rc;
    return integrate_host_locked(h, depth, true, ds.width * ds.height, 0, 0, 0, 0, 0, pose, &ds, color);
}

int hfpf_integrate_depth_pinned(hfpf_handle* h, const hfpf_depth_image* desc, const void* depth, const void* color, const double pose[12])
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DepthSpec ds;
    if (int rc = depth_spec(h, desc, depth, color, &ds)) return rc;
    if (!is_pinned_host(depth) || (color && !is_pinned_host(color)))
        return fail(h, HFPF_ERR_BAD_ARG, "integrate_depth_pinned: an image is not page-locked host memory (hfpf_host_alloc / hipHostRegister); use hfpf_integrate_depth");
    return integrate_host_locked(h, depth, false, ds.width * ds.height, 0, 0, 0, 0, 0, pose, &ds, color);
}

int hfpf_integrate_depth_device(hfpf_handle* h, const hfpf_depth_image* desc, const void* dev_depth, uint64_t depth_frame_stride, const void* dev_color,
                                uint64_t color_frame_stride, uint32_t n_frames, const double* poses, const uint32_t* frame_ids)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DepthSpec ds;
    if (int rc = depth_spec(h, desc, dev_depth, dev_color, &ds)) return rc;
    const uint32_t dbpp = ds.depth_f32 ? 4u : 2u, calign = ds.color_bpp == 4 ? 4u : 1u;
    if ((uintptr_t)dev_depth % dbpp || depth_frame_stride % dbpp || (uintptr_t)dev_color % calign || color_frame_stride % calign)
        return fail(h, HFPF_ERR_BAD_ARG, "integrate_depth_device: images and frame strides must be aligned to the sample size");
    if (n_frames > 1 && (depth_frame_stride < ds.depth_bytes() || (ds.color_bpp && color_frame_stride < ds.color_bytes())))
        return fail(h, HFPF_ERR_BAD_ARG, "integrate_depth_device: frame stride below the image size");
    if (int rcf = flush_pending_locked(h)) return rcf;  // host frames still waiting for their launch
    if (int rc = check_usable(h)) return rc;
    const DepthLayout dl = depth_layout(ds, dev_color, color_frame_stride);
    return integrate_device_locked(h, dev_depth, n_frames, depth_frame_stride, ds.width * ds.height, 0, 0, 0, 0, 0, poses, frame_ids, &dl);
}

int hfpf_host_alloc(hfpf_handle* h, uint64_t bytes, void** host_ptr)
{
    if (!h || !host_ptr) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipHostMalloc(host_ptr, (size_t)std::max<uint64_t>(bytes, 1), hipHostMallocDefault));
    return HFPF_OK;
}

int hfpf_host_free(hfpf_handle* h, void* host_ptr)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rcf = flush_pending_locked(h)) return rcf;  // host frames still waiting for their launch
    HIPCHK(h, sync_copy_streams(h));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipHostFree(host_ptr));
    return HFPF_OK;
}

int hfpf_is_dirty(hfpf_handle* h)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    return h->ss.dirty ? 1 : 0;
}

int hfpf_clean(hfpf_handle* h)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    // Everything that can fail in front of the collectives of a distributed clean is folded into `pre`: a rank whose device
    // cannot be selected or whose deferred host-frame launch fails (scratch allocation, frame id >= max_frames, HIP error) still
    // enters the status gather of clean_locked, so its peers leave with HFPF_ERR_DIST instead of waiting in ncclAllGather for ever.
    int pre = HFPF_OK;
    if (hipError_t e_ = hipSetDevice(h->cfg.device)) pre = fail(h, HFPF_ERR_HIP, "hipSetDevice failed: %s", hipGetErrorString(e_));
    if (!pre) pre = poison_on_error(h, flush_pending_locked(h));  // host frames still waiting for their launch
    if (!pre) pre = check_usable(h);
    if (pre && !h->dist_on) return pre;
    if (pre) return poison_on_error(h, clean_locked(h, pre));
    Timed timed(h);  // after every queued integrate: measures the clean pass alone (nothing with timing off)
    if (timed.rc) return timed.rc;
    const int rc = poison_on_error(h, clean_locked(h, 0));
    if (int rc1 = timed.file(kTimeClean)) return rc1;
    return rc;
}

// The row set of a read-out.  rows live in h->rows_dev.  record_of_row (row -> id of its normal record) lives in h->vals_b, the
// output of the row sort: it is dead as soon as the caller sorts through the handle's sort buffers (keys_a/b, vals_a/b) again.
struct RowSet {
    const Row* rows = nullptr;
    const uint32_t* record_of_row = nullptr;
    uint64_t n = 0;
};

// First half of extract (and of a render): the row set of `opt` built on the device, row j = the j-th in lexicographic (x, y, z)
// order.  `stats` are the (possibly merged) sums to finalise.
static int build_rows_locked(hfpf_handle* h, const unsigned long long* stats, const ExtractOpts& opt, RowSet* out)
{
    Tables& t = h->t;
    int rc;
    *out = RowSet{};
    const uint64_t n = h->h_ctr[C_NORMALS];
    if (n == 0) return HFPF_OK;
    uint64_t *keys_in, *keys_out; if ((rc = scratch_n(h, h->keys_a, n, &keys_in)) || (rc = scratch_n(h, h->keys_b, n, &keys_out))) return rc;
    uint32_t *vals_in, *vals_out; if ((rc = scratch_n(h, h->vals_a, n, &vals_in)) || (rc = scratch_n(h, h->vals_b, n, &vals_out))) return rc;
    hipLaunchKernelGGL(k_set_ctr, dim3(1), dim3(1), 0, h->stream, t.ctr, (int)C_ROWS, 0ull);
    hipLaunchKernelGGL(k_extract_keys, dim3(blocks_for(n, 256 * kExtractTiles)), dim3(256), 0, h->stream, h->g, t, stats, n, opt, keys_in, vals_in);
    HIPCHK(h, hipGetLastError());
    if ((rc = sort_pairs_u64(h, keys_in, keys_out, vals_in, vals_out, n))) return rc;
    if ((rc = read_counters(h))) return rc;
    const uint64_t nr = h->h_ctr[C_ROWS];
    if (nr == 0) return HFPF_OK;
    Row* rows; if ((rc = scratch_n(h, h->rows_dev, nr, &rows))) return rc;
    hipLaunchKernelGGL(k_extract_rows, dim3(blocks_for(nr, 256)), dim3(256), 0, h->stream, h->g, t, stats, nr, opt, keys_out, vals_out, rows);
    HIPCHK(h, hipGetLastError());
    *out = RowSet{rows, vals_out, nr};
    return HFPF_OK;
}

// Device -> pageable host copy, complete on return.  A direct device-to-pageable copy runs at ~10 GB/s through the runtime's own
// staging.  Copies of at least `pinned_from` bytes go through the two pinned 16 MB buffers instead: chunk i+1 crosses the link while
// chunk i is copied out by the caller and the helper threads.
static hipError_t download_pageable(hfpf_handle* h, void* host, const void* dev, size_t total, size_t pinned_from = 2 * kXferChunk)
{
    hipError_t e = hipSuccess;
    if (h->xfer_pin[0] && total >= pinned_from) {
        const size_t n_chunks = (total + kXferChunk - 1) / kXferChunk;
        auto issue = [&](size_t i) -> hipError_t {
            const size_t off = i * kXferChunk, len = std::min(kXferChunk, total - off);
            const hipError_t r = hipMemcpyAsync(h->xfer_pin[i & 1], (const char*)dev + off, len, hipMemcpyDeviceToHost, h->stream);
            return r != hipSuccess ? r : hipEventRecord(h->xfer_ev[i & 1], h->stream);
        };
        e = issue(0);
        if (e == hipSuccess && n_chunks > 1) e = issue(1);
        for (size_t i = 0; i < n_chunks && e == hipSuccess; i++) {
            const size_t off = i * kXferChunk, len = std::min(kXferChunk, total - off);
            e = hipEventSynchronize(h->xfer_ev[i & 1]);
            if (e != hipSuccess) break;
            host_copy(h, (char*)host + off, h->xfer_pin[i & 1], len);
            if (i + 2 < n_chunks) e = issue(i + 2);  // this buffer is free again
        }
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    } else {
        e = hipMemcpyAsync(host, dev, total, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    }
    return e;
}

// A result array the caller will free(): 2 MB-aligned and advised as huge pages from 4 MB on (a fresh 125 MB result is then ~60 page
// faults instead of 30,000 while it is filled), plain malloc below.
static void* host_result_alloc(size_t want)
{
    void* mem = nullptr;
    const size_t huge = (want + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1);
    if (want >= (4u << 20) && posix_memalign(&mem, 2u << 20, huge) == 0) {
        (void)madvise(mem, huge, MADV_HUGEPAGE);
        return mem;
    }
    return malloc(want);
}

// The arrays a read-out returns, up to kResultArrays (four: hfpf_mesh_topology).  result_alloc gives each a device array;
// the kernels fill them; result_deliver hands them to the caller of the device form and downloads them for the host form's.
constexpr int kResultArrays = 4;
struct ResultSet {
    struct Array {
        size_t bytes = 0;
        bool absent = false;           // an optional output the caller passed NULL for: no memory, NULL wherever it would appear
        const void* borrow = nullptr;  // device memory of the handle that already holds the array: the host form downloads from it
        void* dev = nullptr;           // the device array (result_alloc)
    };
    Array a[kResultArrays];
    int n = 0;
    bool owned = false;  // device form: the arrays are allocations of their own, and this set frees them unless it hands them over
    ResultSet() = default;
    ResultSet(const ResultSet&) = delete;
    ResultSet& operator=(const ResultSet&) = delete;
    ~ResultSet()  // every error exit behind result_alloc
    {
        for (Array& x : a)
            if (owned && x.dev) (void)hipFree(x.dev);
    }
    void add(size_t bytes, bool absent = false, const void* borrow = nullptr) { a[n++] = Array{bytes, absent, borrow, nullptr}; }
    void keep(ResultSet* to)  // the success exit: the arrays go to *to, which describes them and frees nothing
    {
        for (int i = 0; i < kResultArrays; i++) to->a[i] = a[i];
        to->n = n;
        owned = false;
    }
};

// Device form: one hipMalloc per present array (a borrowed one too: the caller copies it over).  Host form: 16-byte aligned slices of
// h->result_out, and borrowed arrays where they are.
static int result_alloc(hfpf_handle* h, ResultSet& set, bool on_device, const char* what)
{
    set.owned = on_device;
    if (on_device) {
        for (int i = 0; i < set.n; i++) {
            if (set.a[i].absent) continue;
            const hipError_t e = hipMalloc(&set.a[i].dev, set.a[i].bytes);
            if (e == hipSuccess) continue;
            return fail(h, HFPF_ERR_HIP, "%s: device allocation of %llu bytes failed: %s", what, (unsigned long long)set.a[i].bytes, hipGetErrorString(e));
        }
        return HFPF_OK;
    }
    ScratchLayout lay;
    uint8_t* slice[kResultArrays] = {};
    for (int i = 0; i < set.n; i++)
        if (!set.a[i].absent && !set.a[i].borrow) lay.add(&slice[i], set.a[i].bytes, 16);
    if (lay.bytes())
        if (int rc = scratch(h, h->result_out, lay)) return rc;
    for (int i = 0; i < set.n; i++)
        if (!set.a[i].absent) set.a[i].dev = set.a[i].borrow ? const_cast<void*>(set.a[i].borrow) : slice[i];
    return HFPF_OK;
}

// The host form's tail: every present array into pageable memory the caller will free() (out[i]; NULL for an absent one).
static int result_to_host(hfpf_handle* h, const ResultSet& set, const char* what, void* out[kResultArrays])
{
    bool ok = true;
    for (int i = 0; i < kResultArrays; i++) {
        const bool present = i < set.n && !set.a[i].absent;
        out[i] = present ? host_result_alloc(set.a[i].bytes) : nullptr;
        ok = ok && (!present || out[i]);
    }
    hipError_t e = hipSuccess;
    for (int i = 0; i < set.n && ok && e == hipSuccess; i++)
        if (out[i]) e = download_pageable(h, out[i], set.a[i].dev, set.a[i].bytes);
    if (ok && e == hipSuccess) return HFPF_OK;
    for (int i = 0; i < kResultArrays; i++) {
        free(out[i]);
        out[i] = nullptr;
    }
    if (!ok) return fail(h, HFPF_ERR_CAPACITY, "%s: host allocation of the result failed", what);
    return fail(h, HFPF_ERR_HIP, "%s copy: %s", what, hipGetErrorString(e));
}

// The delivery of both forms, behind ResultSet::keep.  Device form: the device arrays themselves, now the caller's (out[i]; NULL for an
// absent or a never-added one).  Host form: result_to_host; an empty set downloads nothing and gives three NULLs.
static int result_deliver(hfpf_handle* h, const ResultSet& set, bool on_device, const char* what, void* out[kResultArrays])
{
    for (int i = 0; i < kResultArrays; i++) out[i] = on_device ? set.a[i].dev : nullptr;
    return on_device || set.n == 0 ? HFPF_OK : result_to_host(h, set, what, out);
}

// Shared tail of extract: `stats` are the (possibly merged) sums to finalise.
static int extract_locked(hfpf_handle* h, const unsigned long long* stats, const hfpf_extract_opts* o, hfpf_row** rows, uint64_t* n_rows)
{
    ExtractOpts opt{0.0, -1, 0};
    if (o) {
        opt.min_count = o->min_count;
        opt.classify_threshold = o->classify_threshold;
        opt.paint_white = o->paint_white ? 1 : 0;
    }
    RowSet rs;
    int rc;
    if ((rc = build_rows_locked(h, stats, opt, &rs))) return rc;
    if (rs.n == 0) return HFPF_OK;
    ResultSet set;
    set.add(rs.n * sizeof(Row), false, rs.rows);
    void* host[kResultArrays];
    if ((rc = result_alloc(h, set, false, "extract")) || (rc = result_to_host(h, set, "extract", host))) return rc;
    *rows = (hfpf_row*)host[0];
    *n_rows = rs.n;
    return HFPF_OK;
}

int hfpf_extract(hfpf_handle* h, hfpf_row** rows, uint64_t* n_rows) { return hfpf_extract_filtered(h, nullptr, rows, n_rows); }

int hfpf_extract_filtered(hfpf_handle* h, const hfpf_extract_opts* opts, hfpf_row** rows, uint64_t* n_rows)
{
    if (!h || !rows || !n_rows) return HFPF_ERR_BAD_ARG;
    if (opts && opts->struct_size != sizeof(hfpf_extract_opts)) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    *rows = nullptr;
    *n_rows = 0;
    Tables& t = h->t;
    // (as in hfpf_clean: a local failure in front of the collective travels through the status gather, it does not skip it)
    int rc = read_prologue_locked(h);
    if (rc && !h->dist_on) return rc;
    const unsigned long long* stats = t.stats;
    if (h->dist_on) {
        // Sum the ranks' private partial records (exact integer adds) into scratch; the partials stay intact.
        // Normal records are replicated, so every rank holds the same n and the same record ids -- checked: the count travels as
        // the payload of the status gather that makes every rank agree to enter the all-reduce (or to leave together).
        // The whole table is reduced, (n + 1) x 64 bytes = 125 MB at 2 M voxels: one collective per extract, a few ms over xGMI
        // against an extract that sorts and downloads the same records; a list of touched records would need a second collective.
        const uint64_t n_mine = h->h_ctr[C_NORMALS];
        const uint64_t words = (n_mine + 1) * kStatWords;
        unsigned long long* total = nullptr;
        if (!rc) rc = scratch_n(h, h->stats_total, words, &total);
        std::vector<unsigned long long> n_of(h->world, 0ull);
        if ((rc = dist_status_gather_locked(h, rc, n_mine, "statistics all-reduce of extract", n_of.data()))) return rc;
        for (int r = 0; r < h->world; r++)  // every rank sees the same payloads, so all of them take this exit or none does
            if (n_of[r] != n_of[0])
                return fail(h, HFPF_ERR_DIST, "rank %d holds %llu normal records, rank 0 %llu: the ranks did not run the same clean schedule", r,
                            (unsigned long long)n_of[r], (unsigned long long)n_of[0]);
        NCCLCHK(h, g_rccl.AllReduce(t.stats, total, words, ncclUint64_, ncclSum_, (ncclComm_t_)h->comm, h->stream));
        stats = total;
    }
    return extract_locked(h, stats, opts, rows, n_rows);
}

int hfpf_extract_with_stats(hfpf_handle* h, const void* dev_words, const void* dev_cwords, hfpf_row** rows, uint64_t* n_rows)
{
    if (!h || !rows || !n_rows || !dev_words) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rcf = flush_pending_locked(h)) return rcf;  // host frames still waiting for their launch
    *rows = nullptr;
    *n_rows = 0;
    int rc = read_counters(h);
    if (rc) return rc;
    if ((rc = check_device_errors(h))) return rc;
    (void)dev_cwords;  // colour sums travel in words 5-7 of the statistics records since ABI 3
    return extract_locked(h, (const unsigned long long*)dev_words, nullptr, rows, n_rows);
}

// ---- render (include/hfpf.h) ----------------------------------------------------------------------------------------------
static bool view_opts_ok(const hfpf_render_opts* o)
{
    if (!o || o->struct_size != sizeof(hfpf_render_opts) || o->reserved != 0) return false;
    if (o->flags & ~(HFPF_RENDER_CULL_BACKFACES | HFPF_RENDER_WORLD_NORMALS)) return false;
    const uint64_t wh = (uint64_t)o->width * o->height;
    if (wh == 0 || wh > (1ull << 31)) return false;
    if (!(std::isfinite(o->fx) && o->fx > 0.0 && std::isfinite(o->fy) && o->fy > 0.0 && std::isfinite(o->cx) && std::isfinite(o->cy))) return false;
    if (!(std::isfinite(o->z_near) && std::isfinite(o->z_far) && 0.0 < o->z_near && o->z_near < o->z_far)) return false;
    if (std::isnan(o->min_count)) return false;
    return !(o->splat_radius < -1 || o->splat_radius > 15 || o->max_splat_radius < 0 || o->max_splat_radius > 15);
}

static bool render_opts_ok(const hfpf_render_opts* o, const hfpf_render_planes* pl)
{
    return view_opts_ok(o) && pl && (pl->depth || pl->normal || pl->rgb || pl->count || pl->voxel);
}

// The read prologue of the calls that work on one GPU's model only.
static int local_read_prologue_locked(hfpf_handle* h, const char* what = "render")
{
    if (h->dist_on) return fail(h, HFPF_ERR_STATE, "%s: not available on a handle with an RCCL communicator (hfpf_dist_disable drops it)", what);
    return read_prologue_locked(h);
}

// The camera of view.hpp from the options of a view, and from a depth image with the z range of its call.
static Pinhole pinhole_of(const hfpf_render_opts& o) { return Pinhole{o.fx, o.fy, o.cx, o.cy, o.z_near, o.z_far, o.width, o.height}; }
static Pinhole pinhole_of(const hfpf_depth_image& d, double z_near, double z_far) { return Pinhole{d.fx, d.fy, d.cx, d.cy, z_near, z_far, d.width, d.height}; }

// Views per chunk of depth buffers with word_bytes a pixel: at most kRenderChunkViews (their poses sit in LDS) and kRenderZbufBytes
// of buffers, one view at least.
static uint32_t view_chunk(uint64_t WH, size_t word_bytes, uint32_t n_views)
{
    return (uint32_t)std::min<uint64_t>({(uint64_t)kRenderChunkViews, std::max<uint64_t>(1, kRenderZbufBytes / (word_bytes * WH)), std::max<uint32_t>(n_views, 1)});
}

// n poses (12 f64 each, host memory) into the scratch buffer `buf`, enqueued on the handle's stream.
static int upload_poses(hfpf_handle* h, DevBuf& buf, const double* poses, uint64_t n, double** pose_d)
{
    if (int rc = scratch_n(h, buf, 12ull * n, pose_d)) return rc;
    HIPCHK(h, hipMemcpyAsync(*pose_d, poses, (size_t)n * 12 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return HFPF_OK;
}

// The views of a render (or the model view of a track): the row set, the z-buffer scratch of one chunk of views, the poses on the
// device and the splat's parameters.
struct RenderViews {
    RowSet rows;
    unsigned long long* zbuf;  // per_chunk z-buffers
    double* pose_d;            // n_views poses
    uint32_t n_views, per_chunk;
    RenderParams p;
};
static int render_views_locked(hfpf_handle* h, const hfpf_render_opts* o, uint32_t n_views, const double* poses, RenderViews* rv)
{
    int rc;
    const ExtractOpts opt{std::max(1.0, o->min_count), -1, 0};  // count >= max(1, min_count), the compare of k_extract_keys
    if ((rc = build_rows_locked(h, h->t.stats, opt, &rv->rows))) return rc;
    const uint64_t nr = rv->rows.n;
    if (nr > 0xFFFFFFFFull) return fail(h, HFPF_ERR_CAPACITY, "render: %llu rows do not fit the 32-bit row field of a z-buffer word", (unsigned long long)nr);
    const uint64_t WH = (uint64_t)o->width * o->height;
    const uint32_t per_chunk = view_chunk(WH, sizeof *rv->zbuf, n_views);
    if ((rc = scratch_n(h, h->zbuf, per_chunk * WH, &rv->zbuf))) return rc;
    if ((rc = upload_poses(h, h->render_pose, poses, n_views, &rv->pose_d))) return rc;
    RenderParams& p = rv->p;
    p = RenderParams{};
    p.cam = pinhole_of(*o);
    p.cull = (o->flags & HFPF_RENDER_CULL_BACKFACES) ? 1u : 0u;
    p.world_normals = (o->flags & HFPF_RENDER_WORLD_NORMALS) ? 1u : 0u;
    p.radius = o->splat_radius;
    p.max_radius = o->max_splat_radius;
    p.r_num = (0.5 * h->g.res) * std::max(o->fx, o->fy);
    rv->n_views = n_views;
    rv->per_chunk = per_chunk;
    return HFPF_OK;
}

// The z-buffers of the chunk of views starting at v0, left in h->zbuf: all ones, then k_render_splat.  Sets rv->p.n_views.
static int render_splat_locked(hfpf_handle* h, RenderViews* rv, uint32_t v0)
{
    RenderParams& p = rv->p;
    p.n_views = std::min(rv->per_chunk, rv->n_views - v0);
    const uint64_t pix = p.n_views * (uint64_t)p.cam.width * p.cam.height;
    HIPCHK(h, hipMemsetAsync(rv->zbuf, 0xFF, pix * 8, h->stream));
    if (rv->rows.n)
        hipLaunchKernelGGL(k_render_splat, dim3(blocks_for(rv->rows.n, 256)), dim3(256), 0, h->stream, rv->rows.rows, (uint32_t)rv->rows.n,
                           rv->pose_d + 12ull * v0, p, rv->zbuf);
    HIPCHK(h, hipGetLastError());
    return HFPF_OK;
}

// The row set once, then per chunk of views: the z-buffers (render_splat_locked), k_render_resolve into the device planes.
static int render_locked(hfpf_handle* h, const hfpf_render_opts* o, uint32_t n_views, const double* poses, const hfpf_render_planes& dev)
{
    RenderViews rv;
    if (int rc = render_views_locked(h, o, n_views, poses, &rv)) return rc;
    const uint64_t WH = (uint64_t)o->width * o->height;
    for (uint32_t v0 = 0; v0 < n_views; v0 += rv.per_chunk) {
        if (int rc = render_splat_locked(h, &rv, v0)) return rc;
        const RenderParams& p = rv.p;
        const uint64_t pix = p.n_views * WH, off = v0 * WH;
        const RenderPlanes pl{dev.depth ? dev.depth + off : nullptr, dev.normal ? dev.normal + 3 * off : nullptr, dev.rgb ? dev.rgb + off : nullptr,
                              dev.count ? dev.count + off : nullptr, dev.voxel ? dev.voxel + 3 * off : nullptr};
        hipLaunchKernelGGL(k_render_resolve, dim3(blocks_for(pix, 256)), dim3(256), 0, h->stream, rv.rows.rows, rv.zbuf, rv.pose_d + 12ull * v0, p, pl);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HFPF_OK;
}

int hfpf_render_device(hfpf_handle* h, const hfpf_render_opts* o, uint32_t n_views, const double* poses, const hfpf_render_planes* dev_out)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    if (!render_opts_ok(o, dev_out)) return fail(h, HFPF_ERR_BAD_ARG, "render: invalid options or planes");
    if (n_views == 0) return HFPF_OK;
    if (!poses) return fail(h, HFPF_ERR_BAD_ARG, "render: NULL poses");
    if (int rc = local_read_prologue_locked(h)) return rc;
    return render_locked(h, o, n_views, poses, *dev_out);
}

int hfpf_render(hfpf_handle* h, const hfpf_render_opts* o, const double pose_3x4[12], const hfpf_render_planes* host_out)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    if (!render_opts_ok(o, host_out) || !pose_3x4) return fail(h, HFPF_ERR_BAD_ARG, "render: invalid options, pose or planes");
    if (int rc = local_read_prologue_locked(h)) return rc;
    // device planes, each 256-byte aligned, in one scratch buffer; then one download per requested plane
    const uint64_t WH = (uint64_t)o->width * o->height;
    void* host[5] = {host_out->depth, host_out->normal, host_out->rgb, host_out->count, host_out->voxel};
    const uint64_t bytes[5] = {4 * WH, 12 * WH, 4 * WH, 4 * WH, 12 * WH};
    hfpf_render_planes dev{};
    ScratchLayout lay;
    if (host[0]) lay.add(&dev.depth, WH, 256);
    if (host[1]) lay.add(&dev.normal, 3 * WH, 256);
    if (host[2]) lay.add(&dev.rgb, WH, 256);
    if (host[3]) lay.add(&dev.count, WH, 256);
    if (host[4]) lay.add(&dev.voxel, 3 * WH, 256);
    if (int rc = scratch(h, h->render_out, lay)) return rc;
    if (int rc = render_locked(h, o, 1, pose_3x4, dev)) return rc;
    const void* plane[5] = {dev.depth, dev.normal, dev.rgb, dev.count, dev.voxel};
    for (int k = 0; k < 5; k++) {
        if (!host[k]) continue;
        const hipError_t e = download_pageable(h, host[k], plane[k], bytes[k], 0);  // every plane through the pinned buffers
        if (e != hipSuccess) return fail(h, HFPF_ERR_HIP, "render copy: %s", hipGetErrorString(e));
    }
    return HFPF_OK;
}

// ---- pose tracking (include/hfpf.h) -------------------------------------------------------------------------------------
// The checks on the options of refine_pose that hfpf_track* and hfpf_align_mesh* both make (Opts is either call's), with the call's
// own stride limit.
extern "C++" template <typename Opts>
static bool refine_opts_ok(const Opts* o, uint32_t max_stride)
{
    if (o->max_iterations < 1 || o->max_iterations > 64 || o->stride < 1 || o->stride > max_stride || o->min_inliers < 6) return false;
    if (!(std::isfinite(o->damping) && o->damping >= 0.0)) return false;
    return std::isfinite(o->eps_rotation) && o->eps_rotation >= 0.0 && std::isfinite(o->eps_translation) && o->eps_translation >= 0.0;
}

static bool track_opts_ok(const hfpf_track_opts* o)
{
    if (!o || o->struct_size != sizeof(hfpf_track_opts) || o->reserved != 0) return false;
    if (!refine_opts_ok(o, 16)) return false;
    if (!(o->max_distance > 0.0 && o->max_distance <= 1.0)) return false;
    return view_opts_ok(&o->view);
}

// A 3x4 pose of 12 finite doubles.
static bool pose_ok(const double* pose)
{
    if (!pose) return false;
    for (int k = 0; k < 12; k++)
        if (!std::isfinite(pose[k])) return false;
    return true;
}

static bool track_args_ok(const double* pose, const hfpf_track_result* res)
{
    return res && res->struct_size == sizeof(hfpf_track_result) && pose_ok(pose);
}

// Pageable host -> device copy, complete on return: chunks through the two pinned 16 MB buffers (the mirror of download_pageable),
// or the runtime's own staging when they are missing.
static hipError_t upload_pageable(hfpf_handle* h, void* dev, const void* host, size_t total)
{
    hipError_t e = hipSuccess;
    if (!h->xfer_pin[0]) {
        e = hipMemcpyAsync(dev, host, total, hipMemcpyHostToDevice, h->stream);
        return e != hipSuccess ? e : hipStreamSynchronize(h->stream);
    }
    const size_t n_chunks = (total + kXferChunk - 1) / kXferChunk;
    for (size_t i = 0; i < n_chunks && e == hipSuccess; i++) {
        const size_t off = i * kXferChunk, len = std::min(kXferChunk, total - off);
        if (i >= 2) e = hipEventSynchronize(h->xfer_ev[i & 1]);  // the copy out of this buffer two chunks ago
        if (e != hipSuccess) break;
        host_copy(h, h->xfer_pin[i & 1], (const char*)host + off, len);
        e = hipMemcpyAsync((char*)dev + off, h->xfer_pin[i & 1], len, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipEventRecord(h->xfer_ev[i & 1], h->stream);
    }
    return e != hipSuccess ? e : hipStreamSynchronize(h->stream);
}

// The points of a track or a query: a depth image (ds, n = width * height) or a cloud of n records (lay), in host memory (the
// consumer stages them in its scratch) or on the device.
struct PointSource {
    const void* host;
    const void* dev;
    bool depth;
    DepthSpec ds;
    FrameLayout lay;
    uint32_t n;
    // the bytes that hold the first n_pts points: the whole image for a depth image
    size_t bytes(uint32_t n_pts) const
    {
        return depth ? ds.depth_bytes() : (size_t)(n_pts - 1) * lay.point_step + std::max({lay.off_x, lay.off_y, lay.off_z}) + 4;
    }
    // the PointForm the kernels read it in from device address base
    int form(const void* base) const { return depth ? kFormDepth : packed16(lay, base, false) ? kFormPacked16 : kFormStrided; }
};

// A depth image for a consumer that reads no colour (track, query): the descriptor is validated as integrate validates it, its
// colour fields included, but no colour image is read (color_bpp = 0).
static int colorless_depth_source(hfpf_handle* h, const hfpf_depth_image* desc, const void* depth, PointSource* f)
{
    if (int rc = depth_spec(h, desc, depth, desc && desc->color_format != HFPF_COLOR_NONE ? depth : nullptr, &f->ds)) return rc;
    f->ds.color_bpp = 0;
    f->depth = true;
    f->n = f->ds.width * f->ds.height;
    return HFPF_OK;
}

// (A + damping I) x = -b by Cholesky L L^T, column j outer, then the two triangular solves: the order include/hfpf.h states.
// false when a pivot is not > 0.
static bool track_solve(const double A[6][6], const double b[6], double damping, double x[6])
{
    double L[6][6] = {};
    for (int j = 0; j < 6; j++) {
        double s = A[j][j] + damping;
        for (int k = 0; k < j; k++) s = s - L[j][k] * L[j][k];
        if (!(s > 0.0)) return false;
        L[j][j] = std::sqrt(s);
        for (int i = j + 1; i < 6; i++) {
            double t = A[i][j];
            for (int k = 0; k < j; k++) t = t - L[i][k] * L[j][k];
            L[i][j] = t / L[j][j];
        }
    }
    double y[6];
    for (int i = 0; i < 6; i++) {
        double s = -b[i];
        for (int k = 0; k < i; k++) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
    for (int i = 5; i >= 0; i--) {
        double s = y[i];
        for (int k = i + 1; k < 6; k++) s = s - L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
    return true;
}

// T <- (R(omega) R, (c + R(omega) (t - c)) + tau), R(omega) the Cayley map of include/hfpf.h.
static void track_update(double T[12], const double xi[6], const double c[3])
{
    const double wx = 0.5 * xi[0], wy = 0.5 * xi[1], wz = 0.5 * xi[2];
    const double ww = (wx * wx + wy * wy) + wz * wz;
    const double f = 2.0 / (1.0 + ww);
    const double W[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
    double R[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double w2 = (W[i][0] * W[0][j] + W[i][1] * W[1][j]) + W[i][2] * W[2][j];
            R[i][j] = (i == j ? 1.0 : 0.0) + f * (W[i][j] + w2);
        }
    const double e[3] = {T[3] - c[0], T[7] - c[1], T[11] - c[2]};
    double out[12];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out[4 * i + j] = (R[i][0] * T[j] + R[i][1] * T[4 + j]) + R[i][2] * T[8 + j];
        out[4 * i + 3] = (c[i] + ((R[i][0] * e[0] + R[i][1] * e[1]) + R[i][2] * e[2])) + xi[3 + i];
    }
    memcpy(T, out, sizeof out);
}

static_assert(HFPF_TRACK_CONVERGED == HFPF_ALIGN_CONVERGED && HFPF_TRACK_DEGENERATE == HFPF_ALIGN_DEGENERATE && HFPF_TRACK_TOO_FEW == HFPF_ALIGN_TOO_FEW,
              "refine_pose writes one set of outcome flags for both calls");

// The Gauss-Newton loop of hfpf_track* and hfpf_align_mesh* (include/hfpf.h, the track section), from the start pose.  Per iteration
// enqueue(T, acc) zeroes acc and puts the n_terms int64 sums of k_track_reduce / k_align_reduce at the estimate T into it on
// h->stream; the sums are read back, and the host solves and updates about c.  A failing enqueue returns its code at once and *res
// (either call's result) stays as it was; otherwise the fields both results have are written, and *word29 is the last system's sum
// 29 (track's points used; 0 with 29 terms).
extern "C++" template <typename Opts, typename Enqueue, typename Res>
static int refine_pose(hfpf_handle* h, const Opts* o, const double c[3], int n_terms, const double pose[12], Enqueue&& enqueue, Res* res, uint64_t* word29)
{
    const size_t bytes = (size_t)n_terms * sizeof(unsigned long long);
    unsigned long long* acc; if (int rc = scratch_n(h, h->icp_acc, (uint64_t)n_terms, &acc)) return rc;
    unsigned long long local[kTrackTerms];
    unsigned long long* back = h->xfer_pin[0] ? (unsigned long long*)h->xfer_pin[0] : local;  // the read-back of the sums
    double T[12], A[6][6] = {}, rr = 0.0;
    memcpy(T, pose, sizeof T);
    uint64_t inliers = 0;
    uint32_t flags = 0, it = 0;
    while (it < o->max_iterations) {
        it++;
        if (int rc = enqueue(T, acc)) return rc;
        HIPCHK(h, hipMemcpyAsync(back, acc, bytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        long long s[kTrackTerms] = {};
        memcpy(s, back, bytes);
        for (int i = 0, k = 0; i < 6; i++)
            for (int j = i; j < 6; j++, k++) A[i][j] = A[j][i] = (double)s[k] / kTrackScaleJJ;
        double b[6];
        for (int i = 0; i < 6; i++) b[i] = (double)s[21 + i] / kTrackScaleJR;
        rr = (double)s[27] / kTrackScaleRR;
        inliers = (uint64_t)s[28];
        *word29 = (uint64_t)s[29];
        if (inliers < o->min_inliers) {
            flags = HFPF_TRACK_TOO_FEW;
            break;
        }
        double xi[6];
        if (!track_solve(A, b, o->damping, xi)) {
            flags = HFPF_TRACK_DEGENERATE;
            break;
        }
        track_update(T, xi, c);
        if ((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2] < o->eps_rotation * o->eps_rotation &&
            (xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5] < o->eps_translation * o->eps_translation) {
            flags = HFPF_TRACK_CONVERGED;
            break;
        }
    }
    res->iterations = it;
    res->flags = flags;
    res->reserved = 0;
    res->inliers = inliers;
    res->rms = inliers ? std::sqrt(rr / (double)inliers) : 0.0;
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) res->information[6 * i + j] = A[i][j];
    memcpy(res->pose, T, sizeof T);
    return HFPF_OK;
}

// Validated arguments in, under the lock: the model view once, then refine_pose with one k_track_reduce per iteration.
static int track_locked(hfpf_handle* h, const hfpf_track_opts* o, const PointSource& f, const double pose[12], hfpf_track_result* res)
{
    // the sampling of include/hfpf.h, at most 2^26 points (the headroom of the int64 sums); cols: sampled columns of a depth image
    const uint32_t stride = o->stride;
    const uint32_t cols = f.depth ? (f.ds.width + stride - 1) / stride : 0u;
    const uint64_t n_samples = f.depth ? (uint64_t)cols * ((f.ds.height + stride - 1) / stride) : ((uint64_t)f.n + stride - 1) / stride;
    if (n_samples > (1ull << 26)) return fail(h, HFPF_ERR_BAD_ARG, "track: more than 2^26 sampled points");
    int rc;
    if ((rc = local_read_prologue_locked(h, "track"))) return rc;
    const uint8_t* frame = (const uint8_t*)f.dev;
    if (f.host) {  // one copy per call, through the pinned buffers
        uint8_t* staged; if ((rc = scratch_n(h, h->track_in, f.bytes(f.n), &staged))) return rc;
        const hipError_t e = upload_pageable(h, staged, f.host, f.bytes(f.n));
        if (e != hipSuccess) return fail(h, HFPF_ERR_HIP, "track upload: %s", hipGetErrorString(e));
        frame = staged;
    }
    RenderViews rv;
    if ((rc = render_views_locked(h, &o->view, 1, pose, &rv))) return rc;
    if ((rc = render_splat_locked(h, &rv, 0))) return rc;

    TrackParams p{};
    memcpy(p.V, pose, sizeof p.V);
    p.cam = pinhole_of(o->view);
    p.max_d2 = o->max_distance * o->max_distance;
    p.zc_lo = h->g.zc_lo, p.zc_hi = h->g.zc_hi;
    p.n_samples = (uint32_t)n_samples;
    p.stride = stride;
    p.cols = cols;
    p.n_points = f.n;
    const double c[3] = {pose[3], pose[7], pose[11]};
    const int form = f.form(frame);
    const DepthLayout dl = depth_layout(f.ds, nullptr, 0);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(kTrackMaxBlocks, blocks_for(n_samples, 256));
    const Row* rows = rv.rows.rows;
    const unsigned long long* zb = rv.zbuf;
    uint64_t used = 0;
    rc = refine_pose(h, o, c, kTrackTerms, pose, [&](const double* T, unsigned long long* acc) -> int {
        memcpy(p.T, T, sizeof p.T);
        HIPCHK(h, hipMemsetAsync(acc, 0, kTrackTerms * sizeof(unsigned long long), h->stream));
        with_form(form, [&](auto F) {
            hipLaunchKernelGGL((k_track_reduce<F>), dim3(blocks), dim3(256), 0, h->stream, p, frame, form_layout<F>(f.lay, &dl), rows, zb, acc);
        });
        HIPCHK(h, hipGetLastError());
        return HFPF_OK;
    }, res, &used);
    if (!rc) res->points_used = used;
    return rc;
}

static int track_depth_common(hfpf_handle* h, const hfpf_track_opts* o, const hfpf_depth_image* desc, const void* depth, bool on_device,
                              const double pose[12], hfpf_track_result* res)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    if (!track_opts_ok(o) || !track_args_ok(pose, res)) return fail(h, HFPF_ERR_BAD_ARG, "track: invalid options, pose or result");
    PointSource f{};
    if (int rc = colorless_depth_source(h, desc, depth, &f)) return rc;
    if (on_device && (uintptr_t)depth % (f.ds.depth_f32 ? 4u : 2u)) return fail(h, HFPF_ERR_BAD_ARG, "track_depth_device: the image must be aligned to the sample size");
    (on_device ? f.dev : f.host) = depth;
    return track_locked(h, o, f, pose, res);
}

int hfpf_track_depth(hfpf_handle* h, const hfpf_track_opts* o, const hfpf_depth_image* desc, const void* depth, const double pose_3x4[12],
                     hfpf_track_result* result)
{
    return track_depth_common(h, o, desc, depth, false, pose_3x4, result);
}

int hfpf_track_depth_device(hfpf_handle* h, const hfpf_track_opts* o, const hfpf_depth_image* desc, const void* dev_depth, const double pose_3x4[12],
                            hfpf_track_result* result)
{
    return track_depth_common(h, o, desc, dev_depth, true, pose_3x4, result);
}

int hfpf_track(hfpf_handle* h, const hfpf_track_opts* o, const void* base, uint32_t n_points, uint32_t point_step, uint32_t off_x, uint32_t off_y,
               uint32_t off_z, const double pose_3x4[12], hfpf_track_result* result)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    if (!track_opts_ok(o) || !track_args_ok(pose_3x4, result)) return fail(h, HFPF_ERR_BAD_ARG, "track: invalid options, pose or result");
    if (!base || n_points == 0) return fail(h, HFPF_ERR_BAD_ARG, "track: null cloud or no points");
    PointSource f{};
    f.host = base;
    f.lay = FrameLayout{point_step, off_x, off_y, off_z, 0};
    f.n = n_points;
    if (int rc = check_cloud_layout(h, "track", f.lay, false)) return rc;
    return track_locked(h, o, f, pose_3x4, result);
}

// ---- point queries (include/hfpf.h) ---------------------------------------------------------------------------------------
constexpr uint32_t kQueryChunk = 1u << 20;  // points per launch of the host forms: 64 MB of hits + 64 MB of rows of scratch

static bool query_args_ok(const hfpf_query_opts* o, const double* pose)
{
    if (!o || o->struct_size != sizeof(hfpf_query_opts) || o->reserved0 != 0 || o->reserved != 0) return false;
    if ((o->flags & ~HFPF_QUERY_ZCLIP) || o->radius < 0 || o->radius > kQueryMaxRadius) return false;
    if (std::isnan(o->min_count) || !(o->max_distance > 0.0)) return false;
    return pose_ok(pose);
}

// Validated arguments in, under the lock.  The device form is one launch into the caller's buffers; the host forms run chunks of
// kQueryChunk points through h->query_out and download each through the pinned buffers.
static int query_locked(hfpf_handle* h, const hfpf_query_opts* o, const PointSource& f, const double pose[12], hfpf_query_hit* hits, hfpf_row* rows)
{
    int rc;
    if ((rc = local_read_prologue_locked(h, "query"))) return rc;
    if (f.n == 0) return HFPF_OK;
    QueryParams p{};
    memcpy(p.T, pose, sizeof p.T);
    p.min_count = std::max(1.0, o->min_count);
    p.max_d2 = o->max_distance * o->max_distance;
    p.radius = o->radius;
    p.zclip = (o->flags & HFPF_QUERY_ZCLIP) ? 1u : 0u;
    const DepthLayout dl = depth_layout(f.ds, nullptr, 0);
    auto launch = [&](const uint8_t* frame, uint64_t first, uint32_t n, QueryHit* dh, Row* dr) -> int {
        p.first = first;
        p.n = n;
        const dim3 grid(blocks_for(n, 256));
        with_form(f.form(frame), [&](auto F) {
            hipLaunchKernelGGL((k_query<F>), grid, dim3(256), 0, h->stream, h->g, h->t, p, frame, form_layout<F>(f.lay, &dl), dh, dr);
        });
        HIPCHK(h, hipGetLastError());
        return HFPF_OK;
    };
    if (f.dev) {
        if ((rc = launch((const uint8_t*)f.dev, 0, f.n, (QueryHit*)hits, (Row*)rows))) return rc;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return HFPF_OK;
    }
    const uint32_t chunk = std::min(f.n, kQueryChunk);
    QueryHit* dh; Row* dr = nullptr;
    ScratchLayout out = ScratchLayout().add(&dh, chunk);
    if (rows) out.add(&dr, chunk);
    if ((rc = scratch(h, h->query_out, out))) return rc;
    uint8_t* in; if ((rc = scratch_n(h, h->query_in, f.bytes(chunk), &in))) return rc;
    if (f.depth) {  // the whole image once; the chunks index into it
        const hipError_t e = upload_pageable(h, in, f.host, f.bytes(f.n));
        if (e != hipSuccess) return fail(h, HFPF_ERR_HIP, "query upload: %s", hipGetErrorString(e));
    }
    for (uint64_t first = 0; first < f.n; first += chunk) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(chunk, f.n - first);
        uint64_t k_first = first;
        if (!f.depth) {  // this chunk's records
            const hipError_t e = upload_pageable(h, in, (const uint8_t*)f.host + first * f.lay.point_step, f.bytes(n));
            if (e != hipSuccess) return fail(h, HFPF_ERR_HIP, "query upload: %s", hipGetErrorString(e));
            k_first = 0;
        }
        if ((rc = launch(in, k_first, n, dh, dr))) return rc;
        hipError_t e = download_pageable(h, hits + first, dh, (size_t)n * sizeof(QueryHit), 0);
        if (e == hipSuccess && rows) e = download_pageable(h, rows + first, dr, (size_t)n * sizeof(Row), 0);
        if (e != hipSuccess) return fail(h, HFPF_ERR_HIP, "query download: %s", hipGetErrorString(e));
    }
    return HFPF_OK;
}

static int query_cloud_common(hfpf_handle* h, const hfpf_query_opts* o, const void* base, bool on_device, uint32_t n_points, uint32_t point_step,
                              uint32_t off_x, uint32_t off_y, uint32_t off_z, const double pose[12], hfpf_query_hit* hits, hfpf_row* rows)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    if (!query_args_ok(o, pose)) return fail(h, HFPF_ERR_BAD_ARG, "query: invalid options or pose");
    if (n_points && (!base || !hits)) return fail(h, HFPF_ERR_BAD_ARG, "query: null cloud or hits");
    PointSource f{};
    f.lay = FrameLayout{point_step, off_x, off_y, off_z, 0};
    if (int rc = check_cloud_layout(h, "query", f.lay, false)) return rc;
    if (on_device && (((uintptr_t)base & 3) || ((uintptr_t)hits & 15) || ((uintptr_t)rows & 15)))
        return fail(h, HFPF_ERR_BAD_ARG, "query_device: the cloud must be 4-byte and hits / rows 16-byte aligned");
    (on_device ? f.dev : f.host) = base;
    f.n = n_points;
    return query_locked(h, o, f, pose, hits, rows);
}

int hfpf_query(hfpf_handle* h, const hfpf_query_opts* o, const void* base, uint32_t n_points, uint32_t point_step, uint32_t off_x, uint32_t off_y,
               uint32_t off_z, const double pose_3x4[12], hfpf_query_hit* hits, hfpf_row* rows)
{
    return query_cloud_common(h, o, base, false, n_points, point_step, off_x, off_y, off_z, pose_3x4, hits, rows);
}

int hfpf_query_device(hfpf_handle* h, const hfpf_query_opts* o, const void* dev_base, uint32_t n_points, uint32_t point_step, uint32_t off_x,
                      uint32_t off_y, uint32_t off_z, const double pose_3x4[12], hfpf_query_hit* dev_hits, hfpf_row* dev_rows)
{
    return query_cloud_common(h, o, dev_base, true, n_points, point_step, off_x, off_y, off_z, pose_3x4, dev_hits, dev_rows);
}

int hfpf_query_depth(hfpf_handle* h, const hfpf_query_opts* o, const hfpf_depth_image* desc, const void* depth, const double pose_3x4[12],
                     hfpf_query_hit* hits, hfpf_row* rows)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    if (!query_args_ok(o, pose_3x4) || !hits) return fail(h, HFPF_ERR_BAD_ARG, "query: invalid options, pose or hits");
    PointSource f{};
    if (int rc = colorless_depth_source(h, desc, depth, &f)) return rc;
    f.host = depth;
    return query_locked(h, o, f, pose_3x4, hits, rows);
}

// ---- raycast (include/hfpf.h) ---------------------------------------------------------------------------------------------
constexpr uint64_t kRayChunk = 1ull << 20;       // rays (or pixels) per launch of the host forms: 24 MB of rays, 64 MB of hits
constexpr double kRayMaxSamples = 1048576.0;     // samples per ray
constexpr uint32_t kRayViewsPerLaunch = 32768;   // views per launch (grid.y)

int hfpf_check_raycast_opts(const hfpf_raycast_opts* o)
{
    if (!o || o->struct_size != sizeof(hfpf_raycast_opts) || o->reserved0 != 0 || o->reserved != 0) return HFPF_ERR_BAD_ARG;
    if ((o->flags & ~HFPF_RAYCAST_CULL_BACKFACES) || o->radius < 1 || o->radius > kQueryMaxRadius) return HFPF_ERR_BAD_ARG;
    if (std::isnan(o->min_count) || !(o->max_distance > 0.0)) return HFPF_ERR_BAD_ARG;
    if (!(std::isfinite(o->step) && o->step >= 0.125 && o->step <= 4.0)) return HFPF_ERR_BAD_ARG;
    if (!(std::isfinite(o->t_min) && std::isfinite(o->t_max) && 0.0 <= o->t_min && o->t_min < o->t_max)) return HFPF_ERR_BAD_ARG;
    return HFPF_OK;
}

// The checks of a raycast that need the handle: options, pose and the sample count n = floor((t1 - t0) / dt) + 1 <= 2^20.
static bool ray_args_ok(const hfpf_handle* h, const hfpf_raycast_opts* o, const double* pose, uint32_t n_poses, uint32_t* n_samples)
{
    if (hfpf_check_raycast_opts(o) != HFPF_OK) return false;
    const double q = std::floor((o->t_max - o->t_min) / (o->step * h->g.res));
    if (!(q < kRayMaxSamples)) return false;
    *n_samples = (uint32_t)q + 1u;
    if (n_poses && !pose) return false;
    for (uint32_t v = 0; v < n_poses; v++)
        if (!pose_ok(pose + 12ull * v)) return false;
    return true;
}

// The empty-space maps of k_raycast in h->ray_map (per directory entry "has a row", then maps 0..2), and the launch parameters.
static int ray_setup_locked(hfpf_handle* h, const hfpf_raycast_opts* o, uint32_t n_samples, RayParams* p)
{
    *p = RayParams{};
    p->min_count = std::max(1.0, o->min_count);
    p->max_d2 = o->max_distance * o->max_distance;
    p->t0 = o->t_min;
    p->dt = o->step * h->g.res;
    p->n_samples = n_samples;
    p->radius = o->radius;
    p->cull = (o->flags & HFPF_RAYCAST_CULL_BACKFACES) ? 1u : 0u;
    uint64_t cells[kRayLevels];
    for (int l = 0; l < kRayLevels; l++) {
        for (int a = 0; a < 3; a++) p->mdim[l][a] = l == 0 ? h->g.bdim[a] : (p->mdim[l - 1][a] + 3) / 4;
        cells[l] = (uint64_t)p->mdim[l][0] * p->mdim[l][1] * p->mdim[l][2];
    }
    if (cells[0] > 0xFFFFFFFFull) return fail(h, HFPF_ERR_CAPACITY, "raycast: %llu directory entries exceed the 32-bit map index", (unsigned long long)cells[0]);
    uint8_t *has, *maps[kRayLevels];
    ScratchLayout lay = ScratchLayout().add(&has, cells[0], 256);  // every map in whole 256-byte lines
    for (int l = 0; l < kRayLevels; l++) lay.add(&maps[l], cells[l], 256);
    if (int rc = scratch(h, h->ray_map, lay)) return rc;
    for (int l = 0; l < kRayLevels; l++) p->map[l] = maps[l];
    hipLaunchKernelGGL(k_ray_map_bricks, dim3(blocks_for(cells[0], 256)), dim3(256), 0, h->stream, h->t, (uint32_t)cells[0], has);
    hipLaunchKernelGGL(k_ray_map_dilate, dim3(blocks_for(cells[0], 256)), dim3(256), 0, h->stream, has, p->mdim[0][0], p->mdim[0][1], p->mdim[0][2], maps[0]);
    for (int l = 1; l < kRayLevels; l++)
        hipLaunchKernelGGL(k_ray_map_up, dim3(blocks_for(cells[l], 256)), dim3(256), 0, h->stream, maps[l - 1], p->mdim[l - 1][0], p->mdim[l - 1][1],
                           p->mdim[l - 1][2], p->mdim[l][0], p->mdim[l][1], p->mdim[l][2], maps[l]);
    HIPCHK(h, hipGetLastError());
    return HFPF_OK;
}

static int raycast_common(hfpf_handle* h, const hfpf_raycast_opts* o, const hfpf_ray* rays, bool on_device, uint64_t n_rays, const double pose[12],
                          hfpf_ray_hit* hits)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    uint32_t n_samples = 0;
    if (!ray_args_ok(h, o, pose, 1, &n_samples)) return fail(h, HFPF_ERR_BAD_ARG, "raycast: invalid options, pose or more than 2^20 samples a ray");
    if (!hits || (n_rays && !rays)) return fail(h, HFPF_ERR_BAD_ARG, "raycast: null rays or hits");
    if (on_device && (((uintptr_t)rays & 3) || ((uintptr_t)hits & 15)))
        return fail(h, HFPF_ERR_BAD_ARG, "raycast_device: rays must be 4-byte and hits 16-byte aligned");
    int rc;
    if ((rc = local_read_prologue_locked(h, "raycast"))) return rc;
    if (n_rays == 0) return HFPF_OK;
    RayParams p;
    if ((rc = ray_setup_locked(h, o, n_samples, &p))) return rc;
    memcpy(p.T, pose, sizeof p.T);
    auto launch = [&](const hfpf_ray* dr, uint64_t n, hfpf_ray_hit* dh) -> int {
        p.n_rays = n;
        return timed_launch(h, kTimeRaycast, [&] {
            hipLaunchKernelGGL(k_raycast, dim3(blocks_for(n, 256)), dim3(256), 0, h->stream, h->g, h->t, p, (const float*)dr, (RayHit*)dh);
        });
    };
    if (on_device) {
        if ((rc = launch(rays, n_rays, hits))) return rc;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return HFPF_OK;
    }
    const uint64_t chunk = std::min(n_rays, kRayChunk);
    hfpf_ray* d_rays; RayHit* d_hits; if ((rc = scratch_n(h, h->ray_in, chunk, &d_rays)) || (rc = scratch_n(h, h->ray_out, chunk, &d_hits))) return rc;
    for (uint64_t first = 0; first < n_rays; first += chunk) {
        const uint64_t n = std::min(chunk, n_rays - first);
        hipError_t e = upload_pageable(h, d_rays, rays + first, n * sizeof(hfpf_ray));
        if (e != hipSuccess) return fail(h, HFPF_ERR_HIP, "raycast upload: %s", hipGetErrorString(e));
        if ((rc = launch(d_rays, n, (hfpf_ray_hit*)d_hits))) return rc;
        e = download_pageable(h, hits + first, d_hits, n * sizeof(RayHit), 0);
        if (e != hipSuccess) return fail(h, HFPF_ERR_HIP, "raycast download: %s", hipGetErrorString(e));
    }
    return HFPF_OK;
}

int hfpf_raycast(hfpf_handle* h, const hfpf_raycast_opts* o, const hfpf_ray* rays, uint64_t n_rays, const double pose_3x4[12], hfpf_ray_hit* hits)
{
    return raycast_common(h, o, rays, false, n_rays, pose_3x4, hits);
}

int hfpf_raycast_device(hfpf_handle* h, const hfpf_raycast_opts* o, const hfpf_ray* dev_rays, uint64_t n_rays, const double pose_3x4[12],
                        hfpf_ray_hit* dev_hits)
{
    return raycast_common(h, o, dev_rays, true, n_rays, pose_3x4, dev_hits);
}

// Views: the device form runs whole images, kRayViewsPerLaunch views a launch; the host form runs one view in bands of whole
// 8-row tiles of about kRayChunk pixels through h->ray_out.
static int raycast_view_common(hfpf_handle* h, const hfpf_raycast_opts* o, uint32_t width, uint32_t height, double fx, double fy, double cx, double cy,
                               uint32_t n_views, const double* poses, bool on_device, hfpf_ray_hit* hits)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    uint32_t n_samples = 0;
    if (!ray_args_ok(h, o, poses, n_views, &n_samples)) return fail(h, HFPF_ERR_BAD_ARG, "raycast: invalid options, pose or more than 2^20 samples a ray");
    const uint64_t WH = (uint64_t)width * height;
    if (WH == 0 || WH > (1ull << 31)) return fail(h, HFPF_ERR_BAD_ARG, "raycast: width * height must lie in 1..2^31");
    if (!(std::isfinite(fx) && fx > 0.0 && std::isfinite(fy) && fy > 0.0 && std::isfinite(cx) && std::isfinite(cy)))
        return fail(h, HFPF_ERR_BAD_ARG, "raycast: invalid intrinsics");
    if (!hits) return fail(h, HFPF_ERR_BAD_ARG, "raycast: null hits");
    if (on_device && ((uintptr_t)hits & 15)) return fail(h, HFPF_ERR_BAD_ARG, "raycast_view_device: hits must be 16-byte aligned");
    int rc;
    if ((rc = local_read_prologue_locked(h, "raycast"))) return rc;
    if (n_views == 0) return HFPF_OK;
    RayParams p;
    if ((rc = ray_setup_locked(h, o, n_samples, &p))) return rc;
    p.fx = fx, p.fy = fy, p.cx = cx, p.cy = cy;
    p.width = width;
    p.view_stride = WH;
    double* pose_d; if ((rc = upload_poses(h, h->render_pose, poses, n_views, &pose_d))) return rc;
    const uint64_t tiles_x = (width + 7ull) / 8;
    auto launch = [&](uint32_t v0, uint32_t nv, uint32_t row0, uint32_t rows, RayHit* dh) -> int {
        p.row0 = row0;
        p.rows = rows;
        const uint64_t tiles = tiles_x * ((rows + 7ull) / 8);
        return timed_launch(h, kTimeRaycast, [&] {
            hipLaunchKernelGGL(k_raycast_view, dim3(blocks_for(tiles * 64, 256), nv), dim3(256), 0, h->stream, h->g, h->t, p, pose_d + 12ull * v0, dh);
        });
    };
    if (on_device) {
        for (uint32_t v0 = 0; v0 < n_views; v0 += kRayViewsPerLaunch)
            if ((rc = launch(v0, std::min(kRayViewsPerLaunch, n_views - v0), 0, height, (RayHit*)hits + v0 * WH))) return rc;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return HFPF_OK;
    }
    const uint32_t band = (uint32_t)std::min<uint64_t>(height, std::max<uint64_t>(8, (kRayChunk / width) & ~7ull));
    RayHit* d_hits; if ((rc = scratch_n(h, h->ray_out, (uint64_t)band * width, &d_hits))) return rc;
    for (uint32_t row0 = 0; row0 < height; row0 += band) {
        const uint32_t rows = std::min(band, height - row0);
        if ((rc = launch(0, 1, row0, rows, d_hits))) return rc;
        const hipError_t e = download_pageable(h, hits + (uint64_t)row0 * width, d_hits, (uint64_t)rows * width * sizeof(RayHit), 0);
        if (e != hipSuccess) return fail(h, HFPF_ERR_HIP, "raycast download: %s", hipGetErrorString(e));
    }
    return HFPF_OK;
}

int hfpf_raycast_view(hfpf_handle* h, const hfpf_raycast_opts* o, uint32_t width, uint32_t height, double fx, double fy, double cx, double cy,
                      const double pose_3x4[12], hfpf_ray_hit* hits)
{
    return raycast_view_common(h, o, width, height, fx, fy, cx, cy, 1, pose_3x4, false, hits);
}

int hfpf_raycast_view_device(hfpf_handle* h, const hfpf_raycast_opts* o, uint32_t width, uint32_t height, double fx, double fy, double cx,
                             double cy, uint32_t n_views, const double* poses, hfpf_ray_hit* dev_hits)
{
    return raycast_view_common(h, o, width, height, fx, fy, cx, cy, n_views, poses, true, dev_hits);
}

// ---- surface mesh (include/hfpf.h) ----------------------------------------------------------------------------------------
int hfpf_check_mesh_opts(const hfpf_mesh_opts* o)
{
    if (!o || o->struct_size != sizeof(hfpf_mesh_opts) || o->flags != 0 || o->reserved != 0) return HFPF_ERR_BAD_ARG;
    if (o->radius < 1 || o->radius > kQueryMaxRadius) return HFPF_ERR_BAD_ARG;
    return !std::isnan(o->min_count) && o->max_distance > 0.0 ? HFPF_OK : HFPF_ERR_BAD_ARG;  // (a NaN max_distance fails the compare)
}
static bool mesh_opts_ok(const hfpf_mesh_opts* o) { return hfpf_check_mesh_opts(o) == HFPF_OK; }

// h->mesh_ctr: the count a unique pass leaves, and behind it the word a corner lookup that misses sets (a broken invariant).
static int mesh_ctr_locked(hfpf_handle* h, uint64_t** n_unique, uint32_t** miss)
{
    return scratch(h, h->mesh_ctr, ScratchLayout().add(n_unique, 1).add(miss, 2));
}

// One 1-D dilation of the sorted unique keys in[0, n_in): k_mesh_dilate into keys_a, sort into keys_b, unique into out (*out_keys).
// in may be out, and is therefore the one buffer read here through the pointer of an earlier allocation: the dilation that reads it
// is enqueued before scratch() of out, which synchronises before it reallocates.
static int mesh_dilate_locked(hfpf_handle* h, const DevBuf& in, uint64_t n_in, int axis, int lo, int hi, int32_t lim, DevBuf& out, const uint64_t** out_keys, uint64_t* n_out)
{
    const uint64_t n = n_in * (uint64_t)(hi - lo + 1);
    int rc;
    uint64_t *dilated, *sorted, *unique, *n_unique; uint32_t* miss;
    if ((rc = scratch_n(h, h->keys_a, n, &dilated)) || (rc = scratch_n(h, h->keys_b, n, &sorted))) return rc;
    hipLaunchKernelGGL(k_mesh_dilate, dim3(blocks_for(n_in, 256)), dim3(256), 0, h->stream, static_cast<const uint64_t*>(in.p), n_in, axis, lo, hi, lim, dilated);
    HIPCHK(h, hipGetLastError());
    unsigned xbits = 0;  // x <= dim[0]: the keys are below 2^(42 + xbits)
    while ((uint32_t)h->g.dim[0] >> xbits) xbits++;
    if ((rc = sort_keys_u64(h, dilated, sorted, n, 2 * kMeshKeyBits + xbits))) return rc;
    if ((rc = scratch_n(h, out, n, &unique)) || (rc = mesh_ctr_locked(h, &n_unique, &miss))) return rc;
    *out_keys = unique;
    return unique_keys_locked(h, sorted, n, unique, n_unique, n_out);
}

// Validated arguments in, under the lock, behind the read prologue.  The row set, the cube set (the rows' cells dilated by 1) and the
// corner set (the cubes dilated by (0, +1)), the corner samples, the edge marks and triangle counts, two scans, then vertices and
// triangles into device arrays (*out: vertices, triangles).  The read-backs are the sizes between the stages.
static int mesh_locked(hfpf_handle* h, const hfpf_mesh_opts* o, bool on_device, ResultSet* out, uint64_t* n_verts, uint64_t* n_tris)
{
    *n_verts = 0, *n_tris = 0;  // (*out: the caller's fresh, empty set)
    int rc;
    for (int a = 0; a < 3; a++)
        if (h->g.dim[a] >= (1 << kMeshKeyBits) - 1) return fail(h, HFPF_ERR_CAPACITY, "mesh: a grid dimension of 2^21 - 1 cells or more");
    RowSet rs;
    const ExtractOpts opt{std::max(1.0, o->min_count), -1, 0};  // count >= max(1, min_count), the compare of k_extract_keys
    if ((rc = build_rows_locked(h, h->t.stats, opt, &rs))) return rc;
    const uint64_t nr = rs.n;
    if (nr == 0) return HFPF_OK;
    uint64_t* row_keys; if ((rc = scratch_n(h, h->mesh_cube, nr, &row_keys))) return rc;
    hipLaunchKernelGGL(k_mesh_row_keys, dim3(blocks_for(nr, 256)), dim3(256), 0, h->stream, rs.rows, nr, row_keys);
    HIPCHK(h, hipGetLastError());
    uint64_t n = nr;
    const uint64_t *cubes = nullptr, *corners = nullptr;
    for (int a = 0; a < 3; a++)
        if ((rc = mesh_dilate_locked(h, h->mesh_cube, n, a, -1, 1, h->g.dim[a] - 1, h->mesh_cube, &cubes, &n))) return rc;
    const uint64_t nc = n;
    for (int a = 0; a < 3; a++)
        if ((rc = mesh_dilate_locked(h, a == 0 ? h->mesh_cube : h->mesh_corner, n, a, 0, 1, h->g.dim[a], h->mesh_corner, &corners, &n))) return rc;
    const uint64_t nk = n;
    // vertex and triangle ids are 32-bit: at most 7 vertices a corner and 12 triangles a cube
    if (7 * nk >= 0xFFFFFFFFull || 12 * nc >= 0xFFFFFFFFull)
        return fail(h, HFPF_ERR_CAPACITY, "mesh: %llu corners / %llu cubes exceed the 32-bit vertex and triangle ids", (unsigned long long)nk,
                    (unsigned long long)nc);
    const uint64_t K1 = nk + 1, C1 = nc + 1;
    float* s;  // per corner (nk + 1 entries each): the sample, the nearest row, the edge marks, the vertex count and its scan
    uint32_t *nid, *marks, *vcount, *vbase;
    uint32_t *tcount, *tbase;  // per cube (nc + 1 entries each): the triangle count and its scan
    if ((rc = scratch(h, h->mesh_kdata, ScratchLayout().add(&s, K1).add(&nid, K1).add(&marks, K1).add(&vcount, K1).add(&vbase, K1)))) return rc;
    if ((rc = scratch(h, h->mesh_cdata, ScratchLayout().add(&tcount, C1).add(&tbase, C1)))) return rc;
    const MeshParams p{std::max(1.0, o->min_count), o->max_distance * o->max_distance, o->radius};
    uint64_t* n_unique; uint32_t* miss; if ((rc = mesh_ctr_locked(h, &n_unique, &miss))) return rc;
    HIPCHK(h, hipMemsetAsync(miss, 0, 4, h->stream));
    hipLaunchKernelGGL(k_mesh_sample, dim3(blocks_for(nk, 256)), dim3(256), 0, h->stream, h->g, h->t, p, corners, (uint32_t)nk, s, nid);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemsetAsync(marks, 0, K1 * 4, h->stream));
    hipLaunchKernelGGL(k_mesh_mark, dim3(blocks_for(C1, 256)), dim3(256), 0, h->stream, cubes, (uint32_t)nc, corners, (uint32_t)nk, s, nid, marks, tcount, miss);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_mesh_vcount, dim3(blocks_for(K1, 256)), dim3(256), 0, h->stream, marks, (uint32_t)nk, vcount);
    HIPCHK(h, hipGetLastError());
    uint64_t nv = 0, nt = 0;
    if ((rc = scan_counts_locked(h, vcount, vbase, nk, &nv))) return rc;
    if ((rc = scan_counts_locked(h, tcount, tbase, nc, &nt))) return rc;
    uint32_t missed = 0;
    HIPCHK(h, hipMemcpy(&missed, miss, 4, hipMemcpyDeviceToHost));  // (the scan's read-back has synchronised the stream)
    if (missed) return fail(h, HFPF_ERR_STATE, "mesh: a corner of a cube is missing from the corner set (internal)");
    if (nv == 0 || nt == 0) return HFPF_OK;
    ResultSet set;
    set.add(nv * sizeof(MeshVertex));
    set.add(nt * 12);
    if ((rc = result_alloc(h, set, on_device, "mesh"))) return rc;
    MeshVertex* dv = (MeshVertex*)set.a[0].dev;
    uint32_t* dt = (uint32_t*)set.a[1].dev;
    hipLaunchKernelGGL(k_mesh_vertices, dim3(blocks_for(nk, 256)), dim3(256), 0, h->stream, h->g, h->t, corners, (uint32_t)nk, s, nid, marks, vbase, dv, miss);
    hipLaunchKernelGGL(k_mesh_triangles, dim3(blocks_for(nc, 256)), dim3(256), 0, h->stream, cubes, (uint32_t)nc, corners, (uint32_t)nk, s, nid, marks, vbase, tbase, dt, miss);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&missed, miss, 4, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (missed) return fail(h, HFPF_ERR_STATE, "mesh: a corner of a cube or an edge is missing from the corner set (internal)");
    if (e != hipSuccess) return fail(h, HFPF_ERR_HIP, "mesh: %s", hipGetErrorString(e));
    set.keep(out), *n_verts = nv, *n_tris = nt;
    return HFPF_OK;
}

// The read-outs below come as a host and a `_device` form of one *_common function, all written alike: the NULL handle, the lock,
// the argument check, the read prologue, the call's own empty case, the mesh on the device (mesh_on_device_locked), *_locked into
// locals, result_deliver, and only then the caller's outputs.  WHEN THE CALLER'S MEMORY IS WRITTEN: never on HFPF_ERR_BAD_ARG; on
// any other failure compare, align, cover, section, plan and consistency write nothing either, while mesh and components leave the
// NULL / 0 they set behind the argument check; every output is filled on success.
static int extract_mesh_common(hfpf_handle* h, const hfpf_mesh_opts* o, bool on_device, hfpf_mesh_vertex** verts, uint64_t* n_verts, uint32_t** tris,
                               uint64_t* n_tris)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    if (!mesh_opts_ok(o) || !verts || !n_verts || !tris || !n_tris) return fail(h, HFPF_ERR_BAD_ARG, "mesh: invalid options or a NULL output");
    *verts = nullptr, *tris = nullptr, *n_verts = 0, *n_tris = 0;
    ResultSet set;  // empty (nv = 0) without a vertex or without a triangle: NULL arrays, no download
    uint64_t nv = 0, nt = 0;
    void* out[kResultArrays];
    int rc;
    if ((rc = local_read_prologue_locked(h, "mesh")) || (rc = mesh_locked(h, o, on_device, &set, &nv, &nt))) return rc;
    if ((rc = result_deliver(h, set, on_device, "mesh", out))) return rc;
    *verts = (hfpf_mesh_vertex*)out[0], *tris = (uint32_t*)out[1], *n_verts = nv, *n_tris = nt;
    return HFPF_OK;
}

int hfpf_extract_mesh_device(hfpf_handle* h, const hfpf_mesh_opts* o, hfpf_mesh_vertex** dev_verts, uint64_t* n_verts, uint32_t** dev_tris,
                             uint64_t* n_tris)
{
    return extract_mesh_common(h, o, true, dev_verts, n_verts, dev_tris, n_tris);
}

int hfpf_extract_mesh(hfpf_handle* h, const hfpf_mesh_opts* o, hfpf_mesh_vertex** verts, uint64_t* n_verts, uint32_t** tris, uint64_t* n_tris)
{
    return extract_mesh_common(h, o, false, verts, n_verts, tris, n_tris);
}

void hfpf_free_mesh(hfpf_mesh_vertex* verts, uint32_t* tris)
{
    free(verts);
    free(tris);
}

// ---- connected components (include/hfpf.h) --------------------------------------------------------------------------------
int hfpf_check_component_opts(const hfpf_component_opts* o)
{
    if (!o || o->struct_size != sizeof(hfpf_component_opts) || o->flags != 0 || o->reserved0 != 0 || o->reserved != 0) return HFPF_ERR_BAD_ARG;
    if (o->reach < 1 || o->reach > kQueryMaxRadius || std::isnan(o->min_count)) return HFPF_ERR_BAD_ARG;
    return std::isfinite(o->min_normal_dot) && o->min_normal_dot >= -2.0 && o->min_normal_dot <= 1.0 ? HFPF_OK : HFPF_ERR_BAD_ARG;
}

// Validated arguments in, under the lock, behind the read prologue.  The row set, then (timed as kernel id 6) index, link, flatten,
// the scan of the root flags, the per-component reductions, the keep flags (through a sort for keep_largest), the scans of kept
// components and kept rows, and the compaction into *out (rows -- absent without want_rows --, labels, component records).  The
// read-backs are the sizes between the stages.
static int components_locked(hfpf_handle* h, const hfpf_component_opts* o, bool on_device, bool want_rows, ResultSet* out, uint64_t* n_rows,
                             uint64_t* n_comps)
{
    *n_rows = 0, *n_comps = 0;  // (*out: the caller's fresh, empty set)
    int rc;
    RowSet rs;
    const ExtractOpts opt{o->min_count, -1, 0};  // the compare of hfpf_extract_filtered, 0 keeps all
    if ((rc = build_rows_locked(h, h->t.stats, opt, &rs))) return rc;
    const uint64_t nr = rs.n;
    if (nr == 0) return HFPF_OK;
    if (nr >= 0xFFFFFFFFull) return fail(h, HFPF_ERR_CAPACITY, "components: %llu rows exceed the 32-bit row index", (unsigned long long)nr);
    const uint64_t n_rec = h->h_ctr[C_NORMALS];
    const uint32_t n = (uint32_t)nr;
    const uint64_t R1 = nr + 1;
    uint32_t *row_of, *parent, *root, *comp_of;
    uint32_t *flag, *cbase, *rbase;  // root flags, later the rows' keep flags; the scan of the root flags; the scan of the keep flags
    if ((rc = scratch_n(h, h->comp_index, n_rec + 1, &row_of))) return rc;
    if ((rc = scratch(h, h->comp_rows, ScratchLayout().add(&parent, R1).add(&root, R1).add(&comp_of, R1).add(&flag, R1).add(&cbase, R1).add(&rbase, R1)))) return rc;
    const Row* rows = rs.rows;
    const CompParams p{o->min_normal_dot, o->min_points, o->min_rows, o->keep_largest, o->reach};
    const dim3 grid_r(blocks_for(nr, 256)), grid_r1(blocks_for(R1, 256));
    Timed timed(h);
    if (timed.rc) return timed.rc;
    HIPCHK(h, hipMemsetAsync(row_of, 0xFF, (n_rec + 1) * 4, h->stream));
    hipLaunchKernelGGL(k_comp_index, grid_r, dim3(256), 0, h->stream, rs.record_of_row, n, row_of, parent);
    hipLaunchKernelGGL(k_comp_link, grid_r, dim3(256), 0, h->stream, h->g, h->t, p, rows, n, row_of, (uint32_t)n_rec, parent);
    hipLaunchKernelGGL(k_comp_flatten, grid_r1, dim3(256), 0, h->stream, parent, n, root, flag);
    HIPCHK(h, hipGetLastError());
    uint64_t nc = 0;
    if ((rc = scan_counts_locked(h, flag, cbase, nr, &nc))) return rc;
    const uint64_t C1 = nc + 1;
    Component* recs; uint32_t *keep, *kbase;  // per component (nc + 1 entries each): the keep flag and its scan
    if ((rc = scratch(h, h->comp_recs, ScratchLayout().add(&recs, nc).add(&keep, C1).add(&kbase, C1)))) return rc;
    const dim3 grid_c1(blocks_for(C1, 256));
    hipLaunchKernelGGL(k_comp_init, grid_r, dim3(256), 0, h->stream, root, cbase, n, comp_of, recs);
    hipLaunchKernelGGL(k_comp_reduce, grid_r, dim3(256), 0, h->stream, rows, comp_of, n, recs);
    if (o->keep_largest == 0) {
        hipLaunchKernelGGL(k_comp_keep, grid_c1, dim3(256), 0, h->stream, recs, (uint32_t)nc, p, keep);
        HIPCHK(h, hipGetLastError());
    } else {  // the components ranked through the sort buffers: nc <= nr, so nothing grows, and k_comp_index has read record_of_row
        uint64_t *keys_in, *keys_out; if ((rc = scratch_n(h, h->keys_a, nc, &keys_in)) || (rc = scratch_n(h, h->keys_b, nc, &keys_out))) return rc;
        uint32_t *vals_in, *vals_out; if ((rc = scratch_n(h, h->vals_a, nc, &vals_in)) || (rc = scratch_n(h, h->vals_b, nc, &vals_out))) return rc;
        rs.record_of_row = nullptr;  // dead from here: vals_out is the same memory
        hipLaunchKernelGGL(k_comp_rank_keys, grid_c1, dim3(256), 0, h->stream, recs, (uint32_t)nc, p, keys_in, vals_in, keep);
        HIPCHK(h, hipGetLastError());
        if ((rc = sort_pairs_u64(h, keys_in, keys_out, vals_in, vals_out, nc, 64))) return rc;
        const uint32_t front = (uint32_t)std::min<uint64_t>(nc, o->keep_largest);
        hipLaunchKernelGGL(k_comp_rank_keep, dim3(blocks_for(front, 256)), dim3(256), 0, h->stream, keys_out, vals_out, front, keep);
        HIPCHK(h, hipGetLastError());
    }
    hipLaunchKernelGGL(k_comp_row_keep, grid_r1, dim3(256), 0, h->stream, comp_of, keep, n, flag);
    HIPCHK(h, hipGetLastError());
    uint64_t nk = 0, nkr = 0;
    if ((rc = scan_counts_locked(h, keep, kbase, nc, &nk))) return rc;
    if ((rc = scan_counts_locked(h, flag, rbase, nr, &nkr))) return rc;
    if (nk == 0) return timed.file(kTimeComponents);
    ResultSet set;
    set.add(nkr * sizeof(Row), !want_rows);
    set.add(nkr * 4);
    set.add(nk * sizeof(Component));
    if ((rc = result_alloc(h, set, on_device, "components"))) return rc;
    hipLaunchKernelGGL(k_comp_compact, grid_r, dim3(256), 0, h->stream, rows, n, comp_of, keep, kbase, rbase, recs, (Row*)set.a[0].dev, (uint32_t*)set.a[1].dev,
                       (Component*)set.a[2].dev);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) rc = timed.file(kTimeComponents);
    if (e == hipSuccess && !rc) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess || rc) return rc ? rc : fail(h, HFPF_ERR_HIP, "components: %s", hipGetErrorString(e));
    set.keep(out), *n_rows = nkr, *n_comps = nk;
    return HFPF_OK;
}

static bool component_args_ok(const hfpf_component_opts* o, const void* labels, const void* n_rows, const void* comps, const void* n_comps)
{
    return hfpf_check_component_opts(o) == HFPF_OK && labels && n_rows && comps && n_comps;
}

static int extract_components_common(hfpf_handle* h, const hfpf_component_opts* o, bool on_device, hfpf_row** rows, uint32_t** labels, uint64_t* n_rows,
                                     hfpf_component** comps, uint64_t* n_comps)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    if (!component_args_ok(o, labels, n_rows, comps, n_comps)) return fail(h, HFPF_ERR_BAD_ARG, "components: invalid options or a NULL output");
    if (rows) *rows = nullptr;
    *labels = nullptr, *comps = nullptr, *n_rows = 0, *n_comps = 0;
    ResultSet set;  // empty (nc = 0) without a row or without a kept component: NULL arrays, no download
    uint64_t nr = 0, nc = 0;
    void* out[kResultArrays];
    int rc;
    if ((rc = local_read_prologue_locked(h, "components")) || (rc = components_locked(h, o, on_device, rows != nullptr, &set, &nr, &nc))) return rc;
    if ((rc = result_deliver(h, set, on_device, "components", out))) return rc;
    if (rows) *rows = (hfpf_row*)out[0];
    *labels = (uint32_t*)out[1], *comps = (hfpf_component*)out[2], *n_rows = nr, *n_comps = nc;
    return HFPF_OK;
}

int hfpf_extract_components_device(hfpf_handle* h, const hfpf_component_opts* o, hfpf_row** dev_rows, uint32_t** dev_labels, uint64_t* n_rows,
                                   hfpf_component** dev_comps, uint64_t* n_comps)
{
    return extract_components_common(h, o, true, dev_rows, dev_labels, n_rows, dev_comps, n_comps);
}

int hfpf_extract_components(hfpf_handle* h, const hfpf_component_opts* o, hfpf_row** rows, uint32_t** labels, uint64_t* n_rows, hfpf_component** comps,
                            uint64_t* n_comps)
{
    return extract_components_common(h, o, false, rows, labels, n_rows, comps, n_comps);
}

void hfpf_free_components(hfpf_row* rows, uint32_t* labels, hfpf_component* comps)
{
    free(rows);
    free(labels);
    free(comps);
}

// ---- deviation from a triangle mesh (include/hfpf.h) ------------------------------------------------------------------------
int hfpf_check_deviation_opts(const hfpf_deviation_opts* o)
{
    if (!o || o->struct_size != sizeof(hfpf_deviation_opts) || o->flags != 0 || o->reserved != 0 || std::isnan(o->min_count)) return HFPF_ERR_BAD_ARG;
    return std::isfinite(o->max_distance) && o->max_distance > 0.0 && o->max_distance <= 1.0 ? HFPF_OK : HFPF_ERR_BAD_ARG;
}

static unsigned bits_for_count(uint64_t n)  // bits that hold 0..n-1 (at least 1)
{
    unsigned b = 1;
    while (b < 64 && (1ull << b) < n) b++;
    return b;
}

// A triangle mesh as the calls take it (vertices of `stride` bytes that begin with three floats), in host or in device memory.
struct MeshRef {
    const void* verts;
    uint64_t n_verts;
    uint32_t stride;
    const uint32_t* tris;
    uint64_t n_tris;
};

// h->dev_tri: the mesh's vertices in the fusion frame (k_dev_verts), then one record per triangle -- compare's DevTri or cover's CovTri.
extern "C++" template <typename Rec>
static int dev_tri_scratch_locked(hfpf_handle* h, const MeshRef& m, double** V, Rec** recs)
{
    return scratch(h, h->dev_tri, ScratchLayout().add(V, 3 * std::max<uint64_t>(m.n_verts, 1)).add(recs, m.n_tris));
}

// The two halves of a compare, shared with hfpf_align_mesh*.  ROW SIDE (compare_row_side_locked, once per call; it does not depend on
// the pose): the rows of a row set keyed by the brick of their point and sorted, and the list of bricks that hold rows.  MESH SIDE
// (compare_mesh_side_locked, once per pose): the transformed vertices, the triangles' records and pair count, the pairs, their sort
// and per-brick ranges, and k_dev_rows into a Deviation array.  The read-backs are the sizes between the stages.
struct DevCounters {  // zeroed together in front of every mesh side
    unsigned long long ctr[DC_WORDS];
    DevSummary sum;
};
static_assert(sizeof(DevCounters) == DC_WORDS * 8 + sizeof(DevSummary), "the counters and the summary are adjacent");
struct DevRowSide {
    uint32_t n = 0;   // rows
    uint64_t nb = 0;  // bricks that hold rows
    const Row* rows = nullptr;
    const uint32_t* sorted_row = nullptr;  // rank in brick order -> row (h->vals_b, once the row side has sorted)
    // slices of h->dev_bins
    uint64_t* ub_key = nullptr;
    DevCounters* counters = nullptr;
    uint32_t *flag = nullptr, *base = nullptr;  // per sorted row: first of its brick, and the scan
    uint32_t *ub_start = nullptr, *trange = nullptr;  // trange: per brick the start of its triangle range, then (at + n) the end
};

// what: the caller's name in messages.  Allocates; a compare opens its Timed bracket behind it, before compare_row_side_locked.
static int compare_row_scratch_locked(hfpf_handle* h, const RowSet& rows, const char* what, DevRowSide* rs)
{
    if (rows.n >= 0xFFFFFFFFull) return fail(h, HFPF_ERR_CAPACITY, "%s: %llu rows exceed the 32-bit row index", what, (unsigned long long)rows.n);
    const uint32_t n = (uint32_t)rows.n;
    const uint64_t R1 = (uint64_t)n + 1;
    rs->n = n;
    rs->rows = rows.rows;
    return scratch(h, h->dev_bins,
                   ScratchLayout().add(&rs->ub_key, n).add(&rs->counters, 1).add(&rs->flag, R1).add(&rs->base, R1).add(&rs->ub_start, R1).add(&rs->trange, 2 * (uint64_t)n));
}

// Sorts through the handle's sort buffers: the row set's record_of_row is dead behind it, and vals_b is rs->sorted_row.
static int compare_row_side_locked(hfpf_handle* h, DevRowSide* rs)
{
    const uint32_t n = rs->n;
    if (!n) return HFPF_OK;
    int rc;
    const GridParams& g = h->g;
    uint64_t *keys_in, *keys_out; if ((rc = scratch_n(h, h->keys_a, n, &keys_in)) || (rc = scratch_n(h, h->keys_b, n, &keys_out))) return rc;
    uint32_t *vals_in, *vals_out; if ((rc = scratch_n(h, h->vals_a, n, &vals_in)) || (rc = scratch_n(h, h->vals_b, n, &vals_out))) return rc;  // (no growth: the row set's own sort was of at least n pairs)
    const size_t R1 = (size_t)n + 1;
    const dim3 grid_r(blocks_for(n, 256)), grid_r1(blocks_for(R1, 256));
    hipLaunchKernelGGL(k_dev_row_keys, grid_r, dim3(256), 0, h->stream, g, rs->rows, n, keys_in, vals_in);
    HIPCHK(h, hipGetLastError());
    const unsigned key_bits = bits_for_count((uint64_t)g.bdim[0] * (uint64_t)g.bdim[1] * (uint64_t)g.bdim[2]);
    if ((rc = sort_pairs_u64(h, keys_in, keys_out, vals_in, vals_out, n, key_bits))) return rc;
    rs->sorted_row = vals_out;
    hipLaunchKernelGGL(k_dev_row_flags, grid_r1, dim3(256), 0, h->stream, keys_out, n, rs->flag);
    HIPCHK(h, hipGetLastError());
    if ((rc = scan_counts_locked(h, rs->flag, rs->base, n, &rs->nb))) return rc;
    hipLaunchKernelGGL(k_dev_bricks, grid_r1, dim3(256), 0, h->stream, keys_out, rs->flag, rs->base, n, (uint32_t)rs->nb, rs->ub_key, rs->ub_start);
    HIPCHK(h, hipGetLastError());
    return HFPF_OK;
}

// The mesh at `pose` against the row side: the counters, the summary and the bricks' triangle ranges are zeroed first, so it may run
// any number of times behind one row side.  out: n Deviation records (untouched without rows); h_ctr: the DC_WORDS counters read back.
// The launch of k_dev_rows is left unchecked for the caller's hipGetLastError.
static int compare_mesh_side_locked(hfpf_handle* h, const DevRowSide& rs, const hfpf_deviation_opts* o, const MeshRef& m, const double* pose, Deviation* out,
                                    unsigned long long h_ctr[DC_WORDS])
{
    int rc;
    const uint32_t n = rs.n;
    const uint64_t nb = rs.nb;
    const GridParams& g = h->g;
    DevParams p;
    memcpy(p.T, pose, sizeof p.T);
    p.md = o->max_distance, p.md2 = o->max_distance * o->max_distance;
    double box = 0;
    for (int a = 0; a < 3; a++) box = std::max(box, std::max(std::fabs(g.min[a]), std::fabs(g.max[a])));
    // |P - X| for a row point P (inside the bounding box up to the reach of a voxel's statistics, taken generously) and a triangle
    // point X that can matter (within the inflated box of a triangle that reaches a brick): both within `box` + slack of the origin
    p.reach = 2.0 * (box + 64.0 * g.res + 4.0 * (double)g.ball_r + o->max_distance);
    p.face_cap = 4.0 * g.res;
    p.n_verts = m.n_verts, p.n_tris = (uint32_t)m.n_tris, p.stride = m.stride;
    p.nb = (uint32_t)nb, p.tile = h->knobs.test_dev_tile;
    unsigned long long* d_ctr = rs.counters->ctr;
    HIPCHK(h, hipMemsetAsync(rs.counters, 0, sizeof(DevCounters), h->stream));
    if (n) HIPCHK(h, hipMemsetAsync(rs.trange, 0, 2 * (size_t)n * 4, h->stream));
    for (int i = 0; i < DC_WORDS; i++) h_ctr[i] = 0;
    double* V = nullptr; DevTri* recs = nullptr;
    uint64_t *pairs_in = nullptr, *pairs = nullptr;  // pairs: read only inside a non-empty triangle range, and those need pairs
    if (m.n_tris) {
        if ((rc = dev_tri_scratch_locked(h, m, &V, &recs))) return rc;
        const dim3 grid_t(blocks_for(m.n_tris * 64, 256));
        hipLaunchKernelGGL(k_dev_verts, dim3(blocks_for(m.n_verts, 256)), dim3(256), 0, h->stream, p, (const uint8_t*)m.verts, V);
        hipLaunchKernelGGL(k_dev_tris<false>, grid_t, dim3(256), 0, h->stream, g, p, m.tris, V, rs.ub_key, recs, d_ctr, (uint64_t*)nullptr, (uint64_t)0);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(h_ctr, d_ctr, DC_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const uint64_t np = h_ctr[DC_PAIRS];
        if (np) {
            // the pair list is the one buffer whose size the caller cannot foresee: failing to get it is a capacity answer, and the
            // handle's tables were not touched, so it stays usable
            if (np > 0xFFFFFFFEull)
                return fail(h, HFPF_ERR_CAPACITY, "compare_mesh: %llu (triangle, brick) pairs exceed the 32-bit pair index", (unsigned long long)np);
            if (scratch(h, h->dev_pairs, ScratchLayout().add(&pairs_in, np).add(&pairs, np)) != HFPF_OK) {  // the pairs as emitted, then sorted
                (void)hipGetLastError();
                return fail(h, HFPF_ERR_CAPACITY, "compare_mesh: no device memory for %llu (triangle, brick) pairs", (unsigned long long)np);
            }
            hipLaunchKernelGGL(k_dev_tris<true>, grid_t, dim3(256), 0, h->stream, g, p, m.tris, V, rs.ub_key, recs, d_ctr, pairs_in, np);
            HIPCHK(h, hipGetLastError());
            if ((rc = sort_keys_u64(h, pairs_in, pairs, np, 32 + bits_for_count(nb)))) return rc;
            hipLaunchKernelGGL(k_dev_tri_ranges, dim3(blocks_for(np, 256)), dim3(256), 0, h->stream, pairs, (uint32_t)np, (uint32_t)nb, rs.trange, rs.trange + n);
            HIPCHK(h, hipGetLastError());
        }
    }
    if (n)
        hipLaunchKernelGGL(k_dev_rows, dim3((unsigned)nb), dim3(256), 0, h->stream, rs.rows, rs.sorted_row, rs.ub_start, rs.trange, rs.trange + n, pairs, recs, p.md2,
                           (uint32_t)p.tile, out, &rs.counters->sum);
    return HFPF_OK;
}

// Validated arguments in, the mesh on the device, under the lock.  The row set; then (timed as kernel id 7) the row side and the mesh
// side into *out (the rows -- absent without want_rows; the host form takes them from the row set --, the deviations; empty without
// rows), and the read-back of the summary.
static int compare_locked(hfpf_handle* h, const hfpf_deviation_opts* o, const MeshRef& m, const double* pose, bool on_device, bool want_rows, ResultSet* out,
                          hfpf_deviation_summary* summary)
{
    int rc;
    RowSet rows;
    const ExtractOpts opt{o->min_count, -1, 0};  // the compare of hfpf_extract_filtered, 0 keeps all
    if ((rc = build_rows_locked(h, h->t.stats, opt, &rows))) return rc;
    DevRowSide rs;
    if ((rc = compare_row_scratch_locked(h, rows, "compare_mesh", &rs))) return rc;
    const uint32_t n = rs.n;
    Timed timed(h);
    if (timed.rc) return timed.rc;
    if ((rc = compare_row_side_locked(h, &rs))) return rc;
    ResultSet set;
    if (n) {
        set.add((size_t)n * sizeof(Row), !want_rows, rows.rows);
        set.add((size_t)n * sizeof(Deviation));
        if ((rc = result_alloc(h, set, on_device, "compare_mesh"))) return rc;
    }
    unsigned long long h_ctr[DC_WORDS];
    if ((rc = compare_mesh_side_locked(h, rs, o, m, pose, (Deviation*)set.a[1].dev, h_ctr))) return rc;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) rc = timed.file(kTimeCompare);
    if (e == hipSuccess && !rc && on_device && want_rows && n) e = hipMemcpyAsync(set.a[0].dev, rows.rows, (size_t)n * sizeof(Row), hipMemcpyDeviceToDevice, h->stream);
    DevSummary hs;
    if (e == hipSuccess && !rc) e = hipMemcpyAsync(&hs, &rs.counters->sum, sizeof hs, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && !rc) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess || rc) return rc ? rc : fail(h, HFPF_ERR_HIP, "compare_mesh: %s", hipGetErrorString(e));
    memset(summary, 0, sizeof *summary);
    summary->n_rows = rows.n, summary->n_found = hs.n_found, summary->n_negative = hs.n_negative;
    summary->n_tris_invalid = h_ctr[DC_INVALID], summary->n_tris_valid = m.n_tris - h_ctr[DC_INVALID];
    memcpy(&summary->max_abs, &hs.max_abs_bits, 4);
    summary->sum_abs_q30 = hs.sum_abs_q30, summary->sum_sq_q30 = hs.sum_sq_q30;
    set.keep(out);
    return HFPF_OK;
}

// The checks on a mesh and its pose that compare, align and cover share.  0 = fine, else the text of the fault.
static const char* mesh_args_fault(const MeshRef& m, const double* pose)
{
    if (!pose) return "NULL pose";
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(pose[i])) return "non-finite pose";
    if (m.stride < 12 || (m.stride & 3)) return "vertex_stride must be at least 12 and a multiple of 4";
    if ((!m.verts && m.n_verts) || (!m.tris && m.n_tris)) return "NULL mesh pointer with a non-zero count";
    if (m.n_verts >= 0xFFFFFFFFull || m.n_tris >= 0xFFFFFFFFull) return "n_verts and n_tris must stay below 2^32 - 1";
    return nullptr;
}
static bool mesh_misaligned(const MeshRef& m) { return ((((uintptr_t)m.verts) | ((uintptr_t)m.tris)) & 3) != 0; }

// The checks of both forms that need the handle but not the device.  0 = fine, else the text of the fault.
static const char* compare_args_fault(const hfpf_handle* h, const hfpf_deviation_opts* o, const MeshRef& m, const double* pose, const void* dev, const void* n_rows,
                                      const void* summary, bool on_device)
{
    if (hfpf_check_deviation_opts(o) != HFPF_OK) return "invalid hfpf_deviation_opts";
    if (o->max_distance > 32.0 * h->g.res) return "max_distance exceeds 32 voxels";
    if (const char* f = mesh_args_fault(m, pose)) return f;
    if (!dev || !n_rows || !summary) return "NULL dev, n_rows or summary";
    if (on_device && mesh_misaligned(m)) return "device mesh pointers must be 4-byte aligned";
    return nullptr;
}

// The host forms' mesh to the device (h->dev_mesh, *dev): the vertices as they are (stride and all), the indices behind them at a
// 16-byte boundary.
static int upload_mesh_locked(hfpf_handle* h, const char* what, const MeshRef& host, MeshRef* dev)
{
    const uint64_t v_bytes = host.n_verts ? (host.n_verts - 1) * host.stride + 12 : 0;
    uint8_t* d_verts; uint32_t* d_tris;
    // (16 spare bytes behind the indices: the request is part of the recorded device_bytes)
    if (int rc = scratch(h, h->dev_mesh, ScratchLayout().add(&d_verts, v_bytes, 16).add(&d_tris, 3 * host.n_tris).skip(16))) return rc;
    hipError_t e = v_bytes ? upload_pageable(h, d_verts, host.verts, v_bytes) : hipSuccess;
    if (e == hipSuccess && host.n_tris) e = upload_pageable(h, d_tris, host.tris, host.n_tris * 12);
    if (e != hipSuccess) return fail(h, HFPF_ERR_HIP, "%s upload: %s", what, hipGetErrorString(e));
    *dev = MeshRef{d_verts, host.n_verts, host.stride, d_tris, host.n_tris};
    return HFPF_OK;
}

// The mesh input of both forms (*d): the caller's device mesh where it is, the caller's host mesh through upload_mesh_locked.
static int mesh_on_device_locked(hfpf_handle* h, const char* what, const MeshRef& m, bool on_device, MeshRef* d)
{
    if (!on_device) return upload_mesh_locked(h, what, m, d);
    *d = m;
    return HFPF_OK;
}

// A fault in the arguments of the calls that take a mesh: "<name>: <fault>", from the device form "<name>_device: <fault>".
static int args_fail(hfpf_handle* h, const char* name, bool on_device, const char* fault)
{
    return fail(h, HFPF_ERR_BAD_ARG, "%s%s: %s", name, on_device ? "_device" : "", fault);
}

// A mesh without triangles is a mesh like any other here: the host form uploads it (the scratch request shows in device_bytes) and
// the call runs with it.  Without rows the set stays empty: NULL arrays beside the summary, no download.
static int compare_common(hfpf_handle* h, const hfpf_deviation_opts* o, const void* verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* tris,
                          uint64_t n_tris, const double* pose, bool on_device, hfpf_row** rows, hfpf_deviation** dev, uint64_t* n_rows,
                          hfpf_deviation_summary* summary)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    const MeshRef m{verts, n_verts, vertex_stride, tris, n_tris};
    if (const char* f = compare_args_fault(h, o, m, pose, dev, n_rows, summary, on_device)) return args_fail(h, "compare_mesh", on_device, f);
    MeshRef d;
    ResultSet set;
    hfpf_deviation_summary s;
    void* out[kResultArrays];
    int rc;
    if ((rc = local_read_prologue_locked(h, "compare_mesh")) || (rc = mesh_on_device_locked(h, "compare_mesh", m, on_device, &d))) return rc;
    if ((rc = compare_locked(h, o, d, pose, on_device, rows != nullptr, &set, &s)) || (rc = result_deliver(h, set, on_device, "compare_mesh", out))) return rc;
    if (rows) *rows = (hfpf_row*)out[0];
    *dev = (hfpf_deviation*)out[1], *n_rows = s.n_rows, *summary = s;
    return HFPF_OK;
}

int hfpf_compare_mesh_device(hfpf_handle* h, const hfpf_deviation_opts* o, const void* dev_verts, uint64_t n_verts, uint32_t vertex_stride,
                             const uint32_t* dev_tris, uint64_t n_tris, const double* pose_3x4, hfpf_row** dev_rows, hfpf_deviation** dev_dev,
                             uint64_t* n_rows, hfpf_deviation_summary* summary)
{
    return compare_common(h, o, dev_verts, n_verts, vertex_stride, dev_tris, n_tris, pose_3x4, true, dev_rows, dev_dev, n_rows, summary);
}

int hfpf_compare_mesh(hfpf_handle* h, const hfpf_deviation_opts* o, const void* verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* tris,
                      uint64_t n_tris, const double* pose_3x4, hfpf_row** rows, hfpf_deviation** dev, uint64_t* n_rows, hfpf_deviation_summary* summary)
{
    return compare_common(h, o, verts, n_verts, vertex_stride, tris, n_tris, pose_3x4, false, rows, dev, n_rows, summary);
}

void hfpf_free_deviation(hfpf_row* rows, hfpf_deviation* dev)
{
    free(rows);
    free(dev);
}

// ---- best-fitting a mesh to the model (include/hfpf.h) ----------------------------------------------------------------------
int hfpf_check_align_opts(const hfpf_align_opts* o)
{
    if (!o || o->struct_size != sizeof(hfpf_align_opts) || (o->flags & ~HFPF_ALIGN_SKIP_BOUNDARY) || o->reserved0 != 0 || o->reserved != 0) return HFPF_ERR_BAD_ARG;
    if (!refine_opts_ok(o, 65536)) return HFPF_ERR_BAD_ARG;
    return hfpf_check_deviation_opts(&o->compare);
}

// Validated arguments in, the mesh on the device, under the lock.  The row set; then compare's row side once and refine_pose with
// compare's mesh side into h->align_dev and one k_align_reduce per iteration.  Not timed: hfpf_get_kernel_time has no id for it.
static int align_locked(hfpf_handle* h, const hfpf_align_opts* o, const MeshRef& m, const double* pose, hfpf_align_result* res)
{
    int rc;
    RowSet rows;
    const ExtractOpts opt{o->compare.min_count, -1, 0};
    if ((rc = build_rows_locked(h, h->t.stats, opt, &rows))) return rc;
    const uint64_t n_samples = (rows.n + o->stride - 1) / o->stride;
    if (n_samples > (1ull << 26)) return fail(h, HFPF_ERR_BAD_ARG, "align_mesh: more than 2^26 sampled rows");
    DevRowSide rs;
    if ((rc = compare_row_scratch_locked(h, rows, "align_mesh", &rs))) return rc;
    Deviation* dev; if ((rc = scratch_n(h, h->align_dev, std::max<uint32_t>(rs.n, 1), &dev))) return rc;
    AlignParams p{};
    for (int a = 0; a < 3; a++) p.c[a] = (h->g.min[a] + h->g.max[a]) * 0.5;
    p.flags = o->flags, p.stride = o->stride, p.n = (uint32_t)n_samples;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(kTrackMaxBlocks, blocks_for(n_samples, 256));

    if ((rc = compare_row_side_locked(h, &rs))) return rc;
    uint64_t none;
    rc = refine_pose(h, o, p.c, kAlignTerms, pose, [&](const double* T, unsigned long long* acc) -> int {
        unsigned long long h_ctr[DC_WORDS];
        if (int e = compare_mesh_side_locked(h, rs, &o->compare, m, T, dev, h_ctr)) return e;
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemsetAsync(acc, 0, kAlignTerms * sizeof(unsigned long long), h->stream));
        if (n_samples) {  // without rows the zeros are read back: TOO_FEW
            hipLaunchKernelGGL(k_align_reduce, dim3(blocks), dim3(256), 0, h->stream, p, rows.rows, dev, acc);
            HIPCHK(h, hipGetLastError());
        }
        return HFPF_OK;
    }, res, &none);
    if (!rc) res->rows_sampled = n_samples;
    return rc;
}

// The checks of both forms: the options, then compare's own on the mesh, the pose and max_distance, then the result.
static const char* align_args_fault(const hfpf_handle* h, const hfpf_align_opts* o, const MeshRef& m, const double* pose, const hfpf_align_result* res, bool on_device)
{
    if (hfpf_check_align_opts(o) != HFPF_OK) return "invalid hfpf_align_opts";
    if (const char* f = compare_args_fault(h, &o->compare, m, pose, h, h, h, on_device)) return f;
    if (!res || res->struct_size != sizeof(hfpf_align_result)) return "NULL result or wrong struct_size";
    return nullptr;
}

// As in a compare, a mesh without triangles is uploaded and run.  No arrays: align_locked writes *result last, once the fit has ended.
static int align_common(hfpf_handle* h, const hfpf_align_opts* o, const void* verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* tris, uint64_t n_tris,
                        const double* pose, bool on_device, hfpf_align_result* result)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    const MeshRef m{verts, n_verts, vertex_stride, tris, n_tris};
    if (const char* f = align_args_fault(h, o, m, pose, result, on_device)) return args_fail(h, "align_mesh", on_device, f);
    MeshRef d;
    int rc;
    if ((rc = local_read_prologue_locked(h, "align_mesh")) || (rc = mesh_on_device_locked(h, "align_mesh", m, on_device, &d))) return rc;
    return align_locked(h, o, d, pose, result);
}

int hfpf_align_mesh_device(hfpf_handle* h, const hfpf_align_opts* o, const void* dev_verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* dev_tris,
                           uint64_t n_tris, const double* pose_3x4, hfpf_align_result* result)
{
    return align_common(h, o, dev_verts, n_verts, vertex_stride, dev_tris, n_tris, pose_3x4, true, result);
}

int hfpf_align_mesh(hfpf_handle* h, const hfpf_align_opts* o, const void* verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* tris, uint64_t n_tris,
                    const double* pose_3x4, hfpf_align_result* result)
{
    return align_common(h, o, verts, n_verts, vertex_stride, tris, n_tris, pose_3x4, false, result);
}

// ---- coverage of a triangle mesh by the model (include/hfpf.h) ----------------------------------------------------------------
int hfpf_check_cover_opts(const hfpf_cover_opts* o)
{
    if (!o || o->struct_size != sizeof(hfpf_cover_opts) || (o->flags & ~HFPF_COVER_ABS_NORMAL) || o->reserved != 0) return HFPF_ERR_BAD_ARG;
    if (o->radius < 1 || o->radius > kQueryMaxRadius || o->max_subdivision < 1 || o->max_subdivision > 64 || std::isnan(o->min_count)) return HFPF_ERR_BAD_ARG;
    if (!(std::isfinite(o->max_distance) && o->max_distance > 0.0 && o->max_distance <= 1.0)) return HFPF_ERR_BAD_ARG;
    if (!(std::isfinite(o->spacing) && o->spacing > 0.0)) return HFPF_ERR_BAD_ARG;
    return std::isfinite(o->min_normal_dot) && o->min_normal_dot >= -2.0 && o->min_normal_dot <= 1.0 ? HFPF_OK : HFPF_ERR_BAD_ARG;
}

struct CovCounters {  // zeroed together in front of the setup
    CovSummary sum;
    unsigned long long total;  // samples of all triangles
};
static_assert(sizeof(CovCounters) == sizeof(CovSummary) + 8, "the summary and the total are adjacent");

// The samples of a cover as hfpf_plan_views* meets them again.
struct CovSamples {
    CovTri* geo;       // per triangle
    uint32_t* offset;  // n_tris + 1
    uint32_t* target;  // total + 1: 1 = IN_BBOX and not COVERED (the last word 0, for the scan); NULL without samples
    uint64_t total;
};

// Validated arguments in, the mesh on the device, n_tris > 0, under the lock.  The transformed vertices (compare's kernel); per
// triangle a record, the geometry and a sample count; the scan of the counts; one lane per sample; per triangle its share of the
// summary.  The 64-bit total is read back once in front of the scan (whose 32-bit total cannot tell an overflow): the capacity
// check and the size of the sample launch.  cov: room for the n_tris records.  keep != NULL (hfpf_plan_views*): the samples are also
// marked as targets (k_cov_samples<true>) and *keep describes them.  Not timed: hfpf_get_kernel_time has no id for it.
static int cover_run_locked(hfpf_handle* h, const hfpf_cover_opts* o, const MeshRef& m, const double* pose, TriCoverage* cov, hfpf_coverage_summary* summary,
                            CovSamples* keep)
{
    int rc;
    const uint64_t n_tris = m.n_tris, T1 = n_tris + 1;
    double* V; CovTri* geo; CovCounters* ctr;
    uint32_t *count, *offset;  // per triangle (n_tris + 1 entries each): the sample count and its scan
    if ((rc = dev_tri_scratch_locked(h, m, &V, &geo)) || (rc = scratch(h, h->cov_bins, ScratchLayout().add(&ctr, 1).add(&count, T1).add(&offset, T1)))) return rc;
    CovSummary* d_sum = &ctr->sum;
    unsigned long long* d_total = &ctr->total;
    DevParams vp{};  // what k_dev_verts reads of it
    memcpy(vp.T, pose, sizeof vp.T);
    vp.n_verts = m.n_verts, vp.n_tris = (uint32_t)n_tris, vp.stride = m.stride;
    CovParams p{};
    p.spacing = o->spacing, p.min_count = std::max(1.0, o->min_count), p.max_d2 = o->max_distance * o->max_distance, p.min_dot = o->min_normal_dot;
    p.n_verts = m.n_verts, p.n_tris = (uint32_t)n_tris, p.max_sub = o->max_subdivision;
    p.abs_normal = (o->flags & HFPF_COVER_ABS_NORMAL) ? 1u : 0u, p.radius = o->radius;
    hipError_t e = hipMemsetAsync(ctr, 0, sizeof(CovCounters), h->stream);
    if (e != hipSuccess) return fail(h, HFPF_ERR_HIP, "cover_mesh: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_dev_verts, dim3(blocks_for(m.n_verts, 256)), dim3(256), 0, h->stream, vp, (const uint8_t*)m.verts, V);
    hipLaunchKernelGGL(k_cov_setup, dim3(blocks_for(T1, 256)), dim3(256), 0, h->stream, p, m.tris, V, cov, geo, count, d_total);
    unsigned long long total = 0;
    if ((e = hipGetLastError()) == hipSuccess) e = hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, HFPF_ERR_HIP, "cover_mesh: %s", hipGetErrorString(e));
    if (total > 0xFFFFFFFEull)  // nothing on the handle was touched: it stays usable
        return fail(h, HFPF_ERR_CAPACITY, "cover_mesh: %llu samples exceed the 2^32 - 2 a call takes (a larger spacing or a smaller max_subdivision)", total);
    if (total) {
        uint64_t scanned = 0;
        if ((rc = scan_counts_locked(h, count, offset, n_tris, &scanned))) return rc;
        if (scanned != total) return fail(h, HFPF_ERR_STATE, "cover_mesh: the scan of the sample counts disagrees with their sum (internal)");
        if (keep) {
            if ((rc = scratch_n(h, h->plan_mark, total + 1, &keep->target))) return rc;
            HIPCHK(h, hipMemsetAsync(keep->target + total, 0, 4, h->stream));
            hipLaunchKernelGGL(k_cov_samples<true>, dim3(blocks_for(total, 256)), dim3(256), 0, h->stream, h->g, h->t, p, offset, geo, (uint32_t)total, cov,
                               keep->target);
        } else {
            hipLaunchKernelGGL(k_cov_samples<false>, dim3(blocks_for(total, 256)), dim3(256), 0, h->stream, h->g, h->t, p, offset, geo, (uint32_t)total, cov,
                               (uint32_t*)nullptr);
        }
    }
    if (keep) keep->geo = geo, keep->offset = offset, keep->total = total;
    hipLaunchKernelGGL(k_cov_finish, dim3(blocks_for(n_tris, 256)), dim3(256), 0, h->stream, (uint32_t)n_tris, cov, geo, d_sum);
    CovSummary hs;
    if ((e = hipGetLastError()) == hipSuccess) e = hipMemcpyAsync(&hs, d_sum, sizeof hs, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, HFPF_ERR_HIP, "cover_mesh: %s", hipGetErrorString(e));
    static_assert(sizeof(CovSummary) == sizeof(hfpf_coverage_summary), "the device summary is the public one, max_distance as bits");
    memcpy(summary, &hs, sizeof hs);
    return HFPF_OK;
}

// A cover into records of its own.  *out: the n_tris records.
static int cover_locked(hfpf_handle* h, const hfpf_cover_opts* o, const MeshRef& m, const double* pose, bool on_device, ResultSet* out, hfpf_coverage_summary* summary)
{
    ResultSet set;
    set.add((size_t)m.n_tris * sizeof(TriCoverage));
    if (int rc = result_alloc(h, set, on_device, "cover_mesh")) return rc;
    if (int rc = cover_run_locked(h, o, m, pose, (TriCoverage*)set.a[0].dev, summary, nullptr)) return rc;
    set.keep(out);
    return HFPF_OK;
}

// The checks of both forms.  0 = fine, else the text of the fault.
static const char* cover_args_fault(const hfpf_cover_opts* o, const MeshRef& m, const double* pose, const void* cov, const void* summary, bool on_device)
{
    if (hfpf_check_cover_opts(o) != HFPF_OK) return "invalid hfpf_cover_opts";
    if (const char* f = mesh_args_fault(m, pose)) return f;
    if (!cov || !summary) return "NULL cov or summary";
    if (on_device && mesh_misaligned(m)) return "device mesh pointers must be 4-byte aligned";
    return nullptr;
}

// A mesh without triangles is answered here, in front of any upload or scratch request: a zeroed summary and a NULL cov.
static int cover_common(hfpf_handle* h, const hfpf_cover_opts* o, const void* verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* tris, uint64_t n_tris,
                        const double* pose, bool on_device, hfpf_tri_coverage** cov, hfpf_coverage_summary* summary)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    const MeshRef m{verts, n_verts, vertex_stride, tris, n_tris};
    if (const char* f = cover_args_fault(o, m, pose, cov, summary, on_device)) return args_fail(h, "cover_mesh", on_device, f);
    MeshRef d;
    ResultSet set;
    hfpf_coverage_summary s{};
    void* out[kResultArrays];
    int rc;
    if ((rc = local_read_prologue_locked(h, "cover_mesh"))) return rc;
    if (n_tris && (rc = mesh_on_device_locked(h, "cover_mesh", m, on_device, &d))) return rc;
    if (n_tris && (rc = cover_locked(h, o, d, pose, on_device, &set, &s))) return rc;
    if ((rc = result_deliver(h, set, on_device, "cover_mesh", out))) return rc;
    *cov = (hfpf_tri_coverage*)out[0], *summary = s;
    return HFPF_OK;
}

int hfpf_cover_mesh_device(hfpf_handle* h, const hfpf_cover_opts* o, const void* dev_verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* dev_tris,
                           uint64_t n_tris, const double* pose_3x4, hfpf_tri_coverage** dev_cov, hfpf_coverage_summary* summary)
{
    return cover_common(h, o, dev_verts, n_verts, vertex_stride, dev_tris, n_tris, pose_3x4, true, dev_cov, summary);
}

int hfpf_cover_mesh(hfpf_handle* h, const hfpf_cover_opts* o, const void* verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* tris, uint64_t n_tris,
                    const double* pose_3x4, hfpf_tri_coverage** cov, hfpf_coverage_summary* summary)
{
    return cover_common(h, o, verts, n_verts, vertex_stride, tris, n_tris, pose_3x4, false, cov, summary);
}

void hfpf_free_coverage(hfpf_tri_coverage* cov) { free(cov); }

// ---- planar sections of a mesh (include/hfpf.h) -------------------------------------------------------------------------------------
int hfpf_check_section_opts(const hfpf_section_opts* o)
{
    return o && o->struct_size == sizeof(hfpf_section_opts) && o->flags == 0 && o->reserved == 0 ? HFPF_OK : HFPF_ERR_BAD_ARG;
}

static_assert(sizeof(SecPoint) == sizeof(hfpf_section_point) && sizeof(SecSegment) == sizeof(hfpf_section_segment) &&
                  sizeof(SecContour) == sizeof(hfpf_section_contour) && sizeof(SecPlane) == sizeof(hfpf_section_plane),
              "the device records are the public ones");
static_assert(kSecMaxPlanes == HFPF_SECTION_MAX_PLANES && kSecPlaneCap == HFPF_SECTION_MAX_PLANE_SEGMENTS, "host_plan.hpp restates the header's limits");

struct SectionCounts {
    uint64_t n_points = 0, n_segments = 0, n_contours = 0;
};

// Validated arguments in, the mesh on the device, n_tris > 0, under the lock.  The transformed vertices (compare's kernel); the count
// pass over every chunk of planes; the read-back of the per-plane counts (the cap test, the bases and the size of everything behind);
// the emit pass; the two sorts and the unique; points, links, flatten, the scan of the root flags (the number of contours: only now
// can the three result arrays be sized, so the kernels behind write every record once and whole); label, measure, finish; the
// read-back of the plane records.  *out, *nout, *recs (n_planes records) and *S are section_common's locals, empty and zeroed.  Not
// timed: hfpf_get_kernel_time has no id for it (tools/section_rate.py times it with events of its own).
static int section_locked(hfpf_handle* h, const MeshRef& m, const double* pose, const double* planes, uint32_t n_planes, bool on_device, ResultSet* out,
                          SectionCounts* nout, std::vector<hfpf_section_plane>* recs, hfpf_section_summary* S)
{
    int rc;
    const uint64_t P1 = (uint64_t)n_planes + 1;
    double* V; SecCounters* ctr; double* d_planes; SecPlane* d_recs;
    uint32_t *count, *first;  // per plane (n_planes + 1 entries each): the crossings (later the emit pass's cursor) and their exclusive sums
    if ((rc = scratch_n(h, h->dev_tri, 3 * std::max<uint64_t>(m.n_verts, 1), &V))) return rc;
    if ((rc = scratch(h, h->sec_ctr, ScratchLayout().add(&ctr, 1).add(&d_planes, 4 * P1).add(&d_recs, P1).add(&count, P1).add(&first, P1)))) return rc;
    HIPCHK(h, hipMemsetAsync(ctr, 0, sizeof(SecCounters), h->stream));
    HIPCHK(h, hipMemsetAsync(count, 0, P1 * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(d_recs, 0, P1 * sizeof(SecPlane), h->stream));
    if (n_planes) HIPCHK(h, hipMemcpyAsync(d_planes, planes, (size_t)n_planes * 32, hipMemcpyHostToDevice, h->stream));
    DevParams vp{};  // what k_dev_verts reads of it
    memcpy(vp.T, pose, sizeof vp.T);
    vp.n_verts = m.n_verts, vp.n_tris = (uint32_t)m.n_tris, vp.stride = m.stride;
    SecParams p{};
    for (int a = 0; a < 3; a++) p.c[a] = (h->g.min[a] + h->g.max[a]) * 0.5;
    p.n_verts = m.n_verts, p.n_tris = (uint32_t)m.n_tris;
    const uint32_t n_chunks = section_chunks(n_planes);
    const dim3 grid_t(section_grid(m.n_tris));
    hipLaunchKernelGGL(k_dev_verts, dim3(blocks_for(m.n_verts, 256)), dim3(256), 0, h->stream, vp, (const uint8_t*)m.verts, V);
    for (uint32_t c = 0; c < n_chunks; c++) {
        p.plane0 = c * kSecChunkPlanes, p.np = section_chunk_planes(n_planes, c), p.count_tris = c == 0 ? 1u : 0u;
        hipLaunchKernelGGL(k_section<false>, grid_t, dim3(256), 0, h->stream, p, m.tris, V, d_planes, count, (const uint32_t*)nullptr, (uint64_t*)nullptr,
                           (uint32_t*)nullptr, (uint64_t*)nullptr, ctr);
    }
    HIPCHK(h, hipGetLastError());
    SecCounters hc;
    std::vector<uint32_t> h_count(P1, 0u);
    HIPCHK(h, hipMemcpyAsync(&hc, ctr, sizeof hc, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(h_count.data(), count, P1 * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<uint64_t> first64(P1, 0);
    const SecCapFault cap = section_cap_test(h_count.data(), n_planes, first64.data());
    if (cap.over) {  // nothing on the handle was touched: it stays usable
        if (cap.plane < n_planes)
            return fail(h, HFPF_ERR_CAPACITY, "section_mesh: plane %u has %llu segments, more than the 2^20 a plane may have", cap.plane, (unsigned long long)cap.count);
        return fail(h, HFPF_ERR_CAPACITY, "section_mesh: %llu segments in all exceed the 2^31 - 1 a call takes", (unsigned long long)cap.count);
    }
    S->n_tris_valid = hc.n_valid, S->n_tris_invalid = hc.n_invalid, S->n_tris_far = hc.n_far;
    const uint64_t ns = cap.count;
    if (ns == 0) return HFPF_OK;
    std::vector<uint32_t> first32(P1);
    for (uint64_t j = 0; j < P1; j++) first32[j] = (uint32_t)first64[j];
    HIPCHK(h, hipMemcpyAsync(first, first32.data(), P1 * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(count, 0, P1 * 4, h->stream));
    uint64_t *seg_in, *seg_out, *pk, *pk_sorted, *pk_unique, *ucount;
    uint32_t *val_in, *val_out;
    if ((rc = scratch(h, h->sec_keys, ScratchLayout().add(&seg_in, ns).add(&seg_out, ns).add(&pk, 2 * ns).add(&pk_sorted, 2 * ns).add(&pk_unique, 2 * ns)
                                          .add(&ucount, 1).add(&val_in, ns).add(&val_out, ns))))
        return rc;
    // (an append that the count pass did not announce would leave a hole: all ones sort behind every key and fail k_sec_link's test)
    HIPCHK(h, hipMemsetAsync(val_in, 0xFF, ns * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(seg_in, 0xFF, ns * 8, h->stream));
    HIPCHK(h, hipMemsetAsync(pk, 0xFF, 2 * ns * 8, h->stream));
    p.n_total = (uint32_t)ns;
    for (uint32_t c = 0; c < n_chunks; c++) {
        p.plane0 = c * kSecChunkPlanes, p.np = section_chunk_planes(n_planes, c), p.count_tris = 0;
        hipLaunchKernelGGL(k_section<true>, grid_t, dim3(256), 0, h->stream, p, m.tris, V, d_planes, count, first, seg_in, val_in, pk, ctr);
    }
    HIPCHK(h, hipGetLastError());
    if ((rc = sort_pairs_u64(h, seg_in, seg_out, val_in, val_out, ns, kSecSegKeyBits))) return rc;
    if ((rc = sort_keys_u64(h, pk, pk_sorted, 2 * ns, kSecPointKeyBits))) return rc;
    uint64_t np = 0;
    if ((rc = unique_keys_locked(h, pk_sorted, 2 * ns, pk_unique, ucount, &np))) return rc;
    if (np == 0 || np > 2 * ns) return fail(h, HFPF_ERR_STATE, "section_mesh: %llu points from %llu segments (internal)", (unsigned long long)np, (unsigned long long)ns);
    const uint64_t N1 = np + 1;
    double* Pd;
    uint32_t *parent, *root, *flag, *cbase, *deg_out, *deg_in;
    if ((rc = scratch(h, h->sec_data, ScratchLayout().add(&Pd, 3 * np).add(&parent, N1).add(&root, N1).add(&flag, N1).add(&cbase, N1).add(&deg_out, N1)
                                          .add(&deg_in, N1))))
        return rc;
    const dim3 grid_p(blocks_for(np, 256)), grid_p1(blocks_for(N1, 256)), grid_s(blocks_for(ns, 256));
    uint64_t* seg_ends = seg_in;  // the unsorted segment keys are dead behind their sort
    hipLaunchKernelGGL(k_sec_points, grid_p, dim3(256), 0, h->stream, pk_unique, (uint32_t)np, d_planes, n_planes, V, m.n_verts, Pd, parent, deg_out, deg_in);
    hipLaunchKernelGGL(k_sec_link, grid_s, dim3(256), 0, h->stream, val_out, (uint32_t)ns, pk, pk_unique, (uint32_t)np, seg_ends, parent, deg_out, deg_in);
    hipLaunchKernelGGL(k_comp_flatten, grid_p1, dim3(256), 0, h->stream, parent, (uint32_t)np, root, flag);
    HIPCHK(h, hipGetLastError());
    uint64_t nc = 0;
    if ((rc = scan_counts_locked(h, flag, cbase, np, &nc))) return rc;
    if (nc == 0) return fail(h, HFPF_ERR_STATE, "section_mesh: no contour for %llu points (internal)", (unsigned long long)np);
    ResultSet set;
    set.add(np * sizeof(SecPoint));
    set.add(ns * sizeof(SecSegment));
    set.add(nc * sizeof(SecContour));
    if ((rc = result_alloc(h, set, on_device, "section_mesh"))) return rc;
    SecPoint* pts = (SecPoint*)set.a[0].dev;
    SecSegment* segs = (SecSegment*)set.a[1].dev;
    SecContour* conts = (SecContour*)set.a[2].dev;
    HIPCHK(h, hipMemsetAsync(conts, 0, nc * sizeof(SecContour), h->stream));
    hipLaunchKernelGGL(k_sec_label, grid_p, dim3(256), 0, h->stream, root, cbase, (uint32_t)np, pk_unique, Pd, deg_out, deg_in, pts, conts);
    hipLaunchKernelGGL(k_sec_measure, grid_s, dim3(256), 0, h->stream, seg_out, seg_ends, (uint32_t)ns, d_planes, pts, Pd, segs, conts);
    hipLaunchKernelGGL(k_sec_finish, dim3(blocks_for(nc, 256)), dim3(256), 0, h->stream, (uint32_t)nc, conts, d_recs, &ctr->n_closed);
    HIPCHK(h, hipGetLastError());
    static_assert(sizeof(SecPlane) == sizeof(hfpf_section_plane), "the device plane record is the public one");
    if (n_planes) HIPCHK(h, hipMemcpyAsync(recs->data(), d_recs, (size_t)n_planes * sizeof(SecPlane), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&hc, ctr, sizeof hc, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    uint64_t fs = 0, fp = 0, fc = 0;
    for (hfpf_section_plane& r : *recs) {  // the planes before it, also for a plane that has nothing
        r.first_segment = (uint32_t)fs, r.first_point = (uint32_t)fp, r.first_contour = (uint32_t)fc;
        fs += r.n_segments, fp += r.n_points, fc += r.n_contours;
    }
    if (fs != ns || fp != np || fc != nc) return fail(h, HFPF_ERR_STATE, "section_mesh: the plane records do not add up to the arrays (internal)");
    S->n_segments = ns, S->n_points = np, S->n_contours = nc, S->n_closed = hc.n_closed;
    nout->n_points = np, nout->n_segments = ns, nout->n_contours = nc;
    set.keep(out);
    return HFPF_OK;
}

// The checks of both forms, all of them before anything is read through a mesh pointer.  0 = fine, else the text of the fault.
static const char* section_args_fault(const hfpf_section_opts* o, const MeshRef& m, const double* pose, const double* planes, uint32_t n_planes,
                                      const void* const outs[8], bool on_device)
{
    if (hfpf_check_section_opts(o) != HFPF_OK) return "invalid hfpf_section_opts";
    if (const char* f = mesh_args_fault(m, pose)) return f;
    if (const char* f = section_counts_fault(m.n_verts, m.n_tris, n_planes)) return f;
    if (!planes && n_planes) return "NULL planes with a non-zero count";
    if (section_first_bad_plane(planes, n_planes) != n_planes) return "a plane with a non-finite value or a normal of no finite length > 0";
    for (int i = 0; i < 7; i++)
        if (!outs[i]) return "NULL output pointer";
    if (!outs[7] && n_planes) return "NULL plane records with a non-zero count";
    if (on_device && mesh_misaligned(m)) return "device mesh pointers must be 4-byte aligned";
    return nullptr;
}

// A mesh without triangles is answered here, in front of any upload or scratch request: zeroed records and summary and NULL arrays.
// Without planes, or when no plane meets a triangle, section_locked leaves the set empty: NULL arrays beside the counts, no download.
static int section_common(hfpf_handle* h, const hfpf_section_opts* o, const void* verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* tris, uint64_t n_tris,
                          const double* pose, const double* planes, uint32_t n_planes, bool on_device, hfpf_section_point** points, uint64_t* n_points,
                          hfpf_section_segment** segments, uint64_t* n_segments, hfpf_section_contour** contours, uint64_t* n_contours, hfpf_section_plane* plane_recs,
                          hfpf_section_summary* summary)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    const MeshRef m{verts, n_verts, vertex_stride, tris, n_tris};
    const void* const outs[8] = {points, n_points, segments, n_segments, contours, n_contours, summary, plane_recs};
    if (const char* f = section_args_fault(o, m, pose, planes, n_planes, outs, on_device)) return args_fail(h, "section_mesh", on_device, f);
    MeshRef d;
    ResultSet set;
    SectionCounts n;
    std::vector<hfpf_section_plane> recs(n_planes, hfpf_section_plane{});
    hfpf_section_summary s{};
    void* out[kResultArrays];
    int rc;
    if ((rc = local_read_prologue_locked(h, "section_mesh"))) return rc;
    if (n_tris && (rc = mesh_on_device_locked(h, "section_mesh", m, on_device, &d))) return rc;
    if (n_tris && (rc = section_locked(h, d, pose, planes, n_planes, on_device, &set, &n, &recs, &s))) return rc;
    if ((rc = result_deliver(h, set, on_device, "section_mesh", out))) return rc;
    *points = (hfpf_section_point*)out[0], *segments = (hfpf_section_segment*)out[1], *contours = (hfpf_section_contour*)out[2];
    *n_points = n.n_points, *n_segments = n.n_segments, *n_contours = n.n_contours, *summary = s;
    if (n_planes) memcpy(plane_recs, recs.data(), (size_t)n_planes * sizeof(hfpf_section_plane));
    return HFPF_OK;
}

int hfpf_section_mesh_device(hfpf_handle* h, const hfpf_section_opts* o, const void* dev_verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* dev_tris,
                             uint64_t n_tris, const double* pose_3x4, const double* planes, uint32_t n_planes, hfpf_section_point** dev_points, uint64_t* n_points,
                             hfpf_section_segment** dev_segments, uint64_t* n_segments, hfpf_section_contour** dev_contours, uint64_t* n_contours,
                             hfpf_section_plane* plane_recs, hfpf_section_summary* summary)
{
    return section_common(h, o, dev_verts, n_verts, vertex_stride, dev_tris, n_tris, pose_3x4, planes, n_planes, true, dev_points, n_points, dev_segments, n_segments,
                          dev_contours, n_contours, plane_recs, summary);
}

int hfpf_section_mesh(hfpf_handle* h, const hfpf_section_opts* o, const void* verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* tris, uint64_t n_tris,
                      const double* pose_3x4, const double* planes, uint32_t n_planes, hfpf_section_point** points, uint64_t* n_points,
                      hfpf_section_segment** segments, uint64_t* n_segments, hfpf_section_contour** contours, uint64_t* n_contours, hfpf_section_plane* plane_recs,
                      hfpf_section_summary* summary)
{
    return section_common(h, o, verts, n_verts, vertex_stride, tris, n_tris, pose_3x4, planes, n_planes, false, points, n_points, segments, n_segments, contours,
                          n_contours, plane_recs, summary);
}

void hfpf_free_section(hfpf_section_point* points, hfpf_section_segment* segments, hfpf_section_contour* contours)
{
    free(points);
    free(segments);
    free(contours);
}

// ---- open edges of a mesh: boundary loops, shells, watertightness (include/hfpf.h) ------------------------------------------------------
int hfpf_check_topology_opts(const hfpf_topology_opts* o)
{
    return o && o->struct_size == sizeof(hfpf_topology_opts) && o->flags == 0 && o->reserved == 0 ? HFPF_OK : HFPF_ERR_BAD_ARG;
}

static_assert(sizeof(TopEdge) == sizeof(hfpf_topology_edge) && sizeof(TopLoop) == sizeof(hfpf_topology_loop) && sizeof(TopShell) == sizeof(hfpf_topology_shell),
              "the device records are the public ones");
static_assert(kTopMaxVerts == HFPF_TOPOLOGY_MAX_VERTS && kTopNone == HFPF_TOPOLOGY_NONE && kTopBoundary == HFPF_TOPOLOGY_BOUNDARY &&
                  kTopNonManifold == HFPF_TOPOLOGY_NONMANIFOLD && kTopMiswound == HFPF_TOPOLOGY_MISWOUND,
              "host_plan.hpp restates the header's constants");
static_assert(kTopLoopClosed == HFPF_TOPOLOGY_LOOP_CLOSED && kTopLoopBranched == HFPF_TOPOLOGY_LOOP_BRANCHED && kTopShellOpen == HFPF_TOPOLOGY_SHELL_OPEN &&
                  kTopShellNonManifold == HFPF_TOPOLOGY_SHELL_NONMANIFOLD && kTopShellMiswound == HFPF_TOPOLOGY_SHELL_MISWOUND &&
                  kTopShellWatertight == HFPF_TOPOLOGY_SHELL_WATERTIGHT,
              "kernels.hpp restates the header's flags");

struct TopologyCounts {
    uint64_t n_edges = 0, n_loops = 0, n_shells = 0;
};

// Validated arguments in, the mesh on the device, n_tris > 0, under the lock.  The transformed vertices (compare's kernel); the emit
// pass (half-edges, vertex marks, the shells' forest); flatten and the scan of the root flags (the number of shells, and the read-back
// of the triangle counts); the sort; the run walk (classes, degrees, the loops' forest); the scans of the listed flags and of the
// loops' root flags (only now can the result arrays be sized, so the kernels behind write every record once and whole); the
// reductions per vertex, triangle, edge and listed edge; finish; the read-back of the counters.  *out, *nout and *S are
// topology_common's locals, empty and zeroed.  Not timed: hfpf_get_kernel_time has no id for it (tools/topology_rate.py times it
// with events of its own).
static int topology_locked(hfpf_handle* h, const MeshRef& m, const double* pose, bool on_device, bool want_tri_shell, ResultSet* out, TopologyCounts* nout,
                           hfpf_topology_summary* S)
{
    int rc;
    const uint64_t N1 = m.n_verts + 1, n_slots = 3 * m.n_tris;
    double* V; TopCounters* ctr;
    uint32_t *used, *flag, *base, *deg_out, *deg_in;     // per vertex (n_verts + 1 entries each); flag and base serve the shells, then the loops
    uint32_t *parent_s, *parent_l, *root_s, *root_l;     // the shells' and the loops' forest
    uint64_t *key_in, *key_out;
    uint32_t *val_in, *val_out, *use, *listed, *lbase;   // per half-edge slot (use, listed and lbase: n_slots + 1 entries)
    if ((rc = scratch_n(h, h->dev_tri, 3 * std::max<uint64_t>(m.n_verts, 1), &V))) return rc;
    if ((rc = scratch(h, h->top_verts, ScratchLayout().add(&ctr, 1).add(&used, N1).add(&flag, N1).add(&base, N1).add(&deg_out, N1).add(&deg_in, N1)))) return rc;
    if ((rc = scratch(h, h->top_forest, ScratchLayout().add(&parent_s, N1).add(&parent_l, N1).add(&root_s, N1).add(&root_l, N1)))) return rc;
    if ((rc = scratch(h, h->top_keys, ScratchLayout().add(&key_in, n_slots).add(&key_out, n_slots).add(&val_in, n_slots).add(&val_out, n_slots)
                                          .add(&use, n_slots + 1).add(&listed, n_slots + 1).add(&lbase, n_slots + 1))))
        return rc;
    HIPCHK(h, hipMemsetAsync(ctr, 0, sizeof(TopCounters), h->stream));
    // HFPF_TRACE_TOPOLOGY=1 (read per call, so that tools/topology_rate.py can time untraced calls on the same handle): one stderr
    // line with the host's clock where the stream is drained anyway (and, traced only, in front of the first kernel and behind the sort)
    const char* const trace_env = getenv("HFPF_TRACE_TOPOLOGY");
    const bool trace = trace_env && trace_env[0] != '0';
    double stamp[6] = {0, 0, 0, 0, 0, 0};
    const auto mark = [&](int i) { if (trace) stamp[i] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    if (trace) HIPCHK(h, hipStreamSynchronize(h->stream));
    mark(0);
    DevParams vp{};  // what k_dev_verts reads of it
    memcpy(vp.T, pose, sizeof vp.T);
    vp.n_verts = m.n_verts, vp.n_tris = (uint32_t)m.n_tris, vp.stride = m.stride;
    TopParams p{};
    for (int a = 0; a < 3; a++) p.c[a] = (h->g.min[a] + h->g.max[a]) * 0.5;
    p.n_verts = m.n_verts, p.n_tris = (uint32_t)m.n_tris;
    const uint32_t nv = (uint32_t)m.n_verts;
    const dim3 grid_v(blocks_for(m.n_verts, 256)), grid_v1(blocks_for(N1, 256)), grid_t(blocks_for(m.n_tris, 256));
    hipLaunchKernelGGL(k_top_init, grid_v, dim3(256), 0, h->stream, m.n_verts, parent_s, parent_l, used, deg_out, deg_in);
    hipLaunchKernelGGL(k_dev_verts, grid_v, dim3(256), 0, h->stream, vp, (const uint8_t*)m.verts, V);
    hipLaunchKernelGGL(k_top_emit, grid_t, dim3(256), 0, h->stream, p, m.tris, V, key_in, val_in, used, parent_s, ctr);
    hipLaunchKernelGGL(k_comp_flatten, grid_v1, dim3(256), 0, h->stream, parent_s, nv, root_s, flag);
    hipLaunchKernelGGL(k_top_mask, grid_v, dim3(256), 0, h->stream, flag, used, (const uint32_t*)nullptr, m.n_verts);
    HIPCHK(h, hipGetLastError());
    uint64_t n_shells = 0;
    if ((rc = scan_counts_locked(h, flag, base, m.n_verts, &n_shells))) return rc;
    TopCounters hc;
    HIPCHK(h, hipMemcpy(&hc, ctr, sizeof hc, hipMemcpyDeviceToHost));  // (the scan's read-back has synchronised the stream)
    mark(1);
    S->n_tris_valid = hc.n_valid, S->n_tris_invalid = hc.n_invalid, S->n_tris_far = hc.n_far;
    const uint64_t n_used = hc.n_valid - hc.n_far, n_he = 3 * n_used;
    if (hc.n_far > hc.n_valid || n_used > m.n_tris || (n_used == 0) != (n_shells == 0))
        return fail(h, HFPF_ERR_STATE, "mesh_topology: %llu used triangles in %llu shells (internal)", (unsigned long long)n_used, (unsigned long long)n_shells);
    ResultSet set;
    if (n_used == 0) {  // nothing but the optional per-triangle words, all of them "skipped"
        for (int i = 0; i < 3; i++) set.add(0, true);
        set.add((size_t)m.n_tris * 4, !want_tri_shell);
        if ((rc = result_alloc(h, set, on_device, "mesh_topology"))) return rc;
        if (want_tri_shell) {
            HIPCHK(h, hipMemsetAsync(set.a[3].dev, 0xFF, (size_t)m.n_tris * 4, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
        set.keep(out);
        return HFPF_OK;
    }
    uint32_t* vshell = parent_s;  // the shells' forest is dead behind its flatten
    hipLaunchKernelGGL(k_top_vlabel, grid_v, dim3(256), 0, h->stream, root_s, base, used, (const uint32_t*)nullptr, m.n_verts, vshell);
    HIPCHK(h, hipGetLastError());
    if ((rc = sort_pairs_u64(h, key_in, key_out, val_in, val_out, n_slots, kTopKeyBits))) return rc;
    if (trace) HIPCHK(h, hipStreamSynchronize(h->stream));
    mark(2);
    const dim3 grid_e(blocks_for(n_he, 256)), grid_e1(blocks_for(n_he + 1, 256));
    hipLaunchKernelGGL(k_top_classify, grid_e1, dim3(256), 0, h->stream, key_out, n_he, use, listed, parent_l, deg_out, deg_in, ctr);
    HIPCHK(h, hipGetLastError());
    uint64_t n_listed = 0, n_loops = 0;
    if ((rc = scan_counts_locked(h, listed, lbase, n_he, &n_listed))) return rc;
    mark(3);
    hipLaunchKernelGGL(k_comp_flatten, grid_v1, dim3(256), 0, h->stream, parent_l, nv, root_l, flag);
    hipLaunchKernelGGL(k_top_mask, grid_v, dim3(256), 0, h->stream, flag, deg_out, deg_in, m.n_verts);
    HIPCHK(h, hipGetLastError());
    if ((rc = scan_counts_locked(h, flag, base, m.n_verts, &n_loops))) return rc;
    mark(4);
    uint32_t* vloop = parent_l;  // as vshell
    hipLaunchKernelGGL(k_top_vlabel, grid_v, dim3(256), 0, h->stream, root_l, base, deg_out, deg_in, m.n_verts, vloop);
    HIPCHK(h, hipGetLastError());
    set.add(n_listed * sizeof(TopEdge), n_listed == 0);
    set.add(n_loops * sizeof(TopLoop), n_loops == 0);
    set.add(n_shells * sizeof(TopShell));
    set.add((size_t)m.n_tris * 4, !want_tri_shell);
    if ((rc = result_alloc(h, set, on_device, "mesh_topology"))) return rc;
    TopEdge* edges = (TopEdge*)set.a[0].dev;
    TopLoop* loops = (TopLoop*)set.a[1].dev;
    TopShell* shells = (TopShell*)set.a[2].dev;
    uint32_t* tri_shell = (uint32_t*)set.a[3].dev;
    if (n_loops) HIPCHK(h, hipMemsetAsync(loops, 0, n_loops * sizeof(TopLoop), h->stream));
    HIPCHK(h, hipMemsetAsync(shells, 0, n_shells * sizeof(TopShell), h->stream));
    hipLaunchKernelGGL(k_top_vertices, grid_v, dim3(256), 0, h->stream, m.n_verts, used, vshell, vloop, root_s, root_l, deg_out, deg_in, shells, (uint32_t)n_shells, loops,
                       (uint32_t)n_loops, ctr);
    hipLaunchKernelGGL(k_top_tris, grid_t, dim3(256), 0, h->stream, p, m.tris, V, vshell, shells, (uint32_t)n_shells, tri_shell);
    hipLaunchKernelGGL(k_top_edges, grid_e, dim3(256), 0, h->stream, key_out, val_out, n_he, use, lbase, vshell, vloop, m.n_verts, shells, (uint32_t)n_shells, edges,
                       (uint32_t)n_listed);
    if (n_listed)
        hipLaunchKernelGGL(k_top_loops, dim3(blocks_for(n_listed, 256)), dim3(256), 0, h->stream, edges, (uint32_t)n_listed, V, m.n_verts, loops, (uint32_t)n_loops);
    hipLaunchKernelGGL(k_top_finish, dim3(blocks_for(std::max(n_loops, n_shells), 256)), dim3(256), 0, h->stream, (uint32_t)n_loops, loops, (uint32_t)n_shells, shells,
                       ctr);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(&hc, ctr, sizeof hc, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    mark(5);
    if (trace)
        fprintf(stderr, "hfpf: topology: %llu triangles: vertices, emit, shells %.3f ms; sort %.3f ms; run walk, listed scan %.3f ms; loops %.3f ms; "
                        "allocation, reductions, finish %.3f ms\n",
                (unsigned long long)m.n_tris, stamp[1] - stamp[0], stamp[2] - stamp[1], stamp[3] - stamp[2], stamp[4] - stamp[3], stamp[5] - stamp[4]);
    if (hc.n_boundary + hc.n_nonmanifold + hc.n_miswound != n_listed || hc.n_interior + n_listed != hc.n_edges)
        return fail(h, HFPF_ERR_STATE, "mesh_topology: the edge classes do not add up to the arrays (internal)");
    S->n_verts_used = hc.n_verts_used, S->n_edges = hc.n_edges, S->n_interior = hc.n_interior, S->n_boundary = hc.n_boundary;
    S->n_nonmanifold = hc.n_nonmanifold, S->n_miswound = hc.n_miswound, S->n_loops = n_loops, S->n_closed_loops = hc.n_closed_loops;
    S->n_shells = n_shells, S->n_watertight = hc.n_watertight;
    nout->n_edges = n_listed, nout->n_loops = n_loops, nout->n_shells = n_shells;
    set.keep(out);
    return HFPF_OK;
}

// The checks of both forms, all of them before anything is read through a mesh pointer.  0 = fine, else the text of the fault.
static const char* topology_args_fault(const hfpf_topology_opts* o, const MeshRef& m, const double* pose, const void* const outs[7], bool on_device)
{
    if (hfpf_check_topology_opts(o) != HFPF_OK) return "invalid hfpf_topology_opts";
    if (const char* f = mesh_args_fault(m, pose)) return f;
    if (const char* f = topology_counts_fault(m.n_verts, m.n_tris)) return f;
    for (int i = 0; i < 7; i++)
        if (!outs[i]) return "NULL output pointer";
    if (on_device && mesh_misaligned(m)) return "device mesh pointers must be 4-byte aligned";
    return nullptr;
}

// A mesh without triangles is answered here, in front of any upload or scratch request: a zeroed summary and NULL arrays.  tri_shell
// may be NULL: the per-triangle words are then not produced.
static int topology_common(hfpf_handle* h, const hfpf_topology_opts* o, const void* verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* tris, uint64_t n_tris,
                           const double* pose, bool on_device, hfpf_topology_edge** edges, uint64_t* n_edges, hfpf_topology_loop** loops, uint64_t* n_loops,
                           hfpf_topology_shell** shells, uint64_t* n_shells, uint32_t** tri_shell, hfpf_topology_summary* summary)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    const MeshRef m{verts, n_verts, vertex_stride, tris, n_tris};
    const void* const outs[7] = {edges, n_edges, loops, n_loops, shells, n_shells, summary};
    if (const char* f = topology_args_fault(o, m, pose, outs, on_device)) return args_fail(h, "mesh_topology", on_device, f);
    MeshRef d;
    ResultSet set;
    TopologyCounts n;
    hfpf_topology_summary s{};
    void* out[kResultArrays];
    int rc;
    if ((rc = local_read_prologue_locked(h, "mesh_topology"))) return rc;
    if (n_tris && (rc = mesh_on_device_locked(h, "mesh_topology", m, on_device, &d))) return rc;
    if (n_tris && (rc = topology_locked(h, d, pose, on_device, tri_shell != nullptr, &set, &n, &s))) return rc;
    if ((rc = result_deliver(h, set, on_device, "mesh_topology", out))) return rc;
    *edges = (hfpf_topology_edge*)out[0], *loops = (hfpf_topology_loop*)out[1], *shells = (hfpf_topology_shell*)out[2];
    if (tri_shell) *tri_shell = (uint32_t*)out[3];
    *n_edges = n.n_edges, *n_loops = n.n_loops, *n_shells = n.n_shells, *summary = s;
    return HFPF_OK;
}

int hfpf_mesh_topology_device(hfpf_handle* h, const hfpf_topology_opts* o, const void* dev_verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* dev_tris,
                              uint64_t n_tris, const double* pose_3x4, hfpf_topology_edge** dev_edges, uint64_t* n_edges, hfpf_topology_loop** dev_loops,
                              uint64_t* n_loops, hfpf_topology_shell** dev_shells, uint64_t* n_shells, uint32_t** dev_tri_shell, hfpf_topology_summary* summary)
{
    return topology_common(h, o, dev_verts, n_verts, vertex_stride, dev_tris, n_tris, pose_3x4, true, dev_edges, n_edges, dev_loops, n_loops, dev_shells, n_shells,
                           dev_tri_shell, summary);
}

int hfpf_mesh_topology(hfpf_handle* h, const hfpf_topology_opts* o, const void* verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* tris, uint64_t n_tris,
                       const double* pose_3x4, hfpf_topology_edge** edges, uint64_t* n_edges, hfpf_topology_loop** loops, uint64_t* n_loops,
                       hfpf_topology_shell** shells, uint64_t* n_shells, uint32_t** tri_shell, hfpf_topology_summary* summary)
{
    return topology_common(h, o, verts, n_verts, vertex_stride, tris, n_tris, pose_3x4, false, edges, n_edges, loops, n_loops, shells, n_shells, tri_shell, summary);
}

void hfpf_free_topology(hfpf_topology_edge* edges, hfpf_topology_loop* loops, hfpf_topology_shell* shells, uint32_t* tri_shell)
{
    free(edges);
    free(loops);
    free(shells);
    free(tri_shell);
}

// ---- view planning (include/hfpf.h) ---------------------------------------------------------------------------------------------
int hfpf_check_plan_opts(const hfpf_plan_opts* o)
{
    if (!o || o->struct_size != sizeof(hfpf_plan_opts) || (o->flags & ~(HFPF_PLAN_TWO_SIDED | HFPF_PLAN_MODEL_OCCLUDES)) || o->reserved0 != 0 || o->reserved != 0)
        return HFPF_ERR_BAD_ARG;
    if (hfpf_check_cover_opts(&o->cover) != HFPF_OK || !view_opts_ok(&o->view)) return HFPF_ERR_BAD_ARG;
    if (!(std::isfinite(o->occluder_near) && o->occluder_near > 0.0 && o->occluder_near <= o->view.z_near)) return HFPF_ERR_BAD_ARG;
    if (!(std::isfinite(o->min_cos) && o->min_cos >= -1.0 && o->min_cos <= 1.0)) return HFPF_ERR_BAD_ARG;
    if (!(std::isfinite(o->tolerance) && o->tolerance > 0.0 && o->tolerance <= 1.0)) return HFPF_ERR_BAD_ARG;
    if (!(std::isfinite(o->slope) && o->slope >= 0.0 && o->slope <= 1.0)) return HFPF_ERR_BAD_ARG;
    return o->max_views >= 1 && o->max_views <= 256 ? HFPF_OK : HFPF_ERR_BAD_ARG;
}

constexpr uint32_t kPlanMaxViews = 4096;
constexpr uint64_t kPlanMaxPairs = 1ull << 35;  // (target, view) pairs: 4 GiB of bitsets

// The views of one depth-buffer chunk: the zbuf rule of a render on 4-byte words, or what HFPF_PLAN_CHUNK=1..64 forces (tests).
static uint32_t plan_chunk_views(uint64_t WH, uint32_t n_views)
{
    uint32_t per = view_chunk(WH, sizeof(uint32_t), n_views);
    if (const char* e = getenv("HFPF_PLAN_CHUNK")) {
        const long v = strtol(e, nullptr, 10);
        if (v >= 1 && v <= 64) per = std::min(per, (uint32_t)v);
    }
    return per;
}

// Validated arguments in, the mesh on the device, n_tris > 0, under the lock.  The cover with the samples marked; the scan of the
// marks (its total, the number of targets, is read back: the capacity check and the size of everything behind it); then, without a
// host wait: compaction, per chunk of views the occluder splats and the visibility words, the greedy
// rounds, the triangle records.  One read-back of the scores and the state words ends the call.  *out: the n_tris records
// (absent without want_plan).  Not timed: hfpf_get_kernel_time has no id for it.
static int plan_locked(hfpf_handle* h, const hfpf_plan_opts* o, const MeshRef& m, const double* pose, const double* poses, uint32_t n_views, bool on_device,
                       bool want_plan, ResultSet* out, hfpf_view_score* scores, hfpf_plan_summary* summary)
{
    int rc;
    const uint64_t n_tris = m.n_tris, NV1 = std::max<uint32_t>(n_views, 1);
    PlanState* st; PlanScore* score; unsigned long long* gain; TriCoverage* cov;
    if ((rc = scratch(h, h->plan_ctr, ScratchLayout().add(&st, 1).add(&score, NV1).add(&gain, 2 * NV1).add(&cov, n_tris)))) return rc;
    ResultSet set;
    set.add((size_t)n_tris * sizeof(TriPlan), !want_plan);
    if ((rc = result_alloc(h, set, on_device, "plan_views"))) return rc;
    TriPlan* plan = (TriPlan*)set.a[0].dev;  // NULL when absent
    hfpf_plan_summary S;
    memset(&S, 0, sizeof S);
    CovSamples cs{};
    if ((rc = cover_run_locked(h, &o->cover, m, pose, cov, &S.coverage, &cs))) return rc;
    // hi * 2^32 + lo >= 2^62 iff hi + (lo >> 32) >= 2^30 (both words are below 2^63)
    if (S.coverage.area_q40_hi + (S.coverage.area_q40_lo >> 32) >= (1ull << 30)) return fail(h, HFPF_ERR_CAPACITY, "plan_views: the mesh's area is 2^22 m^2 or more: the q40 sums would not fit");
    uint64_t n_targets = 0;
    uint32_t* toff = nullptr;
    if (cs.total) {
        if ((rc = scratch_n(h, h->plan_scan, cs.total + 1, &toff)) || (rc = scan_counts_locked(h, cs.target, toff, cs.total, &n_targets))) return rc;
    }
    if (n_targets * n_views > kPlanMaxPairs)  // nothing on the handle was touched: it stays usable
        return fail(h, HFPF_ERR_CAPACITY, "plan_views: %llu targets x %u views exceed the 2^35 pairs a call takes (fewer views, or a larger spacing)",
                    (unsigned long long)n_targets, n_views);
    const uint64_t n_words = (n_targets + 63) / 64, W1 = std::max<uint64_t>(n_words, 1), WH = (uint64_t)o->view.width * o->view.height;
    float4* tp; unsigned long long *tw, *remaining, *bits;
    if ((rc = scratch(h, h->plan_targets, ScratchLayout().add(&tp, std::max<uint64_t>(n_targets, 1)).add(&tw, std::max<uint64_t>(n_targets, 1))))) return rc;
    if ((rc = scratch(h, h->plan_bits, ScratchLayout().add(&remaining, W1).add(&bits, std::max<uint64_t>(n_views * n_words, 1))))) return rc;
    const bool look = n_targets && n_views;
    RowSet rows{};
    uint32_t* zbuf = nullptr;
    double* pose_d = nullptr;
    const uint32_t per_chunk = plan_chunk_views(WH, n_views);
    PlanParams p{};
    if (look) {
        if (o->flags & HFPF_PLAN_MODEL_OCCLUDES) {
            const ExtractOpts opt{std::max(1.0, o->view.min_count), -1, 0};  // the rows of a render
            if ((rc = build_rows_locked(h, h->t.stats, opt, &rows))) return rc;
            if (rows.n > 0xFFFFFFFFull) return fail(h, HFPF_ERR_CAPACITY, "plan_views: %llu rows exceed the 2^32 - 1 a splat launch takes", (unsigned long long)rows.n);
        }
        if ((rc = scratch_n(h, h->zbuf, per_chunk * WH, &zbuf)) || (rc = upload_poses(h, h->render_pose, poses, n_views, &pose_d))) return rc;
        p.cam = pinhole_of(o->view);
        p.cull = (o->view.flags & HFPF_RENDER_CULL_BACKFACES) ? 1u : 0u, p.two_sided = (o->flags & HFPF_PLAN_TWO_SIDED) ? 1u : 0u;
        p.radius = o->view.splat_radius, p.max_radius = o->view.max_splat_radius;
        p.occ_near = o->occluder_near;
        p.r_num_samples = (0.5 * o->cover.spacing) * std::max(o->view.fx, o->view.fy);
        p.r_num_rows = (0.5 * h->g.res) * std::max(o->view.fx, o->view.fy);
        p.min_cos = o->min_cos, p.tolerance = o->tolerance, p.slope = o->slope;
    }

    HIPCHK(h, hipMemsetAsync(st, 0, sizeof(PlanState) + NV1 * (sizeof(PlanScore) + 16), h->stream));  // the state, the scores and the gains are adjacent
    hipLaunchKernelGGL(k_plan_begin, dim3(blocks_for(std::max<uint64_t>(W1, n_views), 256)), dim3(256), 0, h->stream, (uint32_t)n_targets, n_words, remaining, n_views,
                       score);
    if (plan) hipLaunchKernelGGL(k_plan_tri_begin, dim3(blocks_for(n_tris, 256)), dim3(256), 0, h->stream, (uint32_t)n_tris, cov, plan);
    if (n_targets) {
        hipLaunchKernelGGL(k_plan_compact, dim3(blocks_for(cs.total, 256)), dim3(256), 0, h->stream, cs.offset, cs.geo, (uint32_t)n_tris, (uint32_t)cs.total,
                           cs.target, toff, tp, tw);
    }
    HIPCHK(h, hipGetLastError());
    const unsigned t_blocks = blocks_for(n_targets, 256);
    for (uint32_t v0 = 0; look && v0 < n_views; v0 += per_chunk) {
        p.n_views = std::min(per_chunk, n_views - v0);
        HIPCHK(h, hipMemsetAsync(zbuf, 0xFF, p.n_views * WH * 4, h->stream));
        hipLaunchKernelGGL(k_plan_splat_samples, dim3(blocks_for(cs.total, 256)), dim3(256), 0, h->stream, cs.offset, cs.geo, (uint32_t)n_tris, (uint32_t)cs.total,
                           pose_d + 12ull * v0, p, zbuf);
        if (rows.n)
            hipLaunchKernelGGL(k_plan_splat_rows, dim3(blocks_for(rows.n, 256)), dim3(256), 0, h->stream, rows.rows, (uint32_t)rows.n, pose_d + 12ull * v0, p, zbuf);
        hipLaunchKernelGGL(k_plan_visible, dim3(t_blocks, p.n_views), dim3(256), 0, h->stream, tp, tw, (uint32_t)n_targets, cs.geo, pose_d + 12ull * v0, p, zbuf, v0,
                           n_words, bits, score);
        HIPCHK(h, hipGetLastError());
    }
    const uint32_t rounds = look ? std::min(o->max_views, n_views) : 0u;  // every round takes a view or ends the selection
    for (uint32_t k = 0; k < rounds; k++) {
        hipLaunchKernelGGL(k_plan_gain, dim3(t_blocks, n_views), dim3(256), 0, h->stream, tw, (uint32_t)n_targets, n_words, bits, remaining, score, st, gain);
        hipLaunchKernelGGL(k_plan_argmax, dim3(1), dim3(256), 0, h->stream, k, n_views, (unsigned long long)o->min_gain_q40, score, gain, st);
        hipLaunchKernelGGL(k_plan_take, dim3(blocks_for(n_words, 256)), dim3(256), 0, h->stream, n_words, bits, remaining, st);
    }
    if (n_targets)
        hipLaunchKernelGGL(k_plan_finish, dim3(t_blocks), dim3(256), 0, h->stream, tp, tw, (uint32_t)n_targets, n_words, look ? n_views : 0u, bits, remaining, plan, st);
    HIPCHK(h, hipGetLastError());
    PlanState hs;
    std::vector<PlanScore> hsc(NV1);
    HIPCHK(h, hipMemcpyAsync(&hs, st, sizeof hs, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(hsc.data(), score, NV1 * sizeof(PlanScore), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    S.n_views = n_views, S.n_selected = hs.n_selected;
    S.n_targets = n_targets, S.n_reachable = hs.n_reachable, S.n_planned = hs.n_planned;
    S.target_q40 = hs.target_q40, S.reachable_q40 = hs.reachable_q40, S.planned_q40 = hs.planned_q40;
    static_assert(sizeof(PlanScore) == sizeof(hfpf_view_score) && sizeof(TriPlan) == sizeof(hfpf_tri_plan), "the device records are the public ones");
    if (n_views) memcpy(scores, hsc.data(), (size_t)n_views * sizeof(PlanScore));
    *summary = S;
    set.keep(out);
    return HFPF_OK;
}

// The checks of both forms.  0 = fine, else the text of the fault.
static const char* plan_args_fault(const hfpf_plan_opts* o, const MeshRef& m, const double* pose, const double* poses, uint32_t n_views, const void* scores,
                                   const void* summary, bool on_device)
{
    if (hfpf_check_plan_opts(o) != HFPF_OK) return "invalid hfpf_plan_opts";
    if (const char* f = mesh_args_fault(m, pose)) return f;
    if (!scores || !summary) return "NULL scores or summary";
    if (n_views > kPlanMaxViews) return "more than 4096 views";
    if (n_views && !poses) return "NULL poses";
    for (uint64_t i = 0; i < 12ull * n_views; i++)
        if (!std::isfinite(poses[i])) return "a view's pose is not finite";
    if (on_device && mesh_misaligned(m)) return "device mesh pointers must be 4-byte aligned";
    return nullptr;
}

// n_tris = 0: nothing to plan.
static void plan_empty(uint32_t n_views, hfpf_view_score* scores, hfpf_plan_summary* summary)
{
    memset(summary, 0, sizeof *summary);
    summary->n_views = n_views;
    for (uint32_t v = 0; v < n_views; v++) {
        memset(&scores[v], 0, sizeof scores[v]);
        scores[v].rank = -1;
    }
}

// A mesh without triangles is answered here, in front of any upload or scratch request: plan_empty and a NULL plan.  The scores and
// the summary are computed into locals in both forms, so they reach the caller only when the records have too.
static int plan_common(hfpf_handle* h, const hfpf_plan_opts* o, const void* verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* tris, uint64_t n_tris,
                       const double* pose, const double* poses, uint32_t n_views, bool on_device, hfpf_view_score* scores, hfpf_tri_plan** plan,
                       hfpf_plan_summary* summary)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    const MeshRef m{verts, n_verts, vertex_stride, tris, n_tris};
    if (const char* f = plan_args_fault(o, m, pose, poses, n_views, scores, summary, on_device)) return args_fail(h, "plan_views", on_device, f);
    MeshRef d;
    ResultSet set;
    std::vector<hfpf_view_score> sc(std::max<uint32_t>(n_views, 1));
    hfpf_plan_summary s;
    void* out[kResultArrays];
    int rc;
    if ((rc = local_read_prologue_locked(h, "plan_views"))) return rc;
    if (n_tris == 0) plan_empty(n_views, sc.data(), &s);
    if (n_tris && (rc = mesh_on_device_locked(h, "plan_views", m, on_device, &d))) return rc;
    if (n_tris && (rc = plan_locked(h, o, d, pose, poses, n_views, on_device, plan != nullptr, &set, sc.data(), &s))) return rc;
    if ((rc = result_deliver(h, set, on_device, "plan_views", out))) return rc;
    if (n_views) memcpy(scores, sc.data(), (size_t)n_views * sizeof(hfpf_view_score));
    *summary = s;
    if (plan) *plan = (hfpf_tri_plan*)out[0];
    return HFPF_OK;
}

int hfpf_plan_views_device(hfpf_handle* h, const hfpf_plan_opts* o, const void* dev_verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* dev_tris,
                           uint64_t n_tris, const double* pose_3x4, const double* poses, uint32_t n_views, hfpf_view_score* scores, hfpf_tri_plan** dev_plan,
                           hfpf_plan_summary* summary)
{
    return plan_common(h, o, dev_verts, n_verts, vertex_stride, dev_tris, n_tris, pose_3x4, poses, n_views, true, scores, dev_plan, summary);
}

int hfpf_plan_views(hfpf_handle* h, const hfpf_plan_opts* o, const void* verts, uint64_t n_verts, uint32_t vertex_stride, const uint32_t* tris, uint64_t n_tris,
                    const double* pose_3x4, const double* poses, uint32_t n_views, hfpf_view_score* scores, hfpf_tri_plan** plan, hfpf_plan_summary* summary)
{
    return plan_common(h, o, verts, n_verts, vertex_stride, tris, n_tris, pose_3x4, poses, n_views, false, scores, plan, summary);
}

void hfpf_free_plan(hfpf_tri_plan* plan) { free(plan); }

// ---- rows that depth frames see through (include/hfpf.h) -------------------------------------------------------------------
int hfpf_check_consistency_opts(const hfpf_consistency_opts* o)
{
    if (!o || o->struct_size != sizeof(hfpf_consistency_opts) || (o->flags & ~HFPF_CONSISTENCY_DROP) || o->reserved != 0) return HFPF_ERR_BAD_ARG;
    if (o->window < 0 || o->window > 2 || std::isnan(o->min_count)) return HFPF_ERR_BAD_ARG;
    if (!(std::isfinite(o->z_near) && std::isfinite(o->z_far) && 0.0 < o->z_near && o->z_near < o->z_far)) return HFPF_ERR_BAD_ARG;
    if (!(std::isfinite(o->tolerance) && o->tolerance > 0.0 && o->tolerance <= 1.0)) return HFPF_ERR_BAD_ARG;
    if (!(std::isfinite(o->slope) && o->slope >= 0.0 && o->slope <= 1.0)) return HFPF_ERR_BAD_ARG;
    if (!(std::isfinite(o->min_cos) && o->min_cos >= -1.0 && o->min_cos <= 1.0)) return HFPF_ERR_BAD_ARG;
    return std::isfinite(o->through_ratio) && o->through_ratio >= 0.0 ? HFPF_OK : HFPF_ERR_BAD_ARG;
}

constexpr uint32_t kConsMaxFrames = 1u << 20;

// The frames of a call, host or device.
struct ConsFrames {
    const void* depth;
    uint64_t stride;
    uint32_t n;
    const double* poses;
};

// The checks of both forms (HFPF_ERR_BAD_ARG; nothing on the handle changes) and the descriptor as the kernels take it.
static int consistency_args_locked(hfpf_handle* h, const hfpf_consistency_opts* o, const hfpf_depth_image* desc, const ConsFrames& f, const void* cons,
                                   const void* n_rows, const void* summary, bool on_device, DepthSpec* ds)
{
    if (hfpf_check_consistency_opts(o) != HFPF_OK) return fail(h, HFPF_ERR_BAD_ARG, "depth_consistency: invalid hfpf_consistency_opts");
    if (!cons || !n_rows || !summary) return fail(h, HFPF_ERR_BAD_ARG, "depth_consistency: NULL cons, n_rows or summary");
    if (f.n > kConsMaxFrames) return fail(h, HFPF_ERR_BAD_ARG, "depth_consistency: %u frames exceed 2^20", f.n);
    // the descriptor as hfpf_query_depth checks it; without frames there is no image to be NULL
    PointSource src{};
    if (int rc = colorless_depth_source(h, desc, f.n ? f.depth : (const void*)desc, &src)) return rc;
    *ds = src.ds;
    if (f.n == 0) return HFPF_OK;
    if (!f.poses) return fail(h, HFPF_ERR_BAD_ARG, "depth_consistency: NULL poses");
    for (uint64_t i = 0; i < 12ull * f.n; i++)
        if (!std::isfinite(f.poses[i])) return fail(h, HFPF_ERR_BAD_ARG, "depth_consistency: pose %llu is not finite", (unsigned long long)(i / 12));
    const uint32_t dbpp = ds->depth_f32 ? 4u : 2u;
    if (f.stride < ds->depth_bytes() || f.stride % dbpp)
        return fail(h, HFPF_ERR_BAD_ARG, "depth_consistency: depth_frame_stride %llu (an image takes %zu bytes, samples %u)", (unsigned long long)f.stride,
                    ds->depth_bytes(), dbpp);
    if (on_device && (uintptr_t)f.depth % dbpp) return fail(h, HFPF_ERR_BAD_ARG, "depth_consistency_device: the images must be aligned to the sample size");
    return HFPF_OK;
}

// k_consistency over the n frames at `dev` (frame_base = the index of the first in the call; d_pose = its pose), in the launches
// plan_consistency cuts them into.  plain: this span is the whole call and one chunk covers it.
static int consistency_span_locked(hfpf_handle* h, const RowSet& rs, ConsParams p, const void* dev, uint32_t n, uint32_t frame_base, const double* d_pose,
                                   const ConsPlan& plan, bool plain, ConsRec* recs)
{
    p.depth = (const uint8_t*)dev;
    p.n_frames = n;
    p.per_chunk = plan.frames_per_chunk;
    p.frame_base = frame_base;
    p.plain = plain ? 1u : 0u;
    for (uint32_t c0 = 0; c0 < plan.n_chunks; c0 += plan.chunks_per_launch) {
        p.chunk0 = c0;
        const uint32_t nc = std::min(plan.chunks_per_launch, plan.n_chunks - c0);
        hipLaunchKernelGGL(k_consistency, dim3(blocks_for(rs.n, kConsRowTile), nc), dim3(kConsRowTile), 0, h->stream, rs.rows, (uint32_t)rs.n, d_pose, p, recs);
        HIPCHK(h, hipGetLastError());
    }
    return HFPF_OK;
}

// Validated arguments in, under the lock, behind the read prologue.  The row set; the records (k_cons_init unless one plain launch
// writes them whole, k_consistency per span of frames: the device form has one span, the host form one per upload of at most
// kXferChunk bytes); flags, keep marks and summary (k_cons_finish); with HFPF_CONSISTENCY_DROP the scan of the marks and the
// compaction.  *out: rows (absent without want_rows) and records.  Not timed: hfpf_get_kernel_time has no id for it.
static int consistency_locked(hfpf_handle* h, const hfpf_consistency_opts* o, const hfpf_depth_image* desc, const DepthSpec& ds, const ConsFrames& f,
                              bool on_device, bool want_rows, ResultSet* out, uint64_t* n_out, hfpf_consistency_summary* summary)
{
    int rc;
    *n_out = 0;
    memset(summary, 0, sizeof *summary);
    RowSet rs;
    const ExtractOpts opt{o->min_count, -1, 0};  // the compare of hfpf_extract_filtered, 0 keeps all
    if ((rc = build_rows_locked(h, h->t.stats, opt, &rs))) return rc;
    const uint64_t nr = rs.n;
    if (nr == 0) return HFPF_OK;
    if (nr >= 0xFFFFFFFFull) return fail(h, HFPF_ERR_CAPACITY, "depth_consistency: %llu rows exceed the 32-bit row index", (unsigned long long)nr);
    const uint32_t n = (uint32_t)nr;
    const uint64_t R1 = nr + 1;
    ConsRec* recs; ConsSummary* d_sum; uint32_t *keep, *base;
    if ((rc = scratch(h, h->cons_recs, ScratchLayout().add(&recs, nr).add(&d_sum, 1).add(&keep, R1).add(&base, R1)))) return rc;
    double* d_pose = nullptr;
    if (f.n && (rc = upload_poses(h, h->cons_pose, f.poses, f.n, &d_pose))) return rc;
    ConsParams p{};
    p.frame_stride = f.stride;
    p.depth_step = ds.depth_step, p.depth_f32 = ds.depth_f32;
    p.gate = o->min_cos >= 0.0 ? 1u : 0u;
    p.window = o->window;
    p.unit = ds.unit;
    p.cam = pinhole_of(*desc, o->z_near, o->z_far);
    p.tolerance = o->tolerance, p.slope = o->slope, p.min_cos2 = o->min_cos * o->min_cos;
    p.through_ratio = o->through_ratio;
    p.min_through = std::max(1u, o->min_through);
    p.drop = (o->flags & HFPF_CONSISTENCY_DROP) ? 1u : 0u;
    // frames per upload of the host form: whole frames, padding between them included, in at most kXferChunk bytes (one at least)
    const size_t img = ds.depth_bytes();
    uint32_t per_upload = f.n;
    if (!on_device && f.n) per_upload = (uint32_t)std::min<uint64_t>(f.n, img <= kXferChunk ? 1 + (kXferChunk - img) / f.stride : 1);
    const uint32_t forced = (uint32_t)h->knobs.cons_chunk;
    const bool one_span = per_upload == f.n;
    const bool plain = f.n && one_span && plan_consistency(nr, f.n, (uint32_t)h->compute_units, forced).single;
    HIPCHK(h, hipMemsetAsync(d_sum, 0, sizeof(ConsSummary), h->stream));
    if (!plain) {
        hipLaunchKernelGGL(k_cons_init, dim3(blocks_for(nr, 256)), dim3(256), 0, h->stream, n, recs);
        HIPCHK(h, hipGetLastError());
    }
    for (uint32_t f0 = 0; f0 < f.n; f0 += per_upload) {
        const uint32_t nf = std::min(per_upload, f.n - f0);
        const void* dev = (const uint8_t*)f.depth + (uint64_t)f0 * f.stride;
        if (!on_device) {
            const size_t bytes = (size_t)(nf - 1) * f.stride + img;
            uint8_t* d_in;
            if ((rc = scratch_n(h, h->cons_in, bytes, &d_in))) return rc;
            const hipError_t e = upload_pageable(h, d_in, dev, bytes);  // complete on return: the next upload may overwrite it
            if (e != hipSuccess) return fail(h, HFPF_ERR_HIP, "depth_consistency upload: %s", hipGetErrorString(e));
            dev = d_in;
        }
        const ConsPlan plan = plan_consistency(nr, nf, (uint32_t)h->compute_units, forced);
        if ((rc = consistency_span_locked(h, rs, p, dev, nf, f0, d_pose + 12ull * f0, plan, plain, recs))) return rc;
        if (!on_device) HIPCHK(h, hipStreamSynchronize(h->stream));  // ... and this span's kernels have read it
    }
    hipLaunchKernelGGL(k_cons_finish, dim3(blocks_for(R1, 256)), dim3(256), 0, h->stream, n, p, recs, keep, d_sum);
    HIPCHK(h, hipGetLastError());
    uint64_t nk = nr;
    if (p.drop)
        if ((rc = scan_counts_locked(h, keep, base, nr, &nk))) return rc;
    ConsSummary hs;
    HIPCHK(h, hipMemcpyAsync(&hs, d_sum, sizeof hs, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    static_assert(sizeof(ConsSummary) == sizeof(hfpf_consistency_summary), "the device summary is the public one");
    memcpy(summary, &hs, sizeof hs);
    if (nk == 0) return HFPF_OK;
    ResultSet set;
    set.add((size_t)nk * sizeof(Row), !want_rows, p.drop ? nullptr : rs.rows);
    set.add((size_t)nk * sizeof(ConsRec), false, p.drop ? nullptr : recs);
    if ((rc = result_alloc(h, set, on_device, "depth_consistency"))) return rc;
    hipError_t e = hipSuccess;
    if (p.drop) {
        hipLaunchKernelGGL(k_cons_compact, dim3(blocks_for(nr, 256)), dim3(256), 0, h->stream, rs.rows, n, recs, keep, base, (Row*)set.a[0].dev, (ConsRec*)set.a[1].dev);
        e = hipGetLastError();
    } else if (on_device) {  // the borrowed arrays into the caller's
        if (want_rows) e = hipMemcpyAsync(set.a[0].dev, rs.rows, set.a[0].bytes, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(set.a[1].dev, recs, set.a[1].bytes, hipMemcpyDeviceToDevice, h->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, HFPF_ERR_HIP, "depth_consistency: %s", hipGetErrorString(e));
    set.keep(out), *n_out = nk;
    return HFPF_OK;
}

static int consistency_common(hfpf_handle* h, const hfpf_consistency_opts* o, const hfpf_depth_image* desc, const void* depth, uint64_t depth_frame_stride,
                              uint32_t n_frames, const double* poses, bool on_device, hfpf_row** rows, hfpf_row_consistency** cons, uint64_t* n_rows,
                              hfpf_consistency_summary* summary)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    const ConsFrames f{depth, depth_frame_stride, n_frames, poses};
    DepthSpec ds;
    if (int rc = consistency_args_locked(h, o, desc, f, cons, n_rows, summary, on_device, &ds)) return rc;
    ResultSet set;  // empty (nk = 0) without a row, or with none kept: NULL arrays beside the summary, no download
    uint64_t nk = 0;
    hfpf_consistency_summary s;
    void* out[kResultArrays];
    int rc;
    if ((rc = local_read_prologue_locked(h, "depth_consistency")) || (rc = consistency_locked(h, o, desc, ds, f, on_device, rows != nullptr, &set, &nk, &s))) return rc;
    if ((rc = result_deliver(h, set, on_device, "depth_consistency", out))) return rc;
    if (rows) *rows = (hfpf_row*)out[0];
    *cons = (hfpf_row_consistency*)out[1], *n_rows = nk, *summary = s;
    return HFPF_OK;
}

int hfpf_depth_consistency_device(hfpf_handle* h, const hfpf_consistency_opts* o, const hfpf_depth_image* desc, const void* dev_depth,
                                  uint64_t depth_frame_stride, uint32_t n_frames, const double* poses, hfpf_row** dev_rows,
                                  hfpf_row_consistency** dev_cons, uint64_t* n_rows, hfpf_consistency_summary* summary)
{
    return consistency_common(h, o, desc, dev_depth, depth_frame_stride, n_frames, poses, true, dev_rows, dev_cons, n_rows, summary);
}

int hfpf_depth_consistency(hfpf_handle* h, const hfpf_consistency_opts* o, const hfpf_depth_image* desc, const void* depth, uint64_t depth_frame_stride,
                           uint32_t n_frames, const double* poses, hfpf_row** rows, hfpf_row_consistency** cons, uint64_t* n_rows,
                           hfpf_consistency_summary* summary)
{
    return consistency_common(h, o, desc, depth, depth_frame_stride, n_frames, poses, false, rows, cons, n_rows, summary);
}

void hfpf_free_consistency(hfpf_row* rows, hfpf_row_consistency* cons)
{
    free(rows);
    free(cons);
}

// ---- hidden rows (include/hfpf.h) ------------------------------------------------------------------------------------------
static_assert(kHideOpHide == HFPF_HIDE && kHideOpShow == HFPF_SHOW && kHideOpOthers == HFPF_HIDE_OTHERS, "host_plan.hpp mirrors the ops of include/hfpf.h");

int hfpf_check_hide_opts(const hfpf_hide_opts* o)
{
    return o && hide_opts_ok(o->struct_size, (uint32_t)sizeof(hfpf_hide_opts), o->op, o->flags, o->reserved) ? HFPF_OK : HFPF_ERR_BAD_ARG;
}

// The prologue of the calls that change or list H: the refusals of hfpf_snapshot (H travels in a snapshot), then the read prologue.
static int hide_prologue_locked(hfpf_handle* h, const char* what)
{
    if (h->dist_on) return fail(h, HFPF_ERR_STATE, "%s: not available on a handle with an RCCL communicator", what);
    if (h->epoch_used) return fail(h, HFPF_ERR_STATE, "%s: this handle has exchanged epoch records or statistic words; a distributed form is not provided", what);
    return read_prologue_locked(h);
}

// The HIDDEN bits: allocated, all zero, by the first call that needs to write them.
static int hide_words_locked(hfpf_handle* h)
{
    if (h->hidden_words) return HFPF_OK;
    return dev_alloc(h, &h->hidden_words, (h->t.max_bricks + 1) * 8);
}

// The scratch of one call: the mark words of the used bricks and the counters, zeroed.
struct HideCall {
    unsigned long long* mark;
    HideCounts* cnt;
    uint32_t nb;  // bricks in use (ids 1..nb)
};
static int hide_begin_locked(hfpf_handle* h, HideCall* c)
{
    c->nb = (uint32_t)std::min<uint64_t>(h->h_ctr[C_BRICKS], h->t.max_bricks);
    const ScratchLayout lay = ScratchLayout().add(&c->mark, ((uint64_t)c->nb + 1) * 8).add(&c->cnt, 1);
    if (int rc = scratch(h, h->hide_mark, lay)) return rc;
    HIPCHK(h, hipMemsetAsync(h->hide_mark.p, 0, (size_t)lay.bytes(), h->stream));
    return HFPF_OK;
}

// k_hide_mark over n entries on the device, kHideLaunchEntries a launch.
static int hide_mark_locked(hfpf_handle* h, const HideCall& c, const hfpf_hide_opts* o, const void* dev_voxels, uint64_t n, uint32_t voxel_stride, const void* dev_select,
                            uint32_t select_stride)
{
    for (uint64_t i0 = 0; i0 < n; i0 += kHideLaunchEntries) {
        HideList L{};
        L.voxels = (const uint8_t*)dev_voxels + i0 * voxel_stride;
        L.select = dev_select ? (const uint8_t*)dev_select + i0 * select_stride : nullptr;
        L.n = std::min(kHideLaunchEntries, n - i0);
        L.voxel_stride = voxel_stride, L.select_stride = select_stride, L.select_mask = o->select_mask, L.select_value = o->select_value;
        L.n_bricks = c.nb;
        hipLaunchKernelGGL(k_hide_mark, dim3(blocks_for(L.n, 256)), dim3(256), 0, h->stream, h->g, h->t, L, c.mark, c.cnt);
        HIPCHK(h, hipGetLastError());
    }
    return HFPF_OK;
}

// Second half of every form: H' = op(H, mark) over the words of the used bricks, the counts, Tables::hidden.  mark == NULL: nothing
// is marked (the count of a restored H).  Without the HIDDEN bits the op is counted first and they are allocated only when H' is not
// empty.  Complete on return.
static int hide_apply_locked(hfpf_handle* h, const HideCall& c, uint32_t op, const unsigned long long* mark, HideCounts* out)
{
    const unsigned blocks = blocks_for((uint64_t)c.nb * 8, 256);
    auto run = [&](uint64_t* words, bool write) -> int {
        HIPCHK(h, hipMemsetAsync(&c.cnt->n_changed, 0, 4 * sizeof(unsigned long long), h->stream));
        hipLaunchKernelGGL(k_hide_apply, dim3(blocks), dim3(256), 0, h->stream, h->g, h->t, op, c.nb, mark, (const uint64_t*)words, write ? words : (uint64_t*)nullptr, c.cnt);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(out, c.cnt, sizeof *out, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return HFPF_OK;
    };
    int rc;
    if (!h->hidden_words) {
        if ((rc = run(nullptr, false))) return rc;
        if (out->n_hidden == 0) return HFPF_OK;  // H stays empty: nothing to allocate
        if ((rc = hide_words_locked(h))) return rc;
    }
    if ((rc = run(h->hidden_words, true))) return rc;
    h->ss.n_hidden = out->n_hidden;
    h->t.hidden = out->n_hidden ? h->hidden_words : nullptr;
    return HFPF_OK;
}

static void hide_result(hfpf_hide_result* res, const HideCounts& k)
{
    if (!res) return;
    res->reserved = 0;
    res->n_selected = k.n_selected, res->n_matched = k.n_matched, res->n_changed = k.n_changed, res->n_hidden = k.n_hidden, res->n_full = k.n_full;
}

// Both list forms: validated here (HFPF_ERR_BAD_ARG: nothing on the handle changes), then mark and apply.  The host form uploads
// hide_entries_per_upload entries at a time (voxels, then selector words) and marks them; the device form marks in place.
static int hide_voxels_common(hfpf_handle* h, const hfpf_hide_opts* o, const void* voxels, uint64_t n, uint32_t voxel_stride, const void* select, uint32_t select_stride,
                              hfpf_hide_result* res, bool on_device)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    const char* what = on_device ? "hide_voxels_device" : "hide_voxels";
    if (hfpf_check_hide_opts(o) != HFPF_OK) return fail(h, HFPF_ERR_BAD_ARG, "%s: invalid hfpf_hide_opts", what);
    if (res && res->struct_size != sizeof(hfpf_hide_result)) return fail(h, HFPF_ERR_BAD_ARG, "%s: hfpf_hide_result.struct_size", what);
    if (!hide_list_ok(voxels != nullptr, n, voxel_stride, select != nullptr, select_stride))
        return fail(h, HFPF_ERR_BAD_ARG, "%s: voxel_stride %u / select_stride %u (at least 12 / 4, multiples of 4), or NULL voxels with n > 0", what, voxel_stride, select_stride);
    if (on_device && !hide_device_aligned((uint64_t)(uintptr_t)voxels, (uint64_t)(uintptr_t)select)) return fail(h, HFPF_ERR_BAD_ARG, "%s: device pointers must be 4-byte aligned", what);
    int rc;
    if ((rc = hide_prologue_locked(h, what))) return rc;
    HideCounts k{};
    hide_result(res, k);
    if (h->h_ctr[C_NORMALS] == 0) return HFPF_OK;  // no rows yet: F, M and H are empty
    HideCall c;
    if ((rc = hide_begin_locked(h, &c))) return rc;
    if (on_device) {
        if ((rc = hide_mark_locked(h, c, o, voxels, n, voxel_stride, select, select_stride))) return rc;
    } else {
        const uint64_t per = hide_entries_per_upload(voxel_stride, select != nullptr, select_stride, kXferChunk);
        for (uint64_t i0 = 0; i0 < n; i0 += per) {
            const uint64_t ne = std::min(per, n - i0);
            const uint64_t vb = hide_span_bytes(ne, voxel_stride, kHideVoxelBytes), sb = select ? hide_span_bytes(ne, select_stride, kHideSelectBytes) : 0;
            uint8_t *d_vox, *d_sel;
            if ((rc = scratch(h, h->hide_in, ScratchLayout().add(&d_vox, vb, 16).add(&d_sel, sb, 16)))) return rc;
            hipError_t e = upload_pageable(h, d_vox, (const uint8_t*)voxels + i0 * voxel_stride, vb);  // complete on return
            if (e == hipSuccess && select) e = upload_pageable(h, d_sel, (const uint8_t*)select + i0 * select_stride, sb);
            if (e != hipSuccess) return fail(h, HFPF_ERR_HIP, "%s upload: %s", what, hipGetErrorString(e));
            if ((rc = hide_mark_locked(h, c, o, d_vox, ne, voxel_stride, select ? d_sel : nullptr, select_stride))) return rc;
            if (i0 + per < n) HIPCHK(h, hipStreamSynchronize(h->stream));  // the next upload overwrites what this launch reads
        }
    }
    if ((rc = hide_apply_locked(h, c, o->op, c.mark, &k))) return rc;
    hide_result(res, k);
    return HFPF_OK;
}

int hfpf_hide_voxels(hfpf_handle* h, const hfpf_hide_opts* o, const void* voxels, uint64_t n, uint32_t voxel_stride, const void* select, uint32_t select_stride,
                     hfpf_hide_result* res)
{
    return hide_voxels_common(h, o, voxels, n, voxel_stride, select, select_stride, res, false);
}

int hfpf_hide_voxels_device(hfpf_handle* h, const hfpf_hide_opts* o, const void* dev_voxels, uint64_t n, uint32_t voxel_stride, const void* dev_select,
                            uint32_t select_stride, hfpf_hide_result* res)
{
    return hide_voxels_common(h, o, dev_voxels, n, voxel_stride, dev_select, select_stride, res, true);
}

int hfpf_hide_box(hfpf_handle* h, uint32_t op, const int32_t lo[3], const int32_t hi[3], hfpf_hide_result* res)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    if (!hide_op_ok(op) || !lo || !hi) return fail(h, HFPF_ERR_BAD_ARG, "hide_box: unknown op %u, or NULL lo / hi", op);
    if (res && res->struct_size != sizeof(hfpf_hide_result)) return fail(h, HFPF_ERR_BAD_ARG, "hide_box: hfpf_hide_result.struct_size");
    int rc;
    if ((rc = hide_prologue_locked(h, "hide_box"))) return rc;
    HideCounts k{};
    hide_result(res, k);
    if (h->h_ctr[C_NORMALS] == 0) return HFPF_OK;
    HideCall c;
    if ((rc = hide_begin_locked(h, &c))) return rc;
    const HideBox box = clip_hide_box(lo, hi, h->g.dim);
    if (!box.empty) {
        HideBoxArgs B;
        for (int a = 0; a < 3; a++) B.lo[a] = box.lo[a], B.hi[a] = box.hi[a];
        hipLaunchKernelGGL(k_hide_box, dim3(blocks_for((uint64_t)c.nb * 8, 256)), dim3(256), 0, h->stream, h->g, h->t, B, c.nb, c.mark, c.cnt);
        HIPCHK(h, hipGetLastError());
    }
    if ((rc = hide_apply_locked(h, c, op, c.mark, &k))) return rc;
    k.n_selected = k.n_matched;  // the box form has no entries: both are |M|
    hide_result(res, k);
    return HFPF_OK;
}

int hfpf_show_all(hfpf_handle* h)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    if (int rc = hide_prologue_locked(h, "show_all")) return rc;
    if (h->ss.n_hidden == 0) return HFPF_OK;
    const uint64_t nb = std::min<uint64_t>(h->h_ctr[C_BRICKS], h->t.max_bricks);
    HIPCHK(h, hipMemsetAsync(h->hidden_words, 0, (nb + 1) * 8 * 8, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->ss.n_hidden = 0;
    h->t.hidden = nullptr;
    return HFPF_OK;
}

int hfpf_get_hidden(hfpf_handle* h, int32_t* xyz, uint64_t cap, uint64_t* n_out)
{
    if (!h || !n_out) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    int rc;
    if ((rc = hide_prologue_locked(h, "get_hidden"))) return rc;
    const uint64_t nh = h->ss.n_hidden, n = h->h_ctr[C_NORMALS];
    *n_out = nh;
    if (!xyz || nh == 0 || n == 0) return HFPF_OK;
    uint64_t *unsorted, *sorted; if ((rc = scratch_n(h, h->keys_a, n, &unsorted)) || (rc = scratch_n(h, h->keys_b, n, &sorted))) return rc;
    hipLaunchKernelGGL(k_hidden_keys, dim3(blocks_for(n, 256)), dim3(256), 0, h->stream, h->t, n, unsorted);
    HIPCHK(h, hipGetLastError());
    if ((rc = sort_keys_u64(h, unsorted, sorted, n))) return rc;  // the keys of the records that are not hidden are all ones: behind
    const uint64_t take = std::min(nh, cap);
    std::vector<uint64_t> keys(take);
    if (take) HIPCHK(h, hipMemcpyAsync(keys.data(), sorted, take * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (uint64_t i = 0; i < take; i++) key_coords(h->g, keys[i], xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    return HFPF_OK;
}

int hfpf_stats_export(hfpf_handle* h, const void** dev_words, uint64_t* n_words, const void** dev_cwords, uint64_t* n_cwords)
{
    if (!h || !dev_words || !n_words) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rcf = flush_pending_locked(h)) return rcf;  // host frames still waiting for their launch
    int rc = check_usable(h);
    if (!rc) rc = read_counters(h);
    if (!rc) rc = poison_on_error(h, check_device_errors(h));
    if (rc) return rc;
    h->epoch_used = true;
    *dev_words = h->t.stats;
    *n_words = (h->h_ctr[C_NORMALS] + 1) * kStatWords;
    if (dev_cwords) *dev_cwords = nullptr;  // colour sums are words 5-7 of the same records
    if (n_cwords) *n_cwords = 0;
    return HFPF_OK;
}

int hfpf_epoch_export(hfpf_handle* h, const void** dev_records, uint64_t* n_records)
{
    if (!h || !dev_records || !n_records) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rcf = flush_pending_locked(h)) return rcf;  // host frames still waiting for their launch
    uint64_t n = 0;
    int rc = check_usable(h);
    if (!rc) rc = epoch_export_locked(h, &n, 0);
    if (rc) return rc;
    h->epoch_used = true;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *dev_records = h->ex_send.p;
    *n_records = n;
    return HFPF_OK;
}

int hfpf_epoch_import(hfpf_handle* h, const void* dev_records, uint64_t n_records)
{
    if (!h || (!dev_records && n_records)) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rcf = flush_pending_locked(h)) return rcf;  // host frames still waiting for their launch
    h->epoch_used = true;
    int rc = epoch_import_locked(h, dev_records, n_records);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));  // the caller may reuse / free the record buffer
    h->ss.dirty = true;
    return HFPF_OK;
}

int hfpf_epoch_import_gathered(hfpf_handle* h, const void* dev_buffer, uint64_t slice_stride_bytes, int32_t world, int32_t my_rank, const uint64_t* counts)
{
    if (!h || !dev_buffer || !counts || world < 1 || my_rank < 0 || my_rank >= world) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rcf = flush_pending_locked(h)) return rcf;  // host frames still waiting for their launch
    if (int rc0 = check_usable(h)) return rc0;
    std::vector<unsigned long long> c(counts, counts + world);
    h->epoch_used = true;
    int rc = import_gathered_locked(h, dev_buffer, slice_stride_bytes, world, my_rank, c.data());
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));  // the caller may reuse / free the buffer
    h->ss.dirty = true;
    return HFPF_OK;
}

int hfpf_device_copy(hfpf_handle* h, void* dev_dst, const void* dev_src, uint64_t bytes)
{
    if (!h || (!dev_dst && bytes) || (!dev_src && bytes)) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (bytes) HIPCHK(h, hipMemcpyAsync(dev_dst, dev_src, (size_t)bytes, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HFPF_OK;
}

int hfpf_dist_unique_id(void* id128)
{
    if (!id128) return HFPF_ERR_BAD_ARG;
    std::string err;
    if (load_rccl(err)) return fail(nullptr, HFPF_ERR_DIST, "%s", err.c_str());
    ncclUniqueId_ id;
    int r = g_rccl.GetUniqueId(&id);
    if (r != ncclSuccess_) return fail(nullptr, HFPF_ERR_DIST, "ncclGetUniqueId failed: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    memcpy(id128, &id, sizeof id);
    return HFPF_OK;
}

int hfpf_dist_init(hfpf_handle* h, int rank, int world, const void* id128)
{
    if (!h || !id128 || world < 1 || rank < 0 || rank >= world) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (h->dist_on) return fail(h, HFPF_ERR_STATE, "hfpf_dist_init called twice");
    if (h->h_counts) { (void)hipHostFree(h->h_counts); h->h_counts = nullptr; }
    std::string err;
    if (load_rccl(err)) return fail(h, HFPF_ERR_DIST, "%s", err.c_str());
    ncclUniqueId_ id;
    memcpy(&id, id128, sizeof id);
    ncclComm_t_ comm = nullptr;
    NCCLCHK(h, g_rccl.CommInitRank(&comm, world, id, rank));
    h->comm = comm;
    h->rank = rank;
    h->world = world;
    HIPCHK(h, hipHostMalloc((void**)&h->h_counts, (size_t)(world + 1) * 8, hipHostMallocDefault));
    {  // exchange buffers for epochs of up to 4 M newly occupied cells per rank exist from here on; larger epochs grow them
        const uint64_t recs = std::min<uint64_t>(h->t.max_occ, 4ull << 20);
        int rc;
        unsigned long long *d_counts, *d_mine;
        if ((rc = scratch(h, h->ex_counts, ex_counts_layout(world, &d_counts, &d_mine))) || (rc = scratch(h, h->ex_send, recs * sizeof(EpochRec))) ||
            (rc = scratch(h, h->ex_recv, (size_t)world * recs * sizeof(EpochRec))))
            return rc;
        h->ex_cap_records = recs;
    }
    h->dist_on = true;
    return HFPF_OK;
}

int hfpf_dist_info(hfpf_handle* h, int32_t* rank, int32_t* world)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    int r = 0, w = 1;
    if (h->dist_on && h->comm) {  // what the communicator itself reports, not what the caller passed to hfpf_dist_init
        if (!g_rccl.CommCount || !g_rccl.CommUserRank) return fail(h, HFPF_ERR_DIST, "librccl lacks ncclCommCount / ncclCommUserRank");
        NCCLCHK(h, g_rccl.CommCount((ncclComm_t_)h->comm, &w));
        NCCLCHK(h, g_rccl.CommUserRank((ncclComm_t_)h->comm, &r));
    }
    if (rank) *rank = r;
    if (world) *world = w;
    return HFPF_OK;
}

int hfpf_dist_disable(hfpf_handle* h)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (h->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy((ncclComm_t_)h->comm);
    h->comm = nullptr;
    h->dist_on = false;
    h->rank = 0;
    h->world = 1;
    return HFPF_OK;
}

int hfpf_device_download(hfpf_handle* h, void* host_dst, const void* dev_src, uint64_t bytes)
{
    if (!h || !host_dst || !dev_src) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rcf = flush_pending_locked(h)) return rcf;  // host frames still waiting for their launch
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(host_dst, dev_src, (size_t)bytes, hipMemcpyDeviceToHost));
    return HFPF_OK;
}

void hfpf_free_rows(hfpf_row* rows) { free(rows); }

// hfpf_clear under the handle's lock (hfpf_restore begins with it).
static int clear_locked(hfpf_handle* h)
{
    h->ss.pend_n = 0;  // host frames still waiting for their launch would be wiped with the rest
    // how far the session got (the counters as the device has them now); a handle whose stream has failed is reset in full
    uint64_t bricks_used = ~0ull, normals_used = ~0ull;
    if (read_counters(h) == HFPF_OK) {
        bricks_used = h->h_ctr[C_BRICKS];
        normals_used = h->h_ctr[C_NORMALS];
    }
    int rc = reset_state(h, bricks_used, normals_used);
    h->ss.dirty = true;  // clearVoxels sets state_changed, grid.hpp:169
    return rc;
}

int hfpf_clear(hfpf_handle* h)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return clear_locked(h);
}

int hfpf_sync(hfpf_handle* h)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rcf = flush_pending_locked(h)) return rcf;  // host frames still waiting for their launch
    int rc = read_counters(h);
    if (rc) return rc;
    return poison_on_error(h, check_device_errors(h));
}

int hfpf_get_counters(hfpf_handle* h, hfpf_counters* out)
{
    if (!h || !out) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rcf = flush_pending_locked(h)) return rcf;  // host frames still waiting for their launch
    int rc = read_counters(h);
    if (rc) return rc;
    const unsigned long long* c = h->h_ctr;
    out->points_presented = c[C_PRESENTED];
    out->points_zclip_pass = c[C_ZPASS];
    out->points_in_bbox = c[C_INBOX];
    out->points_buffered = c[C_LOG];
    out->dep_pairs_tested = c[C_DEP_TESTED];
    out->dep_pairs_member = c[C_DEP_MEMBER];
    out->voxels_occupied = c[C_OCC];
    out->voxels_with_normal = c[C_NORMALS];
    out->bricks_allocated = std::min<uint64_t>(c[C_BRICKS], h->t.max_bricks);
    out->registrations = c[C_REG];
    out->dep_entries = c[C_DEP];  /* includes relocated (garbage) lists until the next compaction */
    out->frames_integrated = h->frames_integrated;
    out->clean_passes = h->clean_passes;
    out->device_bytes = h->device_bytes;
    out->replay_members = c[C_REPLAY_MEMBER];
    out->points_direct = c[C_BUFFERED];
    out->table_misses = c[C_TABLE_MISS];
    out->update_extra_rounds = c[C_UPD_ROUNDS];
    return HFPF_OK;
}

int hfpf_get_occupied(hfpf_handle* h, int32_t* xyz, uint64_t cap, uint64_t* n_out)
{
    if (!h || !n_out) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rcf = flush_pending_locked(h)) return rcf;  // host frames still waiting for their launch
    int rc = read_counters(h);
    if (rc) return rc;
    const uint64_t n = std::min<uint64_t>(h->h_ctr[C_OCC], h->t.max_occ);
    *n_out = n;
    if (!xyz || n == 0) return HFPF_OK;
    uint64_t *unsorted, *sorted; if ((rc = scratch_n(h, h->keys_a, n, &unsorted)) || (rc = scratch_n(h, h->keys_b, n, &sorted))) return rc;
    hipLaunchKernelGGL(k_occupied_keys, dim3(blocks_for(n, 256)), dim3(256), 0, h->stream, h->g, h->t, n, unsorted);
    HIPCHK(h, hipGetLastError());
    if ((rc = sort_keys_u64(h, unsorted, sorted, n))) return rc;
    std::vector<uint64_t> keys(n);
    HIPCHK(h, hipMemcpyAsync(keys.data(), sorted, n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (uint64_t i = 0; i < std::min(n, cap); i++) key_coords(h->g, keys[i], xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    return HFPF_OK;
}

int hfpf_device_alloc(hfpf_handle* h, uint64_t bytes, void** dev_ptr)
{
    if (!h || !dev_ptr) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMalloc(dev_ptr, (size_t)std::max<uint64_t>(bytes, 1)));
    return HFPF_OK;
}

int hfpf_device_free(hfpf_handle* h, void* dev_ptr)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipFree(dev_ptr));
    return HFPF_OK;
}

int hfpf_device_upload(hfpf_handle* h, void* dev_dst, const void* host_src, uint64_t bytes)
{
    if (!h || !dev_dst || !host_src) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpy(dev_dst, host_src, (size_t)bytes, hipMemcpyHostToDevice));
    return HFPF_OK;
}

int hfpf_kernel_timing(hfpf_handle* h, int enable)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rcf = flush_pending_locked(h)) return rcf;  // host frames still waiting for their launch
    int rc = resolve_timing(h);
    if (rc) return rc;
    h->timing = enable != 0;
    h->timing_detail = enable == 2;
    if (enable) {
        for (TimedId& t : h->timed) t.ms = 0, t.n = 0;
    }
    return HFPF_OK;
}

int hfpf_get_kernel_time(hfpf_handle* h, int kernel_id, double* total_ms, uint64_t* launches)
{
    if (!h || kernel_id < 0 || kernel_id >= kTimedIds) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rcf = flush_pending_locked(h)) return rcf;  // host frames still waiting for their launch
    int rc = resolve_timing(h);
    if (rc) return rc;
    if (total_ms) *total_ms = h->timed[kernel_id].ms;
    if (launches) *launches = h->timed[kernel_id].n;
    return HFPF_OK;
}

}  // extern "C"

// ================================================================================================
// What is no part of the hot path and builds on everything above, one unit each; nothing above names them.
#include "snapshot.hpp"
#include "probe.hpp"
#include "file_io.hpp"
