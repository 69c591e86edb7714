// csrc/kernels.hpp -- HIP kernels of the fusion path (gfx950, 64-wide waves).
//
//   K1 k_integrate        decode + z-clip + SE(3) + bbox clip + voxel index + brick claim + first occupancy; what is left to do
//                         with a point (buffer it / update its cell's dependants) is parked in its brick's bin, region A
//                         (cell has a normal) or B (it has none) (node.cpp:190-214,251-255,289; grid.hpp:194-243)
//   K2 k_update           region A: dependant updates per brick, LDS-staged statistic records, one flush per record (grid.hpp:244-277)
//      k_buffer           region B: the brick's buffered points go to the point log as one run, chained per cell (grid.hpp:210-211,230,239)
//      (k_integrate<.., BIN=false>, and lanes whose bin region is full, keep the direct forms: log append + one memory-side
//      atomic segment per (point, dependant) pair)
//      k_bin_plan/clamp   per-brick bin regions of the next launch from the previous launch's demand
//   K3 k_gate             5x5x5 occupancy count and the >gate test            (grid.hpp:322-352)
//   K4 k_normal           plane fit on occupied neighbour centres, orientation (grid.hpp:356-398)
//   K5 k_register         +-K line walk, dependant registration (grid.hpp:403-417,443-449)
//      k_link_log         chains the point-log entries the direct form appended since the last clean (4 interleaved chains per cell)
//      k_replay           buffer replay of the cells that gained registrants (grid.hpp:418-440)
//      k_replay_reg       the same, one walk per registration of the pass, before the dependant-table update
//      k_depinc_*/k_dep_* incremental update / compacting rebuild of the per-cell dependant table
//   K6 k_extract_*        ordered compaction of normal_found voxels            (grid.hpp:463-480)
//      k_epoch_*          multi-GPU exchange of newly occupied cells
#pragma once
#include <type_traits>

#include "host_plan.hpp"  // hide_word_op (constexpr: host and device)
#include "stats.hpp"
#include "view.hpp"       // the pinhole view: Pinhole, view_depth / view_pixel, view_radius

namespace hfpf {

typedef float vf4 __attribute__((ext_vector_type(4)));  // native vector type (the nontemporal builtins do not take HIP's float4)

struct FrameLayout {
    uint32_t point_step, off_x, off_y, off_z, off_rgb;
};

// A batch of registered depth + colour images (hfpf_integrate_depth*): frame f's depth image at frames + f * frame_stride (the
// kernel's own arguments), its colour image at color + f * color_stride.  Every frame of a launch has the same size, formats and
// intrinsics (the host batches only such frames).  Pixel (u, v) is point i = v * width + u.
struct DepthLayout {
    const uint8_t* color;  // nullptr when color_bpp == 0
    uint64_t color_stride;
    uint32_t width, depth_step, color_step;
    uint32_t depth_f32;   // 0: uint16 counts, 1: f32 metres
    uint32_t color_bpp;   // 0 (no colour: rgb = 0), 3 or 4 bytes per pixel
    uint32_t color_bgr;   // 1: blue first
    float cx, cy, sx, sy, unit;  // depth_backproject's constants, host-rounded
};

// Issue the loads of pixel i of one depth frame: returns (depth sample bits, 0x00RRGGBB, u, v) as raw bits, so that the caller
// can carry it across a tile like a packed record and convert it where it is used.  Sub-dword loads only: a row is never read
// past u's own bytes, so no load crosses the end of a row's step or of the image (an RGB8 pixel is three byte loads).
// WANT_RGB = false skips the colour bytes (the session does not fuse colour; rgb = 0).
template <bool WANT_RGB>
__device__ __forceinline__ vf4 depth_fetch(const uint8_t* __restrict__ dimg, const uint8_t* __restrict__ cimg, const DepthLayout& L, uint32_t i)
{
    const uint32_t v = i / L.width, u = i - v * L.width;
    const uint8_t* drow = dimg + (uint64_t)v * L.depth_step;
    const uint32_t raw = L.depth_f32 ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(drow) + u)
                                     : (uint32_t)__builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(drow) + u);
    uint32_t rgb = 0;
    if (WANT_RGB && L.color_bpp) {
        const uint8_t* px = cimg + (uint64_t)v * L.color_step + (uint64_t)u * L.color_bpp;
        if (L.color_bpp == 4) {
            const uint32_t w = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(px));
            rgb = color_pack(w & 0xFFu, (w >> 8) & 0xFFu, (w >> 16) & 0xFFu, L.color_bgr != 0);
        } else {
            rgb = color_pack(px[0], px[1], px[2], L.color_bgr != 0);
        }
    }
    return vf4{__uint_as_float(raw), __uint_as_float(rgb), __uint_as_float(u), __uint_as_float(v)};
}

// Camera-frame point of a fetched depth pixel (depth_fetch's (raw, rgb, u, v)).
__device__ __forceinline__ F3 depth_point(const DepthLayout& L, const vf4 r)
{
    return depth_backproject(__float_as_uint(r.z), __float_as_uint(r.w), __float_as_uint(r.x), L.depth_f32 != 0, L.cx, L.cy, L.sx, L.sy, L.unit);
}

// The three forms an input frame takes (the host picks one per launch): 16-byte (x, y, z, rgb) records, records of any
// FrameLayout, or a registered depth image (DepthLayout).
enum PointForm : int { kFormPacked16 = 0, kFormStrided = 1, kFormDepth = 2 };
template <int FORM>
using PointLayout = std::conditional_t<FORM == kFormDepth, DepthLayout, FrameLayout>;

// Camera-frame x, y, z of point i of a frame (the colour is not read): record i, or pixel i back-projected.
template <int FORM>
__device__ __forceinline__ F3 load_point(const uint8_t* __restrict__ frame, const PointLayout<FORM>& lay, const uint64_t i)
{
    if constexpr (FORM == kFormDepth) {
        return depth_point(lay, depth_fetch<false>(frame, nullptr, lay, (uint32_t)i));
    } else if constexpr (FORM == kFormPacked16) {
        const vf4 r = reinterpret_cast<const vf4*>(frame)[i];
        return F3{r.x, r.y, r.z};
    } else {
        const uint8_t* rec = frame + i * lay.point_step;
        return F3{*reinterpret_cast<const float*>(rec + lay.off_x), *reinterpret_cast<const float*>(rec + lay.off_y),
                  *reinterpret_cast<const float*>(rec + lay.off_z)};
    }
}

// ------------------------------------------------------------------------------------------------
// K1.  Persistent grid: block b walks tiles b, b+gridDim.x, ... of 256 consecutive points; a tile never
// straddles two frames, so the pose stays in scalar registers.  Loop trip counts are wave-uniform, which
// keeps the ballot/shuffle helpers convergent.
//
// Hot-counter discipline: one same-address device atomic costs ~12 ns at the memory side whatever the
// issuer (MI355X_MICROARCH.md "fanin"), so diagnostics stay in registers until the block retires and the
// point log is striped over kLogRegions append regions with one counter per 128-byte line.
//
// Dependant updates, direct form (BIN = false, and the fallback of the binned form): every (point, dependant) pair
// inside the 1 mm cylinder adds 5 int64 words (8 with colour) to ONE 64-byte statistics record.  A lane-per-pair loop would issue
// as many fully scattered atomic instructions per round (320 memory-side requests); instead the member lanes park their deltas
// in a per-wave LDS queue and the wave replays the queue with 8 lanes per record, so one wave-instruction carries 8 whole
// records as one 64-byte segment each.  That form saturates the chip's ~20 G requests/s atomic unit (41 M per launch).
// Binned form (BIN = true, default): the point is parked in its brick's bin and k_update does the pairs brick by brick.
#ifndef HFPF_REPLAY_B
#define HFPF_REPLAY_B 3  // registrants per chain walk held in registers by k_replay
#endif
constexpr int kLogRegions = 64;
#ifndef HFPF_LOG_CHAINS
#define HFPF_LOG_CHAINS 4
#endif
constexpr uint32_t kLogChains = HFPF_LOG_CHAINS;  // interleaved chains per cell (= kChains below: entry e joins chain e mod kLogChains of its cell)
constexpr uint32_t kLogUnlinked = 0x80000000u;  // log entry .w = slot | this bit until the entry is chained (then: index of the next entry)
#ifndef HFPF_REG_TILES
#define HFPF_REG_TILES 8  // 256-voxel tiles one workgroup of k_register takes per list reservation
#endif
constexpr int kRegTilesLarge = HFPF_REG_TILES, kRegTilesSmall = 2;
constexpr int kImportTiles = HFPF_REG_TILES;  // k_epoch_import: tiles per workgroup (one occ_list reservation)
// Passed instead of an element count: the kernel reads the exact count from its device counter and the host sizes the grid
// from an upper bound, which saves a host round trip between two kernels of a clean pass.
constexpr uint64_t kCountOnDevice = ~0ull;
constexpr int kListTiles = 4;  // same idea for the k_depinc_* list builders (not k_gate: it is latency-heavy per cell and needs every workgroup it can get)

// Wave-cooperative flush of statistic deltas: lanes with `member` park their delta (5 words, + 3 colour sums, + record id)
// in the wave's LDS queue, kQueueRows at a time, and the wave replays the queue with 8 lanes per record, so one
// wave-instruction carries 8 whole 64-byte records (one memory-side atomic segment each).  Convergent (all 64 lanes must call).
constexpr int kQueueStride = 11;  // u64 words per queued delta; odd stride spreads LDS banks
constexpr int kQueueRows = 8;     // deltas staged per round (the queue is 704 bytes per wave: the direct form is the rare path)
template <bool COLOR>
__device__ __forceinline__ void wave_flush_members(const Tables& t, unsigned long long* q, bool member, const StatDeltaT<COLOR>& d, uint32_t sid)
{
    constexpr int W = COLOR ? 8 : kStatUsed;
    const unsigned long long mm = __ballot(member);
    if (mm == 0) return;
    const uint32_t lane = lane_id();
    const uint32_t n_mem = (uint32_t)__popcll(mm);
    const uint32_t rank = (uint32_t)__popcll(mm & ((1ull << lane) - 1ull));
    for (uint32_t r0 = 0; r0 < n_mem; r0 += (uint32_t)kQueueRows) {  // wave-uniform trip count
        if (member && rank >= r0 && rank < r0 + (uint32_t)kQueueRows) {
            unsigned long long* r = q + (rank - r0) * kQueueStride;
#pragma unroll
            for (int w = 0; w < kStatUsed; w++) r[w] = (unsigned long long)d.v[w];
            if constexpr (COLOR) {
                r[SW_R] = (unsigned long long)d.rgb[0];
                r[SW_G] = (unsigned long long)d.rgb[1];
                r[SW_B] = (unsigned long long)d.rgb[2];
            }
            r[8] = sid;
        }
        // same-wave LDS hand-off: DS operations of one wave execute in order; the fences only pin the compiler
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        {
            const uint32_t w = lane & 7u, row = lane >> 3;
            if (r0 + row < n_mem && w < (uint32_t)W) {
                const unsigned long long* r = q + row * kQueueStride;
                atomicAdd(&t.stats[(uint64_t)r[8] * kStatWords + w], r[w]);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

constexpr int kOccStage = 256;  // newly occupied cells ONE WAVE of k_integrate stages before appending them to occ_list
// Append the wave's staged slots with ONE atomic on C_OCC.  Wave-level only (no workgroup barrier, so waves never have to agree on
// when to flush); `n` is wave-uniform.  Convergent for the wave.
__device__ __forceinline__ void flush_occ_stage(const Tables& t, const uint32_t* s_occ, uint32_t n)
{
    const uint32_t lane = lane_id();
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&t.ctr[C_OCC], (unsigned long long)n);
    base = __shfl(base, 0);
    // same-wave LDS hand-off: DS operations of one wave execute in order; the fences only pin the compiler
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    bool overflow = false;
    for (uint32_t k = lane; k < n; k += 64) {
        const unsigned long long oi = base + k;
        if (oi < t.max_occ) t.occ_list[oi] = s_occ[k];
        else overflow = true;
    }
    if (overflow) atomicOr(&t.ctr[C_ERR], (unsigned long long)E_OCC);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Inclusive prefix sum over the 64 lanes of a wave on the DPP data path: four row shifts and two row broadcasts, six VALU
// instructions and no LDS traffic (__shfl_up is a ds_bpermute per step: ~60 cycles of LDS-crossbar latency each, in a chain).
#ifndef HFPF_DPP_SCAN
#define HFPF_DPP_SCAN 1
#endif
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v)
{
#if HFPF_DPP_SCAN
    int x = (int)v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, true);   // row_shr:1, zero shifted in
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, true);   // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true);   // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true);   // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);  // row_bcast:15 into rows 1 and 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);  // row_bcast:31 into rows 2 and 3
    return (uint32_t)x;
#else
    const uint32_t lane = lane_id();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t a = __shfl_up(v, o);
        if (lane >= (uint32_t)o) v += a;
    }
    return v;
#endif
}

__device__ __forceinline__ DepEntry make_dep_entry(const Tables& t, uint32_t nid)  // (nv_line holds every record's line in the layout of a dependant entry)
{
    return *reinterpret_cast<const DepEntry*>(&t.nv_line[2 * (uint64_t)nid]);
}
// A cell gained its first dependant: set its bit in the brick's flag line (read by k_integrate).
__device__ __forceinline__ void set_dep_flag(const Tables& t, uint32_t slot)
{
    uint64_t plane, bit;
    slot_plane_bit(slot, plane, bit);
    atomicOr(reinterpret_cast<unsigned long long*>(&t.nd_mask[plane * 2 + 1]), (unsigned long long)bit);
}
// The ONE dependant a cell can carry while it is unoccupied (grid.hpp:443-449: the last registrant wins) lives in pre_dep[slot]
// alone -- no list entry, no flag bit, nothing a clean pass has to write per unoccupied target but the atomicMax that settles the
// winner (most registration targets are unoccupied: 8 M of the 13.7 M in the bench's first pass, and on 0.5 mm voxels the slot
// arrays they used to touch fall out of the caches).  A cell that has become occupied gets the entry filed as its dependant list
// at the head of the next clean pass (k_materialize_new: list entry, info word, flag bit, a place in prereg_list for compacting
// rebuilds).  In between -- the cell was occupied in the running epoch -- whoever reads dependant lists while points arrive
// (k_update_cells, k_update, k_integrate_overflow, the un-binned k_integrate) takes an EMPTY list of an occupied cell to mean
// "look at pre_dep": the one entry is the record's own line, which nv_line keeps in the layout of a dependant entry.
__device__ __forceinline__ void pre_list_entry(const Tables& t, uint32_t nid, float4& e0, float4& e1)  // = the two halves of make_dep_entry(t, nid)
{
    e0 = t.nv_line[2 * (uint64_t)nid];
    e1 = t.nv_line[2 * (uint64_t)nid + 1];
}

// The direct forms of buffering (grid.hpp:205-243) and of the dependant update (grid.hpp:244-277) for one point per lane: the whole
// path of the un-binned engine (BIN = false, inline in k_integrate), and in the binned one what k_integrate_overflow does with the
// few points that found no room in their brick's bin.  Convergent for the wave (every lane calls; `todo` says which have a point).
constexpr uint32_t kOvfHasNormal = 0x80000000u, kOvfHasDeps = 0x40000000u;  // flags beside the frame id (< 2^23, host-checked) in Tables::ovf_aux
template <bool COLOR, bool BIN>
__device__ __forceinline__ void direct_buffer(const Tables& t, unsigned long long* log_ctr, const uint64_t log_base, const F3 p, const uint32_t slot, const uint32_t b,
                                              const uint32_t fid, const uint32_t rgb, const bool todo, const bool has_n, uint32_t& c_buf)
{
    // direct buffering; the viewpoint latch (smallest frame id that touched the cell, grid.hpp:229,238) is only ever
    // read before the normal exists
    const bool buf = todo && !has_n;
    if (buf && fid < t.first_frame[slot]) atomicMin(&t.first_frame[slot], fid);
    const unsigned long long li = wave_reserve(log_ctr, buf);
    if (buf) {
        if (li < t.log_region_cap) {
            const uint64_t e = log_base + li + 1;
            // Binned form: this is the rare lane whose bin region was full, so it chains its entry right here (one returning
            // atomic) and no pass over the log is needed afterwards.  Direct form (every point comes this way): .w carries the
            // marked slot until k_link_log chains the entries of the epoch in one go.
            uint32_t link = slot | kLogUnlinked;
            if (BIN) {
                link = atomicExch(&t.buf_head[(uint64_t)slot * kLogChains + ((uint32_t)e & (kLogChains - 1))], (uint32_t)e);
                if (!(t.run_cnt[b] & 0x100u)) atomicOr(&t.run_cnt[b], 0x100u);  // an entry outside the brick's runs: its replay walks the chains
            }
            t.log_pt[e] = make_float4(p.x, p.y, p.z, __uint_as_float(link));
            if (COLOR) t.log_rgb[e] = rgb;
        } else {
            atomicOr(&t.ctr[C_ERR], (unsigned long long)E_LOG);
        }
    }
    c_buf += buf;
}

template <bool COLOR, bool BIN>
__device__ __forceinline__ void direct_forms(const GridParams& g, const Tables& t, unsigned long long* q, unsigned long long* log_ctr, const uint64_t log_base,
                                             const F3 p, const uint32_t slot, const uint32_t b, const uint32_t fid, const uint32_t rgb, const bool todo,
                                             const bool has_n, const bool has_d, const uint32_t pre_nid, uint32_t& c_buf, uint32_t& c_tested, uint32_t& c_member)
{
    direct_buffer<COLOR, BIN>(t, log_ctr, log_base, p, slot, b, fid, rgb, todo, has_n, c_buf);

    // direct dependant updates.  pre_nid != 0: the cell was occupied in the running epoch and has no list yet, only the dependant it
    // was given while unoccupied (pre_list_entry): the point is tested against that record's own line.
    const bool direct = todo && has_d;
    uint32_t cnt = 0;
    uint64_t off = 0;
    if (direct) {
        if (pre_nid) {
            cnt = 1;
        } else {
            const uint64_t info = t.info[slot];
            cnt = (uint32_t)((info >> kDepCntShift) & kDepCntMask);
            off = info >> kDepOffShift;
        }
    }
    uint32_t max_cnt = cnt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) max_cnt = max(max_cnt, (uint32_t)__shfl_xor((int)max_cnt, o));
    for (uint32_t j = 0; j < max_cnt; j++) {
        bool member = false;
        StatDeltaT<COLOR> d;
        stat_delta_zero(d);
        uint32_t sid = 0;
        if (j < cnt) {
            const DepEntry e = pre_nid ? make_dep_entry(t, pre_nid) : t.dep[off + j];
            float sp, distf;
            c_tested++;
            if (line_member(g, p, F3{e.ax, e.ay, e.az}, F3{e.abx, e.aby, e.abz}, e.dd, sp, distf)) {
                member = true;
                c_member++;
                sid = e.sid;
                stat_delta_add(d, pair_delta(g, sp, distf), rgb);
            }
        }
        wave_flush_members(t, q, member, d, sid);
    }
}

// Grid constants and table descriptor of k_integrate as ONE struct and its FIRST argument, so that a field's place in the kernarg
// segment is offsetof(IntegrateArgs, field).  (The frame, pose and frame-id pointers stay separate __restrict__ arguments: that
// is what lets the compiler read the wave-uniform pose with scalar loads.)
struct IntegrateArgs {
    GridParams g;
    Tables t;
};
// The table descriptor as the RARE paths of the tile loop see it (a new brick, a newly occupied cell's list flush, a point
// without room in its bin, the one lane a frame that files the viewpoint): read from the kernarg segment where it is needed.
// The compiler treats by-value kernel arguments as loop invariants and keeps every field the loop mentions anywhere in scalar
// registers for its whole length -- some forty table bases and limits here, 37 of which it then parked in VGPR lanes, with a
// v_readlane / v_writelane wherever the tile body wanted one back.  The empty asm hides where the pointer comes from, so the
// scalar loads behind it stay inside the branch they are written in.
typedef const __attribute__((address_space(4))) char* kernarg_ptr;
__device__ __forceinline__ const Tables& kernarg_tables()
{
    kernarg_ptr p = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const Tables*)(p + offsetof(IntegrateArgs, t));
}

// Waves per SIMD: the tile loop is a chain of dependent table round trips, so resident waves are what hides them.  Seven for both
// forms.  The binned one (direct forms moved out to k_integrate_overflow) needs only 59 VGPRs, but 94 SGPRs a wave keep it at seven
// workgroups per CU all the same; asking the compiler for eight shrinks its SGPR budget (94 -> 78, 51 spills instead of 37) for
// nothing.  The un-binned form fits seven in 72 VGPRs without scratch.
#ifndef HFPF_INT_WAVES
#define HFPF_INT_WAVES 7
#endif
#ifndef HFPF_INT_WAVES_BIN
#define HFPF_INT_WAVES_BIN 7
#endif
// The three PointForms as two switches: PACKED16 = kFormPacked16, DEPTH = kFormDepth (each lane reads its pixel's samples and
// back-projects them in registers, depth_point), neither = kFormStrided.  The point and its colour are read here, not through
// load_point: the next tile's record or pixel is fetched ahead of this tile's table lookups, and the colour is needed too.
template <bool PACKED16, bool COLOR, bool BIN, bool DEPTH = false>
__global__ __launch_bounds__(256, BIN ? HFPF_INT_WAVES_BIN : HFPF_INT_WAVES) void k_integrate(const IntegrateArgs A, const uint8_t* __restrict__ frames,
                                                   const uint64_t frame_stride, const uint32_t n_pts, const uint32_t n_frames,
                                                   const std::conditional_t<DEPTH, DepthLayout, FrameLayout> lay, const double* __restrict__ poses,
                                                   const uint32_t* __restrict__ frame_ids, const uint32_t row_w, const uint32_t log_rot,
                                                   const uint32_t probe, const uint32_t pre_possible)
{
    // pre_possible: a clean pass has run, so unoccupied cells may carry a dependant (k_materialize_new)
    const GridParams& g = A.g;
    const Tables& t = A.t;
    // probe != 0: dry run of the batch's first frames for a session that has no bin plan yet -- transform, index, claim the
    // bricks and record the per-region demand; nothing else is touched (the frames come again in the real launch).
    __shared__ unsigned long long queue[4][kQueueRows * kQueueStride];
    __shared__ unsigned int blk_ctr[6];
    __shared__ uint32_t s_occ_all[4][kOccStage];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    unsigned long long* q = queue[wave];
    uint32_t* s_occ = s_occ_all[wave];
    uint32_t occ_n = 0;  // wave-uniform: slots staged by this wave
    if (threadIdx.x < 6) blk_ctr[threadIdx.x] = 0;
    __syncthreads();

    const uint32_t tiles_per_frame = (n_pts + 255u) >> 8;
    const uint64_t n_tiles = (uint64_t)tiles_per_frame * n_frames;  // < 2^32 (host-checked)
    // log_rot changes from launch to launch, so that launches with fewer than kLogRegions workgroups (small frames through
    // hfpf_integrate, one frame per call) still fill every append region of the log
    const uint32_t region = (blockIdx.x + log_rot) & (kLogRegions - 1);
    unsigned long long* log_ctr = &t.log_ctr[region * 16];
    const uint64_t log_base = (uint64_t)region * t.log_region_cap;
    uint32_t c_present = 0, c_z = 0, c_in = 0, c_buf = 0, c_tested = 0, c_member = 0;

    // Where tile `tl` sits: frame and point index of this thread.  row_w != 0 (host-checked: organised frame, width and rows
    // multiples of 16): the tile is a 16x16-pixel patch, whose points fall into ~2x2 bricks and half as many table lines as a
    // 256-pixel run of one image row; each wave takes one 8x8 quadrant of the patch (8 pixels x 16 B = one 128-byte line per
    // image row).  32-bit arithmetic: the host keeps n_tiles below 2^32.
    auto locate = [&](uint32_t tl, uint32_t& f_out, uint32_t& i_out) {
        f_out = tl / tiles_per_frame;
        const uint32_t tile_in_frame = tl - f_out * tiles_per_frame;
        i_out = tile_in_frame * 256u + threadIdx.x;
        if (row_w) {
            const uint32_t tiles_x = row_w >> 4, ty = tile_in_frame / tiles_x, tx = tile_in_frame - ty * tiles_x;
            const uint32_t px = ((threadIdx.x >> 6) & 1u) * 8u + (threadIdx.x & 7u), py = (threadIdx.x >> 7) * 8u + ((threadIdx.x >> 3) & 7u);
            i_out = (ty * 16u + py) * row_w + tx * 16u + px;
        }
    };
    // The frame read of the NEXT tile is issued before this tile's table lookups (packed records and depth images): the stream
    // from HBM is the longest latency of a tile and nothing in the tile depends on it but its own first instructions.
    uint32_t pre_f = 0, pre_i = 0;
    vf4 pre = {0.f, 0.f, 0.f, 0.f};
    const uint32_t n_tiles32 = (uint32_t)n_tiles;
    if (blockIdx.x < n_tiles32) {
        locate(blockIdx.x, pre_f, pre_i);
        if (PACKED16 && pre_i < n_pts)
            pre = __builtin_nontemporal_load(reinterpret_cast<const vf4*>(frames + (uint64_t)pre_f * frame_stride) + pre_i);  // read once
        if constexpr (DEPTH)
            if (pre_i < n_pts) pre = depth_fetch<COLOR>(frames + (uint64_t)pre_f * frame_stride, lay.color + (uint64_t)pre_f * lay.color_stride, lay, pre_i);
    }
    for (uint32_t tile = blockIdx.x; tile < n_tiles32; tile += gridDim.x) {
        const uint32_t f = pre_f, i = pre_i;
        const vf4 nv = pre;
        if (tile + gridDim.x < n_tiles32) {
            locate(tile + gridDim.x, pre_f, pre_i);
            if (PACKED16 && pre_i < n_pts)
                pre = __builtin_nontemporal_load(reinterpret_cast<const vf4*>(frames + (uint64_t)pre_f * frame_stride) + pre_i);
            if constexpr (DEPTH)
                if (pre_i < n_pts) pre = depth_fetch<COLOR>(frames + (uint64_t)pre_f * frame_stride, lay.color + (uint64_t)pre_f * lay.color_stride, lay, pre_i);
        }
        double T[12];
#pragma unroll
        for (int k = 0; k < 12; k++) T[k] = poses[12 * f + k];
        const uint32_t fid = frame_ids[f];
        if (i == 0) {  // viewpoint = float(translation), node.cpp:290
            const Tables& tr = BIN ? kernarg_tables() : t;
            float* vp = tr.frame_vp + 3 * (uint64_t)fid;
            vp[0] = (float)T[3];
            vp[1] = (float)T[7];
            vp[2] = (float)T[11];
            if (!probe) {  // the frames this rank has integrated: what the next epoch exchange sends viewpoints for
                const unsigned long long fi = atomicAdd(&tr.ctr[C_FRAMES], 1ull);
                if (fi < tr.max_frames) tr.frame_list[fi] = fid;  // (ids are below max_frames: the list only fills up when ids repeat, and then they are in it)
            }
        }
        const uint8_t* __restrict__ base = frames + (uint64_t)f * frame_stride;
        bool act = i < n_pts;
        float x = 0.f, y = 0.f, z = 0.f;
        uint32_t rgb = 0;
        if (act) {
            if constexpr (DEPTH) {
                const F3 c = depth_point(lay, nv);
                x = c.x;
                y = c.y;
                z = c.z;
                rgb = __float_as_uint(nv.y);
            } else if (PACKED16) {
                x = nv.x;
                y = nv.y;
                z = nv.z;
                rgb = __float_as_uint(nv.w);
            } else {
                const uint8_t* rec = base + (uint64_t)i * lay.point_step;
                x = *reinterpret_cast<const float*>(rec + lay.off_x);
                y = *reinterpret_cast<const float*>(rec + lay.off_y);
                z = *reinterpret_cast<const float*>(rec + lay.off_z);
                rgb = *reinterpret_cast<const uint32_t*>(rec + lay.off_rgb);
            }
        }
        c_present += act;
        act = act && zclip_pass(g, z);
        c_z += act;
        const F3 p = transform_point(T, x, y, z);
        int32_t ix, iy, iz;
        voxel_coords(g, p, ix, iy, iz);
        // A NaN coordinate passes validPoints in the reference and then indexes out of bounds (crash); dropped here.
        act = act && valid_point(g, p) && ix != INT_MIN && iy != INT_MIN && iz != INT_MIN;
        c_in += act;

        const uint32_t bidx = act ? brick_index(g, ix, iy, iz) : 0u;
        uint32_t dir_word = 0;
        if (act) dir_word = t.dir[bidx];  // issued here, needed after the grouping loop below
        // Lanes of the same brick, as a mask per lane (registers and scalar lane reads only): the loop runs while the directory
        // read is in flight, and the bin reservation further down needs no loop of its own.
        unsigned long long same_brick = 0;
        if (BIN) {
            unsigned long long m = __ballot(act);
            while (m) {
                const int leader = __ffsll((long long)m) - 1;
                const uint32_t lb = (uint32_t)__builtin_amdgcn_readlane((int)bidx, leader);
                const bool same = act && bidx == lb;
                const unsigned long long sm = __ballot(same);
                if (same) same_brick = sm;
                m &= ~sm;
            }
        }
        const uint32_t b = BIN ? brick_acquire_groups(t, bidx, act, dir_word, same_brick, true) : brick_acquire_wave(t, bidx, act, dir_word);
        act = act && b != 0;
        const uint32_t lcell = local_index(ix, iy, iz);
        const uint32_t slot = b * kBrickCells + lcell;
        // What to do with the point is two bits of its cell: normal_found (stop buffering, grid.hpp:210) and has-dependants.
        // Both come from the brick's 128-byte flag line (L2-resident) instead of the cell's 8-byte info word.  The occupancy
        // word of the cell's plane is read in the same round trip (it is only needed while the cell has no normal).
        const uint64_t plane = (uint64_t)b * 8u + ((uint32_t)ix & 7u);
        const uint64_t bit = 1ull << ((((uint32_t)iy & 7u) << 3) | ((uint32_t)iz & 7u));
        bool has_n = false, has_d = false;
        unsigned long long occ_word = ~0ull;
        if (act) {
            const ulonglong2 nd = *reinterpret_cast<const ulonglong2*>(&t.nd_mask[plane * 2]);
            occ_word = *reinterpret_cast<const unsigned long long*>(&t.occ_mask[plane]);
            has_n = (nd.x & bit) != 0;
            has_d = (nd.y & bit) != 0;
        }

        // first occupancy (grid.hpp:219-243): the returning atomic on the brick's occupancy word decides who is first
        bool first = false;
        if (act && !has_n && !probe && !(occ_word & bit)) {  // a stale (cached) word only sends the lane through the atomic
            unsigned long long* om = reinterpret_cast<unsigned long long*>(&t.occ_mask[plane]);
            const unsigned long long old = atomicOr(om, (unsigned long long)bit);
            first = !(old & bit);  // (occupancy lives in occ_mask alone; the cell's info word is not touched)
        }
        // A cell occupied since the last clean pass has no list and no flag yet, but it may carry the ONE dependant it was given
        // while unoccupied (pre_dep, see k_materialize_new): every reader of the lists falls back on it.  The binned form parks
        // every point of a cell without a normal anyway and its per-brick kernels do the looking; the direct form looks here.
        uint32_t pre_nid = 0;
        if (!BIN && pre_possible && act && !has_n && !has_d && !probe) {
            pre_nid = t.pre_dep[slot];
            has_d = pre_nid != 0;
        }
        // newly occupied cells are staged in LDS (per wave) and appended to occ_list in batches: C_OCC is one address for the
        // whole chip (a same-address atomic retires every ~12 ns), so it gets one atomic per flush, not one per tile.  The
        // count lives in a wave-uniform register, so no two waves ever have to agree on a flush (no barrier in the tile loop).
        {
            const unsigned long long fm = __ballot(first);
            if (fm) {
                if (occ_n + 64u > (uint32_t)kOccStage) {
                    flush_occ_stage(BIN ? kernarg_tables() : t, s_occ, occ_n);
                    occ_n = 0;
                }
                if (first) s_occ[occ_n + (uint32_t)__popcll(fm & ((1ull << lane) - 1ull))] = slot;
                occ_n += (uint32_t)__popcll(fm);
            }
        }

        // What is left to do with the point: buffer it while its voxel has no normal (grid.hpp:210-211,230,239) and update the
        // voxel's dependants (grid.hpp:244-277).  Binned form (BIN = true, default): both are handed to the per-brick kernels --
        // the point is parked in its brick's bin, k_update accumulates the brick's records in LDS and flushes each once per
        // launch, k_buffer appends the brick's buffered points to the log as one run and links them into their cells' chains
        // with LDS exchanges.  One reservation per distinct brick per wave (ballot grouping); a lane whose brick region is
        // full or unplanned stays `todo` and takes the direct forms below, so correctness never depends on the plan.
        bool todo = act && (has_d || !has_n);
        if (BIN) {
            const bool want_bin = todo;
            // phase 1 (registers only): the lane's group = the lanes of its bin region (brick x {cell has a normal, cell has
            // none}) -> leader lane, rank in group, group size
            const uint32_t rg = 2u * b + (has_n ? 0u : 1u);
            const unsigned long long hn = __ballot(has_n);
            const unsigned long long grp = same_brick & __ballot(want_bin) & (has_n ? hn : ~hn);
            const uint32_t grp_leader = want_bin ? (uint32_t)(__ffsll((long long)grp) - 1) : lane;
            const uint32_t grp_rank = (uint32_t)__popcll(grp & ((1ull << lane) - 1ull));
            const uint32_t grp_size = (uint32_t)__popcll(grp);
            // phase 2: every group leader reserves for its group in ONE wave-instruction (one memory round trip per tile);
            // the counter also records the demand the next launch's plan is made from
            uint32_t base = 0, cap = 0, roff = 0;
            if (want_bin && grp_leader == lane) {
                base = atomicAdd(&t.bin_fill[rg], grp_size);
                cap = t.bin_capb[rg];
                roff = t.bin_off[rg];
            }
            base = __shfl(base, (int)grp_leader);
            cap = __shfl(cap, (int)grp_leader);
            roff = __shfl(roff, (int)grp_leader);
            if (todo && !probe) {
                const uint32_t pos = base + grp_rank;
                if (pos < cap) {
                    const uint64_t e = (uint64_t)roff + pos;
                    // the point + its cell inside the brick + its frame id (viewpoint latch); read back by k_update / k_buffer
                    t.bin_pt[e] = make_float4(p.x, p.y, p.z, __uint_as_float(lcell | (fid << 9)));
                    if (COLOR) t.bin_rgb[e] = rgb;
                    todo = false;
                }
            }
        }
        if (probe || __ballot(todo) == 0) continue;  // wave-uniform; the common case of the binned form

        if constexpr (BIN) {
            // The rare lane whose bin region was full or unplanned: handed, with what the direct forms need, to k_integrate_overflow,
            // which runs behind this kernel.  Keeping the direct forms out of the tile loop halves the scalar state this kernel
            // spills into VGPR lanes (60 -> 37 SGPRs) and 13 VGPRs, and no wave waits in the loop for a lane that walks a dependant list.
            const Tables& tr = kernarg_tables();
            const unsigned long long oi = wave_reserve(&tr.ctr[C_OVF], todo);
            if (todo) {
                if (oi < tr.ovf_cap) {
                    tr.ovf_pt[oi] = make_float4(p.x, p.y, p.z, __uint_as_float(slot));
                    tr.ovf_aux[oi] = make_uint2(fid | (has_n ? kOvfHasNormal : 0u) | (has_d ? kOvfHasDeps : 0u), rgb);
                } else {
                    atomicOr(&tr.ctr[C_ERR], (unsigned long long)E_OVF);  // (the list holds a whole launch: cannot happen)
                }
            }
        } else {
            direct_forms<COLOR, false>(g, t, q, log_ctr, log_base, p, slot, b, fid, rgb, todo, has_n, has_d, pre_nid, c_buf, c_tested, c_member);
        }
    }
    if (occ_n) flush_occ_stage(t, s_occ, occ_n);  // wave-uniform
    // block-level reduction of the diagnostics: one device atomic per counter per block
    uint32_t cv[6] = {c_present, c_z, c_in, c_buf, c_tested, c_member};
#pragma unroll
    for (int k = 0; k < 6; k++) {
        uint32_t v = cv[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
        cv[k] = v;
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; k++)
            if (cv[k]) atomicAdd(&blk_ctr[k], cv[k]);
    }
    __syncthreads();
    if (!probe && threadIdx.x < 6 && blk_ctr[threadIdx.x]) atomicAdd(&t.ctr[C_PRESENTED + threadIdx.x], (unsigned long long)blk_ctr[threadIdx.x]);
}


// K1b (binned form): the points k_integrate could not park (bin region full, brick unplanned or found within the launch after the
// spare regions ran out: 0.3 % of the bench's points) take the direct forms here, right behind it on the stream.  The list is sized
// for a whole launch, so a session without a bin plan (its first small batch) comes through here entirely.  A workgroup takes 256
// points at a time: one lane per point for the buffering, then one lane per (point, dependant) PAIR -- the pairs of the 256 points
// are numbered through a prefix sum of the list lengths, so a point on a cell with twenty dependants does not hold its wave for
// twenty dependent reads.  The list is reset by the next launch's bin plan (k_bin_place; the host where there is no plan).
template <bool COLOR>
__global__ __launch_bounds__(256) void k_integrate_overflow(const GridParams g, const Tables t, const uint32_t log_rot)
{
    __shared__ unsigned long long queue[4][kQueueRows * kQueueStride];
    __shared__ unsigned int blk_ctr[3];
    __shared__ float s_x[256], s_y[256], s_z[256];
    __shared__ uint32_t s_rgb[COLOR ? 256 : 1];
    __shared__ uint32_t s_off[256];    // first dependant entry of the point's cell (dep[] stays below 2^32 entries, host-checked), or ...
    __shared__ uint8_t s_pre[256];     // ... 1: the record id of the cell's pre-dependant (cell occupied in this epoch: pre_list_entry)
    __shared__ uint32_t s_pref[257];   // pairs in front of the point
    __shared__ uint32_t s_wsum[4];
    const uint64_t n = min((uint64_t)t.ctr[C_OVF], t.ovf_cap);  // the same in every thread of the grid (nothing appends while this kernel runs)
    if (n == 0) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    unsigned long long* q = queue[wave];
    if (tid < 3) blk_ctr[tid] = 0;
    __syncthreads();
    const uint32_t region = (blockIdx.x + log_rot) & (kLogRegions - 1);
    unsigned long long* log_ctr = &t.log_ctr[region * 16];
    const uint64_t log_base = (uint64_t)region * t.log_region_cap;
    uint32_t c_buf = 0, c_tested = 0, c_member = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < n; base += (uint64_t)gridDim.x * 256u) {  // block-uniform trip count
        const uint64_t i = base + tid;
        const bool todo = i < n;
        float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
        uint2 aux = make_uint2(0u, 0u);
        if (todo) {
            rec = t.ovf_pt[i];
            aux = t.ovf_aux[i];
        }
        const uint32_t slot = __float_as_uint(rec.w);
        uint32_t cnt = 0, off = 0;
        bool pre = false;
        if (todo && ((aux.x & kOvfHasDeps) || !(aux.x & kOvfHasNormal))) {  // issued before the buffering's atomics
            const uint64_t info = t.info[slot];
            cnt = (uint32_t)((info >> kDepCntShift) & kDepCntMask);
            off = (uint32_t)(info >> kDepOffShift);
            if (cnt == 0 && !(aux.x & kOvfHasNormal)) {  // no list yet: a cell occupied in this epoch may carry a pre-dependant
                off = t.pre_dep[slot];
                pre = off != 0;
                cnt = pre ? 1u : 0u;
            }
        }
        direct_buffer<COLOR, true>(t, log_ctr, log_base, F3{rec.x, rec.y, rec.z}, slot, slot >> 9, aux.x & ~(kOvfHasNormal | kOvfHasDeps), aux.y, todo,
                                   (aux.x & kOvfHasNormal) != 0, c_buf);
        const uint32_t inc = wave_inclusive_scan(cnt);
        if (lane == 63) s_wsum[wave] = inc;
        s_x[tid] = rec.x, s_y[tid] = rec.y, s_z[tid] = rec.z;
        if (COLOR) s_rgb[tid] = aux.y;
        s_off[tid] = off;
        s_pre[tid] = pre ? 1 : 0;
        __syncthreads();
        uint32_t before = inc - cnt;
        for (uint32_t w2 = 0; w2 < wave; w2++) before += s_wsum[w2];
        s_pref[tid] = before;
        if (tid == 255) s_pref[256] = before + cnt;
        __syncthreads();
        const uint32_t total = s_pref[256];
        for (uint32_t k0 = 0; k0 < total; k0 += 256u) {  // block-uniform trip count
            const uint32_t k = k0 + tid;
            bool member = false;
            StatDeltaT<COLOR> d;
            stat_delta_zero(d);
            uint32_t sid = 0;
            if (k < total) {
                uint32_t lo = 0, hi = 256;  // s_pref[lo] <= k < s_pref[hi]
#pragma unroll
                for (int st = 0; st < 8; st++) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (s_pref[mid] <= k) lo = mid;
                    else hi = mid;
                }
                const DepEntry e = s_pre[lo] ? make_dep_entry(t, s_off[lo]) : t.dep[(uint64_t)s_off[lo] + (k - s_pref[lo])];
                float sp, distf;
                c_tested++;
                if (line_member(g, F3{s_x[lo], s_y[lo], s_z[lo]}, F3{e.ax, e.ay, e.az}, F3{e.abx, e.aby, e.abz}, e.dd, sp, distf)) {
                    member = true;
                    c_member++;
                    sid = e.sid;
                    stat_delta_add(d, pair_delta(g, sp, distf), COLOR ? s_rgb[lo] : 0u);
                }
            }
            wave_flush_members(t, q, member, d, sid);
        }
        __syncthreads();  // the staged points are rewritten by the next round
    }
    uint32_t cv[3] = {c_buf, c_tested, c_member};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        uint32_t v = cv[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
        if (lane == 0 && v) atomicAdd(&blk_ctr[k], v);
    }
    __syncthreads();
    if (tid < 3 && blk_ctr[tid]) atomicAdd(&t.ctr[C_BUFFERED + tid], (unsigned long long)blk_ctr[tid]);
#ifdef HFPF_OVF_COUNT_DEBUG
    if (tid == 0 && blockIdx.x == 0) atomicAdd(&t.ctr[C_BUFFERED], (unsigned long long)n);
#endif
}

// ------------------------------------------------------------------------------------------------
// K2 (binned form): one workgroup per brick.  The brick's parked points are read back coalesced; a point finds its cell's
// dependant list through the brick's 512 info words (staged in LDS: k_integrate no longer reads them), and every
// (point, dependant) member pair adds its contribution (stats.hpp) to an LDS table keyed by record id (open addressing,
// LDS atomics).  The table is flushed with 8 lanes per record, so a record costs one 64-byte memory-side request per
// brick per launch however many of the brick's cells and points touched it.  A full table falls back to direct device
// atomics.  Tried instead and slower on the bench: points counting-sorted by cell in LDS with
// rows of lanes sharing a list (1.3 ms against 1.0: the sort, the row reductions and the barriers cost more than the
// broadcast reads save) and lists staged in LDS with a table indexed by list position (1.35 ms: 3.7x the flushes).
#ifndef HFPF_UPD_BITS
#define HFPF_UPD_BITS 9  // log2 of the LDS table size of k_update
#endif
constexpr int kUpdSlots = 1 << HFPF_UPD_BITS;
constexpr unsigned long long kPreListBit = 1ull << 63;  // in a staged info word: the list is the cell's pre-dependant alone (pre_list_entry)
constexpr int kUpdThreads = 256;
#ifndef HFPF_UPD_LANES
#define HFPF_UPD_LANES 2  // lanes that share one point in k_update (1, 2, 4 or 8)
#endif
constexpr uint32_t kUpdLanes = HFPF_UPD_LANES;
__device__ __forceinline__ uint32_t upd_hash(uint32_t sid) { return (sid * 2654435761u) >> (32 - HFPF_UPD_BITS); }

template <bool COLOR>
__global__ __launch_bounds__(256) void k_update(const GridParams g, const Tables t, const uint32_t n_bricks)
{
    constexpr int W = COLOR ? 8 : kStatUsed;
    __shared__ uint64_t s_info[kBrickCells];
    __shared__ uint32_t keys[kUpdSlots];
    __shared__ unsigned long long vals[kUpdSlots * W];
    __shared__ unsigned int blk_ctr[2];
    const uint32_t b = blockIdx.x + 1;
    if (b > n_bricks) return;
    // the brick's two bin regions (cells with / without a normal) as one index space [0, fill)
    const uint32_t fill_a = min(t.bin_fill[2 * b], t.bin_capb[2 * b]), fill_b = min(t.bin_fill[2 * b + 1], t.bin_capb[2 * b + 1]);
    const uint32_t fill = fill_a + fill_b;
    if (fill == 0) return;  // block-uniform
    const uint32_t tid = threadIdx.x;
    const uint64_t first_a = t.bin_off[2 * b], first_b = t.bin_off[2 * b + 1];
    auto entry = [&](uint32_t i) -> uint64_t { return i < fill_a ? first_a + i : first_b + (i - fill_a); };
    float4 pe = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid / kUpdLanes < fill) pe = t.bin_pt[entry(tid / kUpdLanes)];  // in flight while the tables are set up
    {
        ulonglong2 inf = *reinterpret_cast<const ulonglong2*>(&t.info[(uint64_t)b * kBrickCells + 2u * tid]);
        for (uint32_t i = tid; i < (uint32_t)kUpdSlots; i += 256) keys[i] = 0;
        for (uint32_t i = tid; i < (uint32_t)(kUpdSlots * W); i += 256) vals[i] = 0;
        if (tid < 2) blk_ctr[tid] = 0;
        // an empty list may belong to a cell occupied in this epoch that carries a pre-dependant: a list of one, marked by bit 63,
        // whose "offset" is the record id (pre_list_entry)
        auto with_pre = [&](unsigned long long info, uint32_t cell) -> unsigned long long {
            if ((info >> kDepCntShift) & kDepCntMask) return info;
            const uint32_t pd = t.pre_dep[(uint64_t)b * kBrickCells + cell];
            return pd ? ((info & 3ull) | (1ull << kDepCntShift) | ((unsigned long long)pd << kDepOffShift) | kPreListBit) : info;
        };
        inf.x = with_pre(inf.x, 2u * tid);
        inf.y = with_pre(inf.y, 2u * tid + 1u);
        s_info[2u * tid] = inf.x;
        s_info[2u * tid + 1] = inf.y;
    }
    __syncthreads();
    const float4* __restrict__ dep4 = reinterpret_cast<const float4*>(t.dep);
    uint32_t c_tested = 0, c_member = 0;
    // kUpdLanes lanes share a point and take every kUpdLanes-th entry of its cell's list: the lanes of a point read
    // consecutive 32-byte entries (the vector L1's access rate bounds this kernel), and a list of up to kUpdLanes entries
    // is one step for all of them.  Measured per 150-frame launch: 1 lane 0.84 ms, 2 lanes 0.80, 4 lanes 0.89, 8 lanes 1.4.
    const uint32_t sub = tid % kUpdLanes;
    for (uint32_t i = tid / kUpdLanes; i < fill; i += 256 / kUpdLanes) {
        const float4 cur = pe;
        const uint32_t rgb = COLOR ? t.bin_rgb[entry(i)] : 0u;
        if (i + 256 / kUpdLanes < fill) pe = t.bin_pt[entry(i + 256 / kUpdLanes)];  // next point: in flight during this one's pairs
        const F3 p = F3{cur.x, cur.y, cur.z};
        const uint64_t info = s_info[__float_as_uint(cur.w) & (kBrickCells - 1)];
        const uint32_t cnt = (uint32_t)((info >> kDepCntShift) & kDepCntMask);
        const uint64_t off = (info & ~kPreListBit) >> kDepOffShift;
        if (sub == 0) c_tested += cnt;
        float4 n0 = make_float4(0.f, 0.f, 0.f, 0.f), n1 = n0;
        if (sub < cnt) {
            if (info & kPreListBit) {
                pre_list_entry(t, (uint32_t)off, n0, n1);
            } else {
                n0 = dep4[2 * (off + sub)];
                n1 = dep4[2 * (off + sub) + 1];
            }
        }
        for (uint32_t j = sub; j < cnt; j += kUpdLanes) {
            const float4 e0 = n0, e1 = n1;
            if (j + kUpdLanes < cnt) {  // next entry: in flight during this pair (without it the loop is latency-bound: 1.16 ms against 0.84)
                n0 = dep4[2 * (off + j + kUpdLanes)];
                n1 = dep4[2 * (off + j + kUpdLanes) + 1];
            }
            float sp, distf;
            if (!line_member(g, p, F3{e0.y, e0.z, e0.w}, F3{e1.x, e1.y, e1.z}, e1.w, sp, distf)) continue;
            c_member++;
            const PairDelta q = pair_delta(g, sp, distf);
            const uint32_t sid = __float_as_uint(e0.x);
            uint32_t h = upd_hash(sid);
            bool placed = false;
            for (int probe = 0; probe < ((t.test_table_skip & sid) ? 0 : 16); probe++) {
                const uint32_t old = atomicCAS(&keys[h], 0u, sid);
                if (old == 0u || old == sid) {
                    placed = true;
                    break;
                }
                h = (h + 1) & (kUpdSlots - 1);
            }
            if (placed) {
                unsigned long long* sv = &vals[h * W];
                atomicAdd(&sv[SW_COUNT], 1ull);
                atomicAdd(&sv[SW_S], (unsigned long long)(long long)q.s);
                atomicAdd(&sv[SW_SS], (unsigned long long)(long long)q.ss);
                atomicAdd(&sv[SW_D], (unsigned long long)(long long)q.d);
                atomicAdd(&sv[SW_DD], (unsigned long long)(long long)q.dd);
                if constexpr (COLOR) {
                    atomicAdd(&sv[SW_R], (unsigned long long)((rgb >> 16) & 255u));
                    atomicAdd(&sv[SW_G], (unsigned long long)((rgb >> 8) & 255u));
                    atomicAdd(&sv[SW_B], (unsigned long long)(rgb & 255u));
                }
            } else {  // table full: straight to HBM
                unsigned long long* v = &t.stats[(uint64_t)sid * kStatWords];
                atomicAdd(&v[SW_COUNT], 1ull);
                atomicAdd(&v[SW_S], (unsigned long long)(long long)q.s);
                atomicAdd(&v[SW_SS], (unsigned long long)(long long)q.ss);
                atomicAdd(&v[SW_D], (unsigned long long)(long long)q.d);
                atomicAdd(&v[SW_DD], (unsigned long long)(long long)q.dd);
                if constexpr (COLOR) {
                    atomicAdd(&v[SW_R], (unsigned long long)((rgb >> 16) & 255u));
                    atomicAdd(&v[SW_G], (unsigned long long)((rgb >> 8) & 255u));
                    atomicAdd(&v[SW_B], (unsigned long long)(rgb & 255u));
                }
            }
        }
    }
    __syncthreads();
    {  // flush: 8 lanes per record, 32 records per pass
        const uint32_t w = tid & 7u;
        for (uint32_t sl = tid >> 3; sl < (uint32_t)kUpdSlots; sl += 32) {
            const uint32_t key = keys[sl];
            if (key != 0u && w < (uint32_t)W) atomicAdd(&t.stats[(uint64_t)key * kStatWords + w], vals[sl * W + w]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c_tested += __shfl_down(c_tested, o);
        c_member += __shfl_down(c_member, o);
    }
    if ((tid & 63u) == 0) {
        if (c_tested) atomicAdd(&blk_ctr[0], c_tested);
        if (c_member) atomicAdd(&blk_ctr[1], c_member);
    }
    __syncthreads();
    // striped like k_replay's counter: words 2 and 3 of the 64 log_ctr lines, summed by the host
    if (tid < 2 && blk_ctr[tid])
        atomicAdd(&t.log_ctr[(blockIdx.x & (kLogRegions - 1)) * 16 + 2 + tid], (unsigned long long)blk_ctr[tid]);
}

// ------------------------------------------------------------------------------------------------
// K2, cell-sorted form.  The per-point form above reads a 32-byte dependant entry from global memory and does five LDS atomics
// for EVERY (point, dependant) pair.  Here the brick's parked points are counting-sorted by cell into LDS (kUpd2Cap at a time),
// and a work item is (cell, dependant entry, run of up to kUpd2Chunk of the cell's points): the entry is read once per item, the
// points come from LDS (lanes of one cell read the same address), the contributions are summed in registers (int32: one is below
// 2^27, stats.hpp) and the item ends with ONE hash insert + five LDS atomics.  Same LDS record table and flush as above; the
// sums are integers, so the result is bit-identical whatever the order.
//
// Thread t owns cell t of the brick for the whole launch (its dependant count and list offset stay in registers).  A round:
//   1. histogram of the round's points by cell with returning LDS atomics (= rank of the point inside its cell)      | barrier
//   2. owner threads: exclusive scans over the cells (first sorted position, first work item) -- wave scan             | barrier
//   3. owner threads: per-cell record (list offset, first position, points) and one 32-bit DESCRIPTOR per work item
//      (cell, chunk, entry) written into LDS in item order                                                             | barrier
//   4. points scattered into LDS in cell order; the first item's dependant entry is already in flight                  | barrier
//   5. items: descriptor -> cell record -> entry (global, read one item ahead) -> pair loop over the run -> table insert
// An item finds its work with two dependent LDS reads (round 2: a 9-step binary search over the item prefix sums, i.e. nine
// dependent LDS reads per item, ~1000 cycles of latency in front of every entry read).  Items beyond the descriptor array
// (kUpd2Desc per round) and entries past 32766 keep the search.
#ifndef HFPF_UPD2_CHUNK
#define HFPF_UPD2_CHUNK 8  // points of a cell one work item takes
#endif
constexpr int kUpd2Chunk = HFPF_UPD2_CHUNK;
static_assert(kUpd2Chunk >= 1 && kUpd2Chunk <= 15, "k_update_cells: int32 item sums hold 15 contributions");
constexpr uint32_t kUpd2NoDesc = ~0u;
// The kernel is a chain of latencies per brick (dependent loads, four barriers a round), so what decides its speed is how many
// bricks a CU works on at once and how many rounds a brick takes, i.e. how its LDS is spent -- the record table (44 bytes a slot),
// the sorted points (12 bytes each).  Two shapes are instantiated and the host picks per launch (hfpf.hip pick_update_shape):
//   kUpdDense  512 threads, 2048 points a round, 352-slot table: 52 KB, three workgroups (24 waves, 80 VGPRs) per CU.  Bricks that
//              update ~100 records each: the 640x480 @ 1 mm bench.  Measured on one box, per 150-frame launch: 1024-point rounds
//              at four workgroups 587 us, 1536 at three 602 us, 2048 at three 537 us (a 320-slot table with 1024 descriptors: 552).
//   kUpdWide   512 threads, 1536 points, 512 slots: 53 KB, three workgroups.  Taken for the rest of the session once the small
//              table has overflowed more than rarely (the kernel counts the items that found no slot, the host sees the count at
//              its counter read-backs): 0.5 mm voxels put 200-300 records on a brick, and an item without a slot costs five
//              scattered memory-side atomics (2048 x 1536 @ 0.5 mm: 1.34 ms per launch; 1.48 ms with 1024-point rounds, 1.71 ms
//              with 2048-point rounds at two workgroups, 2.35 ms with the dense table).
// Measured and dropped: 256 threads with 512-point rounds for bricks with few points (1.9 ms on that workload: the barriers cost
// less, the lanes per brick are missed more).  The table takes any size (the hash is range-reduced with a multiply, not masked).
struct UpdShape {
    int threads, cap, slots, desc, waves;
};
#ifndef HFPF_UPD_DENSE_SHAPE
#define HFPF_UPD_DENSE_SHAPE 512, 2048, 352, 1280, 6
#endif
#ifndef HFPF_UPD_WIDE_SHAPE
#define HFPF_UPD_WIDE_SHAPE 512, 1536, 512, 1024, 6
#endif
constexpr UpdShape kUpdDense{HFPF_UPD_DENSE_SHAPE}, kUpdWide{HFPF_UPD_WIDE_SHAPE};
// With colour the sorted points carry 4 more bytes and a table slot 24 more: 1024-point rounds keep three workgroups on a CU.
constexpr UpdShape kUpdDenseColor{512, 1024, 352, 1024, 6}, kUpdWideColor{512, 1024, 512, 1024, 4};

// REPLAY = true is the buffer replay of a clean pass (grid.hpp:418-440) for bricks whose buffered points form ONE contiguous run of
// the point log (Tables::run_*): the same kernel with the run as its input instead of the bin -- the cell of a logged point is
// recomputed from its coordinates, exactly as k_integrate indexed it -- and with every cell's dependant list cut down to the
// registrants of the running pass (the note k_depinc_fill left in the cell's scratch word, cleared here).  Coalesced reads of the
// run instead of one dependent 16-byte chain hop per point.
template <bool COLOR, int THREADS, int CAP, int SLOTS, int DESC, int WAVES, bool REPLAY = false>
__global__ __launch_bounds__(THREADS, WAVES) void k_update_cells(const GridParams g, const Tables t, const uint32_t n_bricks)
{
    static_assert(THREADS == kBrickCells, "k_update_cells: thread t owns cell t");
    static_assert(CAP % THREADS == 0 && CAP <= 4095 && (CAP + kUpd2Chunk - 1) / kUpd2Chunk <= 256, "k_update_cells: cell record holds 12-bit positions, descriptor 8-bit chunks");
    constexpr int kUpd2Threads = THREADS, kUpd2Cap = CAP, kUpd2Slots = SLOTS, kUpd2Desc = DESC;
    auto upd2_hash = [](uint32_t sid) -> uint32_t { return __umulhi(sid * 2654435761u, (uint32_t)SLOTS); };
    constexpr int W = COLOR ? 8 : kStatUsed;
    constexpr uint32_t T = kUpd2Threads, CPT = 1, PER = kUpd2Cap / T, CH = kUpd2Chunk;
    __shared__ float s_px[kUpd2Cap], s_py[kUpd2Cap], s_pz[kUpd2Cap];  // sorted points, one array per coordinate (12 bytes a point)
    __shared__ uint32_t s_rgb[COLOR ? kUpd2Cap : 1];
    __shared__ uint32_t s_cnt[kBrickCells];
    // per cell and round: first entry of the dependant list (40 bits: an index into ONE entry space that holds dep[] and, for a cell whose
    // "list" is its pre-dependant, the records' own lines -- Tables::ent_base) | first sorted position (12) | points (12)
    __shared__ uint64_t s_pack[kBrickCells];
    __shared__ uint32_t s_items[kBrickCells + 1];  // first work item of each cell (only the search path and the total read it)
    __shared__ uint32_t s_desc[kUpd2Desc];         // per work item: cell (9) | chunk (8) | entry (15)
    __shared__ uint32_t s_wsum[2][T / 64];
    __shared__ uint32_t keys[kUpd2Slots];
    __shared__ unsigned long long vals[kUpd2Slots * W];
    __shared__ unsigned int blk_ctr[3];
    const uint32_t b = blockIdx.x + 1;
    if (b > n_bricks) return;
    if (REPLAY && t.run_cnt[b] != 1u) return;  // block-uniform: several runs or stray entries -- the chain walk replays this brick
    const uint32_t fill_a = REPLAY ? t.run_len[b] : min(t.bin_fill[2 * b], t.bin_capb[2 * b]);
    const uint32_t fill_b = REPLAY ? 0u : min(t.bin_fill[2 * b + 1], t.bin_capb[2 * b + 1]);
    const uint32_t fill = fill_a + fill_b;
    if (fill == 0) return;  // block-uniform
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t first_a = REPLAY ? t.run_start[b] : t.bin_off[2 * b], first_b = REPLAY ? 0u : t.bin_off[2 * b + 1];
    if (REPLAY && first_a + fill_a > t.max_log + 1) {  // block-uniform; a run record that leaves the log (cannot happen: k_buffer records a run only when it fits)
        if (threadIdx.x == 0) atomicOr(&t.ctr[C_ERR], (unsigned long long)E_CHAIN);
        return;
    }
    auto entry = [&](uint32_t i) -> uint64_t { return i < fill_a ? first_a + i : first_b + (i - fill_a); };
    const bool scanner = tid < (uint32_t)kBrickCells / CPT;  // wave-uniform: the threads that own cells
    uint32_t own_cnt[CPT], own_off[CPT], own_pre = 0;
    bool any_note = false;
#pragma unroll
    for (uint32_t k = 0; k < CPT; k++) {
        const uint64_t cslot = (uint64_t)b * kBrickCells + tid * CPT + k;
        const uint64_t info = scanner ? t.info[cslot] : 0ull;
        const uint32_t pd = (!REPLAY && scanner) ? t.pre_dep[cslot] : 0u;  // (read beside the info word, not behind it: one round trip)
        own_cnt[k] = (uint32_t)((info >> kDepCntShift) & kDepCntMask);
        own_off[k] = (uint32_t)(info >> kDepOffShift);  // dep[] stays below 2^32 entries (host-checked)
        // no list: a cell occupied in this epoch may carry a pre-dependant (a list of one: pre_list_entry)
        if (!REPLAY && own_cnt[k] == 0 && pd) own_cnt[k] = 1, own_off[k] = pd, own_pre |= 1u << k;
        if (REPLAY) {  // only the registrants of the running pass: the entries behind the old list length
            const uint32_t note = scanner ? t.dep_tmp[cslot] : 0u;
            const bool noted = (note & kTouchedMark) != 0;
            const uint32_t old_len = noted ? min(note & kDepOldMax, own_cnt[k]) : own_cnt[k];
            own_off[k] += old_len;
            own_cnt[k] -= old_len;
            if (noted) t.dep_tmp[cslot] = 0;
            any_note = any_note || noted;
        }
    }
    if (REPLAY && !__syncthreads_or(any_note ? 1 : 0)) return;  // block-uniform: no cell of this brick gained a registrant
    for (uint32_t i = tid; i < (uint32_t)kBrickCells; i += T) s_cnt[i] = 0;
    for (uint32_t i = tid; i < (uint32_t)kUpd2Slots; i += T) keys[i] = 0;
    for (uint32_t i = tid; i < (uint32_t)(kUpd2Slots * W); i += T) vals[i] = 0;
    if (tid < 3) blk_ctr[tid] = 0;
    const float4* __restrict__ ent4 = reinterpret_cast<const float4*>(t.ent_base);  // dep[] and nv_line as one array of 32-byte entries
    uint32_t c_tested = 0, c_member = 0, c_miss = 0;
    // Software pipeline: the points of round r+1 are read from the bin while round r's items are worked (without it the streaming
    // replay, whose bricks take several rounds, is a third slower), and an item's dependant entry is read one item ahead (the first
    // one of a round ahead of the scatter).
    float4 pt[PER];
    uint32_t col[PER];
    auto load_round = [&](uint32_t r0) {
#pragma unroll
        for (uint32_t k = 0; k < PER; k++) {
            const uint32_t i = r0 + tid + k * T;
            col[k] = 0;
            pt[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < fill) {
                if (REPLAY) {
                    pt[k] = t.log_pt[entry(i)];
                    if (COLOR) col[k] = t.log_rgb[entry(i)];
                    int32_t ix, iy, iz;  // the cell the point was buffered under (grid.hpp:630-637 on the same f32 point)
                    voxel_coords(g, F3{pt[k].x, pt[k].y, pt[k].z}, ix, iy, iz);
                    pt[k].w = __uint_as_float(local_index(ix, iy, iz));
                } else {
                    pt[k] = t.bin_pt[entry(i)];
                    if (COLOR) col[k] = t.bin_rgb[entry(i)];
                }
            }
        }
    };
    struct Item {
        uint32_t first, p_lo, p_hi;
        float4 e0, e1;
    };
    auto locate = [&](uint32_t item, Item& it) {  // work item -> (cell, entry, run of points) + the entry's two 16-byte halves
        uint32_t d = kUpd2NoDesc;
        if (item < (uint32_t)kUpd2Desc) d = s_desc[item];
        uint32_t c, j, ch;
        if (d != kUpd2NoDesc) {
            c = d & (kBrickCells - 1);
            ch = (d >> 9) & 255u;
            j = d >> 17;
        } else {  // no descriptor: search the item prefix sums (s_items[lo] <= item < s_items[hi])
            uint32_t lo = 0, hi = kBrickCells;
#pragma unroll 1
            for (int st = 0; st < 9; st++) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_items[mid] <= item) lo = mid;
                else hi = mid;
            }
            c = lo;
            const uint32_t local = item - s_items[lo];
            const uint32_t chunks = ((uint32_t)((s_pack[lo] >> 52) & 0xFFFu) + CH - 1) / CH;
            j = local / chunks;
            ch = local - j * chunks;
        }
        const uint64_t pk = s_pack[c];
        const uint32_t n_c = (uint32_t)((pk >> 52) & 0xFFFu);
        it.first = (uint32_t)((pk >> 40) & 0xFFFu);
        const uint64_t e = (pk & ((1ull << 40) - 1ull)) + j;
        it.e0 = ent4[2 * e];
        it.e1 = ent4[2 * e + 1];
        it.p_lo = ch * CH;
        it.p_hi = min(n_c, it.p_lo + CH);
    };
    load_round(0);  // in flight while the tables above are cleared
    __syncthreads();
    for (uint32_t r0 = 0; r0 < fill; r0 += (uint32_t)kUpd2Cap) {  // block-uniform trip count
        const uint32_t n_round = min((uint32_t)kUpd2Cap, fill - r0);

        // 1. rank within the cell from the histogram's returning atomic
        uint32_t rk[PER];
#pragma unroll
        for (uint32_t k = 0; k < PER; k++) {
            rk[k] = 0;
            if (tid + k * T < n_round) rk[k] = atomicAdd(&s_cnt[__float_as_uint(pt[k].w) & (kBrickCells - 1)], 1u);
        }
        __syncthreads();
        // 2. exclusive scans over the cells: sorted position of the cell's first point, index of its first work item
        uint32_t n[CPT], it[CPT], sum_n = 0, sum_it = 0, inc_n = 0, inc_it = 0;
        {
#pragma unroll
            for (uint32_t k = 0; k < CPT; k++) {
                const uint32_t c = tid * CPT + k;
                n[k] = s_cnt[c];
                s_cnt[c] = 0;  // for the next round's histogram (three barriers away)
                it[k] = n[k] ? own_cnt[k] * ((n[k] + CH - 1) / CH) : 0u;
                sum_n += n[k];
                sum_it += it[k];
            }
            inc_n = wave_inclusive_scan(sum_n);
            inc_it = wave_inclusive_scan(sum_it);
            if (lane == 63) s_wsum[0][wave] = inc_n, s_wsum[1][wave] = inc_it;
        }
        __syncthreads();
        // 3. cell records and item descriptors
        {
            uint32_t pre_n = inc_n - sum_n, pre_it = inc_it - sum_it;
            for (uint32_t w2 = 0; w2 < wave; w2++) pre_n += s_wsum[0][w2], pre_it += s_wsum[1][w2];
#pragma unroll
            for (uint32_t k = 0; k < CPT; k++) {
                const uint32_t c = tid * CPT + k;
                s_pack[c] = ((((own_pre >> k) & 1u) ? t.ent_nv_first : t.ent_dep_first) + own_off[k]) | ((uint64_t)pre_n << 40) | ((uint64_t)n[k] << 52);
                s_items[c] = pre_it;
                if (it[k]) {
                    const uint32_t chunks = (n[k] + CH - 1) / CH;
                    uint32_t idx = pre_it;
                    for (uint32_t j = 0; j < own_cnt[k] && idx < (uint32_t)kUpd2Desc; j++)
                        for (uint32_t ch = 0; ch < chunks && idx < (uint32_t)kUpd2Desc; ch++, idx++)
                            s_desc[idx] = j < 32767u ? (c | (ch << 9) | (j << 17)) : kUpd2NoDesc;
                }
                pre_n += n[k];
                pre_it += it[k];
            }
            if (tid == (uint32_t)kBrickCells / CPT - 1) s_items[kBrickCells] = pre_it;
        }
        __syncthreads();
        const uint32_t total = s_items[kBrickCells];
        Item nxt;
        nxt.first = nxt.p_lo = nxt.p_hi = 0;
        nxt.e0 = nxt.e1 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid < total) locate(tid, nxt);  // entry read in flight during the scatter
        // 4. scatter into cell order
#pragma unroll
        for (uint32_t k = 0; k < PER; k++)
            if (tid + k * T < n_round) {
                const uint32_t pos = (uint32_t)((s_pack[__float_as_uint(pt[k].w) & (kBrickCells - 1)] >> 40) & 0xFFFu) + rk[k];
                s_px[pos] = pt[k].x;
                s_py[pos] = pt[k].y;
                s_pz[pos] = pt[k].z;
                if (COLOR) s_rgb[pos] = col[k];
            }
        __syncthreads();
        if (r0 + (uint32_t)kUpd2Cap < fill) load_round(r0 + (uint32_t)kUpd2Cap);  // in flight during the items
        // 5. items.  No barrier behind them: the next round's histogram only touches s_cnt, and its first barrier keeps every
        // writer of s_pack / s_desc / the sorted points behind the last reader of this round.
        for (uint32_t item = tid; item < total; item += T) {
            const Item cur = nxt;
            if (item + T < total) locate(item + T, nxt);
            const F3 la = F3{cur.e0.y, cur.e0.z, cur.e0.w}, lab = F3{cur.e1.x, cur.e1.y, cur.e1.z};
            const LineDiv dv = line_div_of(cur.e1.w);
            int32_t a_n = 0, a_s = 0, a_ss = 0, a_d = 0, a_dd = 0, a_r = 0, a_g = 0, a_b = 0;
            F3 qn = F3{0.f, 0.f, 0.f};  // the next point of the run is read while this one is tested
            if (cur.p_lo < cur.p_hi) qn = F3{s_px[cur.first + cur.p_lo], s_py[cur.first + cur.p_lo], s_pz[cur.first + cur.p_lo]};
            for (uint32_t pi = cur.p_lo; pi < cur.p_hi; pi++) {
                const F3 q3 = qn;
                if (pi + 1 < cur.p_hi) qn = F3{s_px[cur.first + pi + 1], s_py[cur.first + pi + 1], s_pz[cur.first + pi + 1]};
                float sp, distf;
                if (!line_member_hoisted(g, q3, la, lab, dv, sp, distf)) continue;
                const PairDelta q = pair_delta(g, sp, distf);
                a_n++;
                a_s += q.s;
                a_ss += q.ss;
                a_d += q.d;
                a_dd += q.dd;
                if constexpr (COLOR) {
                    const uint32_t rgb = s_rgb[cur.first + pi];
                    a_r += (int32_t)((rgb >> 16) & 255u);
                    a_g += (int32_t)((rgb >> 8) & 255u);
                    a_b += (int32_t)(rgb & 255u);
                }
            }
            c_tested += cur.p_hi - cur.p_lo;
            c_member += (uint32_t)a_n;
            if (a_n == 0) continue;
            const uint32_t sid = __float_as_uint(cur.e0.x);
            uint32_t h = upd2_hash(sid);
            bool placed = false;
            for (int probe = 0; probe < ((t.test_table_skip & sid) ? 0 : 16); probe++) {
                const uint32_t old = atomicCAS(&keys[h], 0u, sid);
                if (old == 0u || old == sid) {
                    placed = true;
                    break;
                }
                h = h + 1 == (uint32_t)kUpd2Slots ? 0u : h + 1;
            }
            c_miss += placed ? 0u : 1u;  // the host widens the table when this stops being rare
            unsigned long long* sv = placed ? &vals[h * W] : nullptr;
            unsigned long long* gv = &t.stats[(uint64_t)sid * kStatWords];  // table full: straight to HBM
#define HFPF_UPD2_ADD(word, val)                                                \
    if (placed) atomicAdd(&sv[word], (unsigned long long)(long long)(val));     \
    else atomicAdd(&gv[word], (unsigned long long)(long long)(val))
            HFPF_UPD2_ADD(SW_COUNT, a_n);
            HFPF_UPD2_ADD(SW_S, a_s);
            HFPF_UPD2_ADD(SW_SS, a_ss);
            HFPF_UPD2_ADD(SW_D, a_d);
            HFPF_UPD2_ADD(SW_DD, a_dd);
            if constexpr (COLOR) {
                HFPF_UPD2_ADD(SW_R, a_r);
                HFPF_UPD2_ADD(SW_G, a_g);
                HFPF_UPD2_ADD(SW_B, a_b);
            }
#undef HFPF_UPD2_ADD
        }
    }
    __syncthreads();
    {  // flush: 8 lanes per record
        const uint32_t w = tid & 7u;
        for (uint32_t sl = tid >> 3; sl < (uint32_t)kUpd2Slots; sl += T / 8) {
            const uint32_t key = keys[sl];
            if (key != 0u && w < (uint32_t)W) atomicAdd(&t.stats[(uint64_t)key * kStatWords + w], vals[sl * W + w]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c_tested += __shfl_down(c_tested, o);
        c_member += __shfl_down(c_member, o);
        c_miss += __shfl_down(c_miss, o);
    }
    if (lane == 0) {
        if (c_tested) atomicAdd(&blk_ctr[0], c_tested);
        if (c_member) atomicAdd(&blk_ctr[1], c_member);
        if (c_miss) atomicAdd(&blk_ctr[2], c_miss);
    }
    __syncthreads();
    if (REPLAY) {  // members found at replay time are counted apart (word 1 of the striped lines, like k_replay)
        if (tid == 1 && blk_ctr[1]) atomicAdd(&t.log_ctr[(blockIdx.x & (kLogRegions - 1)) * 16 + 1], (unsigned long long)blk_ctr[1]);
    } else if (tid < 2 && blk_ctr[tid]) {
        atomicAdd(&t.log_ctr[(blockIdx.x & (kLogRegions - 1)) * 16 + 2 + tid], (unsigned long long)blk_ctr[tid]);
    }
    if (tid == 2 && blk_ctr[2]) atomicAdd(&t.ctr[C_TABLE_MISS], (unsigned long long)blk_ctr[2]);  // rare by construction
    if (tid == 3 && fill > (uint32_t)kUpd2Cap) atomicAdd(&t.ctr[C_UPD_ROUNDS], (unsigned long long)((fill - 1u) / (uint32_t)kUpd2Cap));  // (few bricks)
}

// ------------------------------------------------------------------------------------------------
// K2b: the brick's parked points whose cell has no normal yet (its second bin region) are appended to the point log as ONE
// run (one reservation per brick and launch) and chained into their cells' four chains.  A long run (the first epoch:
// everything is buffered) chains with LDS exchanges, the chain heads travelling as one coalesced 8 KB read and write per
// brick; a short run (steady state: a few edge cells) exchanges straight on the heads in global memory.  Replaces one
// returning device atomic per buffered point in a separate pass over the log (k_link_log's atomicExch, ~1.2 ms for the
// first epoch's 39 M entries) and keeps a cell's entries of one launch within a few KB of each other for the replay's
// chain walks.
constexpr uint32_t kChains = kLogChains;  // interleaved chains per cell: k_replay walks them with 4 lanes in parallel
constexpr uint32_t kBufLdsMin = 256;  // runs at least this long chain in LDS
template <bool COLOR>
__global__ __launch_bounds__(256) void k_buffer(const GridParams g, const Tables t, const uint32_t n_bricks)
{
    __shared__ uint32_t s_head[kBrickCells * kChains];  // chain heads of the brick's cells
    __shared__ uint32_t s_minfid[kBrickCells];          // smallest frame id that buffered into the cell in this launch
    __shared__ unsigned long long s_base;
    const uint32_t b = blockIdx.x + 1;
    if (b > n_bricks) return;
    const uint32_t n_buf = min(t.bin_fill[2 * b + 1], t.bin_capb[2 * b + 1]);
    if (n_buf == 0) return;  // block-uniform
    const uint32_t tid = threadIdx.x;
    const uint64_t first = t.bin_off[2 * b + 1];
    const uint32_t region = b & (kLogRegions - 1);
    const bool in_lds = n_buf >= kBufLdsMin;  // block-uniform
    if (tid == 0) {
        s_base = atomicAdd(&t.log_ctr[region * 16], (unsigned long long)n_buf);
        const bool fits = s_base + n_buf <= t.log_region_cap;
        t.run_start[b] = (uint32_t)((uint64_t)region * t.log_region_cap + s_base + 1);
        t.run_len[b] = n_buf;
        t.run_cnt[b] += fits ? 1u : 0x100u;  // (one workgroup per brick and launch: no other writer)
    }
    if (in_lds) {
        for (uint32_t i = tid; i < (uint32_t)(kBrickCells * kChains); i += 256) s_head[i] = t.buf_head[(uint64_t)b * kBrickCells * kChains + i];
        for (uint32_t i = tid; i < (uint32_t)kBrickCells; i += 256) s_minfid[i] = kNoFrame;
    }
    __syncthreads();
    const unsigned long long base = s_base;
    const uint64_t log_base = (uint64_t)region * t.log_region_cap;
    bool overflow = false;
    for (uint32_t i = tid; i < n_buf; i += 256) {
        const unsigned long long k = base + i;
        if (k >= t.log_region_cap) {
            overflow = true;
            continue;
        }
        const float4 pe = t.bin_pt[first + i];
        const uint32_t e = (uint32_t)(log_base + k + 1);
        const uint32_t w = __float_as_uint(pe.w), lcell = w & (kBrickCells - 1), fid = w >> 9;
        uint32_t prev;  // entry e joins chain e mod 4 of its cell
        if (in_lds) {
            prev = atomicExch(&s_head[lcell * kChains + (e & (kChains - 1))], e);
            atomicMin(&s_minfid[lcell], fid);
        } else {
            const uint64_t slot = (uint64_t)b * kBrickCells + lcell;
            prev = atomicExch(&t.buf_head[slot * kChains + (e & (kChains - 1))], e);
            if (fid < t.first_frame[slot]) atomicMin(&t.first_frame[slot], fid);  // viewpoint latch, grid.hpp:229,238
        }
        t.log_pt[e] = make_float4(pe.x, pe.y, pe.z, __uint_as_float(prev));
        if (COLOR) t.log_rgb[e] = t.bin_rgb[first + i];
    }
    if (overflow) atomicOr(&t.ctr[C_ERR], (unsigned long long)E_LOG);
    if (!in_lds) return;
    __syncthreads();
    for (uint32_t i = tid; i < (uint32_t)(kBrickCells * kChains); i += 256) t.buf_head[(uint64_t)b * kBrickCells * kChains + i] = s_head[i];
    for (uint32_t i = tid; i < (uint32_t)kBrickCells; i += 256) {  // viewpoint latch: smallest frame id that touched the cell
        const uint32_t mf = s_minfid[i];
        if (mf != kNoFrame) {
            uint32_t* ff = &t.first_frame[(uint64_t)b * kBrickCells + i];
            if (mf < *ff) atomicMin(ff, mf);
        }
    }
}

// Plan the bin regions of the next launch from the demand of the previous one: cap = demand * scale * slack + 64 (slack 2: a brick's
// share of a launch moves with the poses of its frames -- 15-frame launches of the 0.5 mm workload left 1 % of their points without
// room at 1.25, 0.5 % at 2), where the
// demand is the BRICK's (both regions): a clean pass between two launches moves cells from "no normal" to "normal", so either
// region must be able to take all of the brick's points.  n_regions = 2 * (bricks + 1); regions 0 and 1 belong to the null
// brick and stay empty.
// Regions [n_regions, n_planned) belong to brick ids the host has not seen yet: ids are handed out in order, so the next bricks a
// launch discovers find a region of `spare_cap` entries waiting (without one all their points go through the overflow list and
// take the direct forms).
// Two launches: k_bin_plan writes the capacities and one sum per workgroup of kBinPlanTile regions; k_bin_place turns them into
// region offsets (the sums in front of its tile + a scan inside the tile), switches off what does not fit the pool and restarts
// the demand counters.  (Until round 4: plan, a two-launch library scan, clamp -- four dependent launches of ~5 us in front of
// every integrate call.)
constexpr uint32_t kBinPlanTile = 1024;  // regions per workgroup: 256 threads x 4 consecutive regions
__device__ __forceinline__ uint32_t block_sum_256(uint32_t v, uint32_t* s_w)  // sum over a 256-thread workgroup (convergent; s_w: 4 words)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    const uint32_t r = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    return r;
}
__global__ __launch_bounds__(256) void k_bin_plan(const Tables t, const uint32_t n_regions, const uint32_t n_planned, const uint32_t spare_cap, const float scale,
                                                  const float slack, uint32_t* __restrict__ tile_sums)
{
    __shared__ uint32_t s_w[4];
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t r = blockIdx.x * kBinPlanTile + threadIdx.x * 4u + k;
        if (r >= n_planned) continue;
        uint32_t cap = 0;
        if (r >= n_regions) {
            cap = spare_cap;
        } else if (r >= 2) {
            const uint32_t demand = t.bin_fill[r & ~1u] + t.bin_fill[r | 1u];
            if (demand) cap = (uint32_t)fminf((float)demand * scale * slack, 2.0e9f) + 64u;  // (saturated: a float above 2^32 does not convert)
        }
        t.bin_capb[r] = cap;
        sum += cap;
    }
    sum = block_sum_256(sum, s_w);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = sum;
}

// Offsets, clamp, restart.  Regions that do not fit the pool are switched off, and the demand counters of ALL regions restart --
// also those of bricks the host has not heard of yet (claimed since its last counter read-back: they have no region until then and
// keep recording their demand): left alone, their counters would add up over every launch until the next clean pass and the plan
// made from them would be inflated by that factor.  With every counter holding ONE launch's demand the planned capacities add up
// to at most 2 x slack x points + 128 x bricks < the pool size (hfpf.hip bin_pool_entries), so the 32-bit sums cannot wrap.
__global__ __launch_bounds__(256) void k_bin_place(const Tables t, const uint32_t n_planned, const uint32_t all_regions, const uint64_t pool,
                                                   const uint32_t* __restrict__ tile_sums)
{
    __shared__ uint32_t s_w[4];
    const uint32_t r0 = blockIdx.x * kBinPlanTile + threadIdx.x * 4u;
    if (blockIdx.x * kBinPlanTile < n_planned) {  // block-uniform
        uint32_t before = 0;
        for (uint32_t b = threadIdx.x; b < blockIdx.x; b += 256u) before += tile_sums[b];
        before = block_sum_256(before, s_w);
        uint32_t cap[4], mine = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            cap[k] = r0 + k < n_planned ? t.bin_capb[r0 + k] : 0u;
            mine += cap[k];
        }
        const uint32_t incl = wave_inclusive_scan(mine);
        if ((threadIdx.x & 63u) == 63u) s_w[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint32_t off = before + incl - mine;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) off += s_w[w];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t r = r0 + k;
            if (r < n_planned) {
                t.bin_off[r] = off;
                if ((uint64_t)off + cap[k] > pool) t.bin_capb[r] = 0;
                off += cap[k];
            }
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t r = r0 + k;
        if (r >= all_regions) continue;
        if (r >= n_planned) t.bin_capb[r] = 0;  // (an earlier launch may have planned more spare regions than this one)
        t.bin_fill[r] = 0;
        if (r == 0) t.ctr[C_OVF] = 0;  // the overflow list of the previous launch has been worked off (k_integrate_overflow)
    }
}

// ------------------------------------------------------------------------------------------------
// Link the log entries appended since the last clean into their cells' chains.  grid.y = log region;
// [first[r], last[r]] are 1-based global entry indices (empty when first > last).
struct LinkRanges {
    uint32_t first[kLogRegions];
    uint32_t last[kLogRegions];
};
__global__ __launch_bounds__(256) void k_link_log(const Tables t, const LinkRanges lr)
{
    const uint32_t r = blockIdx.y;
    const uint64_t e = (uint64_t)lr.first[r] + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e > lr.last[r]) return;
    uint32_t* w = reinterpret_cast<uint32_t*>(&t.log_pt[e]) + 3;
    const uint32_t v = *w;
    if (!(v & kLogUnlinked)) return;  // appended and chained by k_buffer
    const uint32_t slot = v & ~kLogUnlinked;
    *w = atomicExch(&t.buf_head[(uint64_t)slot * kChains + (e & (kChains - 1))], (uint32_t)e);  // entry e joins chain e mod 4 of its cell
}

// 125-bit occupancy stencil around (x,y,z): bit d = ((dx+2)*5 + (dy+2))*5 + (dz+2), the setK table order
// (grid.hpp:138-149); only cells with validCoord (grid.hpp:337) can be set.
// The window [c-2, c+2] spans at most two bricks per axis.  All directory entries (<= 8) are read first, then all plane
// masks (<= 20 u64), each batch independent loads, and the 5-bit z-runs are cut out with shifts: two memory round trips
// per call instead of one per (plane, brick), no data-dependent branches.
__device__ inline void neighbourhood(const GridParams& g, const Tables& t, int32_t x, int32_t y, int32_t z, uint64_t& lo, uint64_t& hi)
{
    lo = 0;
    hi = 0;
    const int32_t bx0 = (x - 2) >> 3, by0 = (y - 2) >> 3, bz0 = (z - 2) >> 3;  // arithmetic shifts: -1 below the grid
    const bool two_x = ((x + 2) >> 3) != bx0, two_y = ((y + 2) >> 3) != by0, two_z = ((z + 2) >> 3) != bz0;
    uint32_t bid[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int i = q >> 2, j = (q >> 1) & 1, k = q & 1;
        const int32_t bx = bx0 + i, by = by0 + j, bz = bz0 + k;
        const bool need = (i == 0 || two_x) && (j == 0 || two_y) && (k == 0 || two_z) && bx >= 0 && by >= 0 && bz >= 0 && bx < g.bdim[0] &&
                          by < g.bdim[1] && bz < g.bdim[2];
        uint32_t v = 0;
        if (need) v = t.dir[((uint32_t)bx * (uint32_t)g.bdim[1] + (uint32_t)by) * (uint32_t)g.bdim[2] + (uint32_t)bz];
        bid[q] = v == kLock ? 0u : v;
    }
    // plane masks of the 5 x-planes in the (up to) 2 x 2 bricks of the y/z window
    uint64_t pm[5][4];
#pragma unroll
    for (int a = 0; a < 5; a++) {
        const int32_t xx = x + a - 2;
        const bool vx = xx >= 0 && xx < g.dim[0];
        const bool hi_x = (xx >> 3) != bx0;
#pragma unroll
        for (int jk = 0; jk < 4; jk++) {
            const uint32_t b = hi_x ? bid[4 + jk] : bid[jk];
            uint64_t m = 0;
            if (vx && b) m = t.occ_mask[(uint64_t)b * 8 + ((uint32_t)xx & 7u)];
            pm[a][jk] = m;
        }
    }
    // z clipping: which of the 5 dz positions are valid cells
    uint32_t zclip = 0;
#pragma unroll
    for (int c = 0; c < 5; c++)
        if (z + c - 2 >= 0 && z + c - 2 < g.dim[2]) zclip |= 1u << c;
    const uint32_t zsh = (uint32_t)((z - 2) - bz0 * 8);  // 0..7: first z of the window inside the 16-wide line of the two z-bricks
#pragma unroll
    for (int a = 0; a < 5; a++) {
#pragma unroll
        for (int dy = 0; dy < 5; dy++) {
            const int32_t yy = y + dy - 2;
            const bool vy = yy >= 0 && yy < g.dim[1];
            const bool hi_y = (yy >> 3) != by0;
            const uint32_t sh = ((uint32_t)yy & 7u) * 8u;
            const uint64_t m0 = hi_y ? pm[a][2] : pm[a][0], m1 = hi_y ? pm[a][3] : pm[a][1];
            const uint32_t line = (uint32_t)((m0 >> sh) & 0xFFull) | ((uint32_t)((m1 >> sh) & 0xFFull) << 8);
            uint64_t f = vy ? (uint64_t)((line >> zsh) & 31u & zclip) : 0ull;
            const int d0 = (a * 5 + dy) * 5;
            if (d0 < 64) {
                lo |= f << d0;
                if (d0 + 5 > 64) hi |= f >> (64 - d0);
            } else {
                hi |= f << (d0 - 64);
            }
        }
    }
}

// K3: every occupied cell without a normal is a candidate (the reference's unprocessed_data_ set is
// a superset whose extra members fail the same gate, grid.hpp:315,352).
template <int TILES>
__global__ __launch_bounds__(256) void k_gate(const GridParams g, const Tables t, const uint32_t* __restrict__ cells_a, const uint64_t n_a,
                                              const uint32_t* __restrict__ cells_b, const uint64_t n_b, uint32_t* __restrict__ pend_out)
{
    // Input = the cells that failed the gate last time (cells_a) followed by the cells occupied since (cells_b), one launch.
    // TILES tiles per workgroup, one reservation per output list (hot list counters: see k_register).  The host uses
    // TILES = 4 only for large inputs: the stencil probe is latency-heavy and a small grid needs every workgroup it can get.
    const uint64_t n_cells = n_a + n_b;
    uint64_t key_[TILES];
    uint32_t slot_[TILES];
    uint32_t n_pass[TILES], n_pend[TILES];
#pragma unroll
    for (int tt = 0; tt < TILES; tt++) {
        const uint64_t j = ((uint64_t)blockIdx.x * TILES + tt) * 256u + threadIdx.x;
        key_[tt] = 0;
        slot_[tt] = 0;
        n_pass[tt] = n_pend[tt] = 0;
        if (j < n_cells) {
            const uint32_t slot = j < n_a ? cells_a[j] : cells_b[j - n_a];
            slot_[tt] = slot;
            if (!(t.info[slot] & kNormal)) {
                int32_t x, y, z;
                slot_coords(g, t, slot, x, y, z);
                uint64_t lo, hi;
                neighbourhood(g, t, x, y, z, lo, hi);
                const int total = __popcll(lo) + __popcll(hi);
                if (total > g.gate) n_pass[tt] = 1;
                else n_pend[tt] = 1;  // still without a normal: look at it again next pass (its neighbourhood may fill up)
                key_[tt] = HFPF_MORTON_IDS ? morton_key(x, y, z) : make_key(g, x, y, z);  // the order the pass numbers its records in
            }
        }
    }
    __shared__ TileReserveScratch<TILES> trs;
    unsigned long long ci[TILES], pi[TILES];
    block_reserve_tiles<TILES>(&t.ctr[C_CAND], n_pass, ci, trs);
    block_reserve_tiles<TILES>(&t.ctr[C_PEND], n_pend, pi, trs);
#pragma unroll
    for (int tt = 0; tt < TILES; tt++) {
        if (n_pass[tt]) t.cand_key[ci[tt]] = key_[tt];  // capacity = max_occ >= cells examined
        if (n_pend[tt]) pend_out[pi[tt]] = slot_[tt];
    }
}

// Candidates of the running pass as the kernels after the gate see them: the device counter, clamped to the room left in the
// normal records (the host learns the exact number at its next read-back; E_NORMALS reports the clamp).
__device__ __forceinline__ uint64_t cand_count(const Tables& t, uint64_t base)
{
    const uint64_t n = t.ctr[C_CAND];
    const uint64_t room = t.max_normals > base ? t.max_normals - base : 0;
    return n < room ? n : room;
}
// Head of a clean pass: all-ones sentinels behind the candidate keys the gate is about to write (they sort to the end), the pass's
// list counters back to zero, and (k_materialize_new in the comments: this part, clean_file) the cells occupied since the
// previous pass -- the new tail of occ_list, imported ones included -- that carry a pre-dependant get it filed as their list: entry,
// info word, flag bit, and a place in prereg_list (what a compacting rebuild re-creates the entry from); one reservation per list
// and workgroup.  lists_only: a compacting rebuild follows in this pass and writes every entry and info word itself.  No room in
// dep[] is E_DEP, which the host answers by compacting.  n_in >= n_new (the gate's input contains the new cells).
// One launch (k_clean_begin) when the pass runs alone.  A pass whose front half runs beside the update kernel of the integrate call
// before it (hfpf.hip clean_locked) takes the two parts apart: k_clean_front with the front half, k_clean_file at the head of the
// back half -- the update reads the info word and pre_dep of exactly the cells the filing rewrites, and nothing between the two
// launches (k_gate, the sort, k_normal, k_register) reads a filed entry, the list bits of an info word or the flag.
__device__ __forceinline__ void clean_front(const Tables& t, const uint64_t i, const uint64_t n_in)
{
    if (i < n_in) t.cand_key[i] = ~0ull;
    if (i == 0) {
        t.ctr[C_CAND] = 0;
        t.ctr[C_PEND] = 0;
        t.ctr[C_TOUCHED] = 0;
    }
    if (i < (uint64_t)kLogRegions) t.log_ctr[i * 16 + 4] = 0;  // touched cells in single-run bricks (k_depinc_offsets)
}
__device__ __forceinline__ void clean_file(const Tables& t, const uint64_t i, const uint32_t* __restrict__ new_cells, const uint64_t n_new, const uint32_t lists_only)
{
    if ((uint64_t)blockIdx.x * blockDim.x >= n_new) return;  // block-uniform
    uint32_t slot = 0, nid = 0;
    if (i < n_new) {
        slot = new_cells[i];
        nid = t.pre_dep[slot];
    }
    __shared__ BlockReserveScratch brs;
    const unsigned long long li = block_reserve(&t.ctr[C_PREREG], nid != 0, brs);
    const unsigned long long off = lists_only ? 0ull : block_reserve(&t.ctr[C_DEP], nid != 0, brs);
    if (!nid) return;
    if (li < t.max_reg) t.prereg_list[li] = slot;
    else atomicOr(&t.ctr[C_ERR], (unsigned long long)E_REG);
    set_dep_flag(t, slot);
    if (lists_only) return;
    if (off >= t.max_dep) {
        atomicOr(&t.ctr[C_ERR], (unsigned long long)E_DEP);
        return;
    }
    t.dep[off] = make_dep_entry(t, nid);
    t.info[slot] = (t.info[slot] & 3ull) | (1ull << kDepCntShift) | ((uint64_t)off << kDepOffShift);
}
__global__ __launch_bounds__(256) void k_clean_begin(const Tables t, const uint64_t n_in, const uint32_t* __restrict__ new_cells, const uint64_t n_new,
                                                     const uint32_t lists_only)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    clean_front(t, i, n_in);
    clean_file(t, i, new_cells, n_new, lists_only);
}
__global__ __launch_bounds__(256) void k_clean_front(const Tables t, const uint64_t n_in)
{
    clean_front(t, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, n_in);
}
__global__ __launch_bounds__(256) void k_clean_file(const Tables t, const uint32_t* __restrict__ new_cells, const uint64_t n_new)
{
    clean_file(t, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, new_cells, n_new, 0u);
}

// K4: one thread per candidate, in ascending order of the sorted keys (Z-order codes with HFPF_MORTON_IDS); record id = base + rank + 1.
__global__ __launch_bounds__(128) void k_normal(const GridParams g, const Tables t, const uint64_t* __restrict__ sorted_keys,
                                                const uint64_t n_cand_arg, const uint64_t base)
{
    // n_cand_arg = kCountOnDevice: the grid covers an upper bound (the gate's input size), the sorted keys behind the real
    // candidates are all-ones sentinels
    const uint64_t n_cand = n_cand_arg == kCountOnDevice ? cand_count(t, base) : n_cand_arg;
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r == 0 && n_cand_arg == kCountOnDevice) {  // publish the new record count (nothing in this pass reads it on the device)
        if (t.ctr[C_CAND] > n_cand) atomicOr(&t.ctr[C_ERR], (unsigned long long)E_NORMALS);
        t.ctr[C_NORMALS] = base + n_cand;
    }
    if (r >= n_cand) return;
    int32_t x, y, z;
    uint64_t key = sorted_keys[r];
    if (HFPF_MORTON_IDS) {
        morton_coords(key, x, y, z);
        key = make_key(g, x, y, z);  // what the record keeps: the canonical (x, y, z) key (extract order, registration contests)
    } else {
        key_coords(g, key, x, y, z);
    }
    const uint32_t slot = slot_lookup(g, t, x, y, z);
    uint64_t lo, hi;
    neighbourhood(g, t, x, y, z, lo, hi);
    // the cell centre is separable: 5 values per axis (grid.hpp:131-135 evaluated once each) instead of 125 x 3
    float cxs[5], cys[5], czs[5];
#pragma unroll
    for (int a = 0; a < 5; a++) {
        const F3 c = voxel_center(g, x + a - 2, y + a - 2, z + a - 2);
        cxs[a] = c.x;
        cys[a] = c.y;
        czs[a] = c.z;
    }
    Moments m;
    m.clear();
    int total = 0;
#pragma unroll
    for (int a = 0; a < 5; a++)
#pragma unroll
        for (int bq = 0; bq < 5; bq++) {
            const int d0 = (a * 5 + bq) * 5;
            const uint32_t bits5 = (uint32_t)((d0 < 64 ? (lo >> d0) | (d0 + 5 > 64 ? hi << (64 - d0) : 0ull) : hi >> (d0 - 64)) & 31ull);
#pragma unroll
            for (int c = 0; c < 5; c++)
                if ((bits5 >> c) & 1u) {
                    m.add(F3{cxs[a], cys[bq], czs[c]}, g.cov_shifted != 0);  // grid.hpp:364-369, setK order (x outer, z inner)
                    total++;
                }
        }
    // grid.hpp:301: getNormal leaves the normal alone when fewer than 3 cells are valid and occupied (a gate below 2 lets such a
    // candidate through), and the oracle settles "alone" as zero; the moments of one or two points would give 0/0 instead
    F3 normal = {0.f, 0.f, 0.f};
    const F3 centre = voxel_center(g, x, y, z);  // grid.hpp:391
    if (total >= 3) {
        normal = m.normal(total);
        const uint32_t ff = t.first_frame[slot];
        F3 vp = {0.f, 0.f, 0.f};
        if (ff != kNoFrame && ff < t.max_frames) vp = F3{t.frame_vp[3 * (uint64_t)ff], t.frame_vp[3 * (uint64_t)ff + 1], t.frame_vp[3 * (uint64_t)ff + 2]};
        normal = orient_normal(normal, vp, centre);
    }
    const uint64_t nid = base + r + 1;
    t.nv_key[nid] = key;
    t.nv_slot[nid] = slot;
    t.nv_c[3 * nid + 0] = centre.x;
    t.nv_c[3 * nid + 1] = centre.y;
    t.nv_c[3 * nid + 2] = centre.z;
    t.nv_n[3 * nid + 0] = normal.x;
    t.nv_n[3 * nid + 1] = normal.y;
    t.nv_n[3 * nid + 2] = normal.z;
    {  // the per-voxel half of the cylinder test (grid.hpp:40-49), evaluated once here and copied into dependant entries
        F3 a, ab;
        float dd;
        line_of(g, centre, normal, a, ab, dd);
        t.nv_line[2 * nid] = make_float4(__uint_as_float((uint32_t)nid), a.x, a.y, a.z);  // = DepEntry{sid, a, ab, |ab|^2}
        t.nv_line[2 * nid + 1] = make_float4(ab.x, ab.y, ab.z, dd);
    }
    t.stat_id[slot] = (uint32_t)nid;
    atomicOr(reinterpret_cast<unsigned int*>(&t.info[slot]), 2u);  // normal_found, grid.hpp:398
    atomicOr(reinterpret_cast<unsigned long long*>(&t.nd_mask[((uint64_t)(slot >> 9) * 8u + ((uint32_t)x & 7u)) * 2]),
             1ull << ((((uint32_t)y & 7u) << 3) | ((uint32_t)z & 7u)));
}

// K5: one thread per (new normal, line step).  Occupancy is frozen during a clean pass, so the steps are
// independent; "last registrant wins" on unoccupied cells (grid.hpp:443-449) is an atomicMax over record ids -- they ascend from
// pass to pass -- with the contests inside a pass settled by the canonical (x, y, z) key (see below: ids follow the Z-order there).
template <int kRegTiles>
__global__ __launch_bounds__(256) void k_register(const GridParams g, const Tables t, const uint64_t n_cand_arg, const uint64_t base, const uint32_t count_deps)
{
    // count_deps: the incremental dependant-table update follows (no compacting rebuild was decided): a registration on an occupied
    // cell is counted into the cell's scratch word right here, and the first one of a cell files the cell in touched_list -- what a
    // separate pass over reg_occ (k_depinc_count) did until round 4, one launch and one re-read of the list earlier.
    const uint64_t n_cand = n_cand_arg == kCountOnDevice ? cand_count(t, base) : n_cand_arg;  // the same in every thread
    if (n_cand == 0) return;
    // Step-major mapping: a wave holds 64 key-adjacent voxels at the SAME step, so its targets sit in the same few bricks.
    // A workgroup takes kRegTiles consecutive 256-voxel tiles of one step and reserves its list entries once: same-address device
    // atomics retire one per ~12 ns whoever issues them.  The host takes 8 tiles for passes of millions of candidates (6.7 K
    // reservations in the bench's first pass; 27 K would be a third of a millisecond) and 2 for the small steady ones, where the
    // ~20 K candidates of a pass would otherwise sit on 70 of the 256 CUs.
    const uint32_t steps = 2u * (uint32_t)g.K + 1u;
    const uint64_t tile_items = 256ull * kRegTiles;
    const uint64_t per_step = ((n_cand + tile_items - 1) / tile_items) * tile_items;  // whole workgroups per step keep them uniform in i
    const uint64_t blk_first = (uint64_t)blockIdx.x * tile_items;
    const uint32_t step_idx = (uint32_t)(blk_first / per_step);
    const int i = (int)step_idx - g.K;
    uint32_t slot_[kRegTiles], nid_[kRegTiles];
    uint32_t f_occ = 0, f_fresh = 0;
#pragma unroll
    for (int tt = 0; tt < kRegTiles; tt++) {
        const uint64_t r = blk_first % per_step + (uint64_t)tt * 256u + threadIdx.x;
        bool want = r < n_cand && step_idx < steps;
        uint64_t nid = 0;
        int32_t xx = 0, yy = 0, zz = 0;
        if (want) {
            nid = base + r + 1;
            const F3 c = F3{t.nv_c[3 * nid], t.nv_c[3 * nid + 1], t.nv_c[3 * nid + 2]};
            const F3 n = F3{t.nv_n[3 * nid], t.nv_n[3 * nid + 1], t.nv_n[3 * nid + 2]};
            const F3 nb = line_step(g, c, n, i);  // grid.hpp:405
            want = valid_point(g, nb);            // grid.hpp:406
            voxel_coords(g, nb, xx, yy, zz);      // grid.hpp:409
            want = want && xx != INT_MIN && yy != INT_MIN && zz != INT_MIN && valid_coord(g, xx, yy, zz);  // grid.hpp:410
        }
        const uint32_t bidx = want ? brick_index(g, xx, yy, zz) : 0u;
        const uint32_t b = brick_acquire_wave(t, bidx, want);
        want = want && b != 0;
        const uint32_t slot = b * kBrickCells + local_index(xx, yy, zz);
        uint64_t o_plane, o_bit;
        slot_plane_bit(slot, o_plane, o_bit);
        const bool occ = want && (t.occ_mask[o_plane] & o_bit);
        slot_[tt] = slot;
        nid_[tt] = (uint32_t)nid;
        if (occ) {
            f_occ |= 1u << tt;
            if (count_deps && atomicAdd(&t.dep_tmp[slot], 1u) == 0u) f_fresh |= 1u << tt;  // (scratch words are zero between passes)
        }
        if (want && !occ) {
            // An unoccupied target keeps ONE dependant, in pre_dep[slot] and nowhere else until the cell is occupied (k_materialize_new).
            const uint32_t old = atomicMax(&t.pre_dep[slot], (uint32_t)nid);
#ifdef HFPF_TEST_NO_KEY_CONTEST  // (tests only: shows that test_registration_contest_... notices a contest left to the ids)
            if (false) {
#else
            if (HFPF_MORTON_IDS && old > base && old != (uint32_t)nid) {
#endif
                // Another voxel of this pass registered here as well.  Ids follow the Z-order inside a pass, the contest is about the
                // canonical order: the registrant with the LARGEST (x, y, z) KEY stays (the reference walks its candidates in that
                // order and the last one overwrites, grid.hpp:443-449).  The atomicMax above has put the larger ID into the cell and
                // told this lane whom it met; the lane now sees to it that the cell holds a key at least as large as the better of the
                // two.  Whoever displaces a holder learns of it the same way and takes over that duty, so once every registrant is
                // through, the cell holds the largest key of the pass.  (Uncontested cells -- most -- cost the one atomic they always did.)
                const uint64_t my_key = t.nv_key[nid], old_key = t.nv_key[old];
                const uint32_t best = old_key > my_key ? old : (uint32_t)nid;
                const uint64_t best_key = old_key > my_key ? old_key : my_key;
                uint32_t cur = max(old, (uint32_t)nid);  // what the atomicMax left behind
                for (int spin = 0; spin < kMaxSpin; ++spin) {
                    if (cur == best || t.nv_key[cur] >= best_key) break;  // (every value the cell takes in this pass is an id of this pass)
                    const uint32_t seen = atomicCAS(&t.pre_dep[slot], cur, best);
                    if (seen == cur) break;
                    cur = seen;
                }
            }
        }
    }
    __shared__ TileReserveScratch<kRegTiles> trs;
    uint32_t n_occ[kRegTiles];
    unsigned long long ri[kRegTiles];
#pragma unroll
    for (int tt = 0; tt < kRegTiles; tt++) n_occ[tt] = (f_occ >> tt) & 1u;
    block_reserve_tiles<kRegTiles>(&t.ctr[C_REG], n_occ, ri, trs);
    bool overflow = false;
#pragma unroll
    for (int tt = 0; tt < kRegTiles; tt++) {
        if (n_occ[tt]) {
            if (ri[tt] < t.max_reg) t.reg_occ[ri[tt]] = make_uint2(slot_[tt], nid_[tt]);  // dependants.push_back, grid.hpp:417
            else overflow = true;
        }
    }
    if (overflow) atomicOr(&t.ctr[C_ERR], (unsigned long long)E_REG);
    if (count_deps) {  // (wave-uniform) the cells this workgroup was the first to count a registration for
#pragma unroll
        for (int tt = 0; tt < kRegTiles; tt++) n_occ[tt] = (f_fresh >> tt) & 1u;
        block_reserve_tiles<kRegTiles>(&t.ctr[C_TOUCHED], n_occ, ri, trs);  // capacity max_touched = max_reg >= the registrations of any pass
#pragma unroll
        for (int tt = 0; tt < kRegTiles; tt++)
            if (n_occ[tt]) t.touched_list[ri[tt]] = slot_[tt];
    }
}

// K5b: buffer replay (grid.hpp:418-440), cell-centric.  The reference replays a cell's buffer once per voxel that
// registers on it; here one thread walks the chain of a touched cell ONCE and tests every buffered point against all
// of the cell's registrants of this pass (dependant entries with record id > base), four at a time in registers.
// Random 16-byte chain reads are the cost (sector amplification makes them HBM-bound), so reading each entry once
// instead of once per registrant is the lever.  Runs after the dependant table has been updated.
template <bool COLOR>
__global__ __launch_bounds__(256) void k_replay(const GridParams g, const Tables t, const uint32_t* __restrict__ cells, const uint32_t use_marks,
                                                const uint32_t skip_single, const uint64_t n_touched_arg, const uint64_t base)
{
    // use_marks: the incremental update left kTouchedMark | old list length in the cell's scratch word.  It appends, so the
    // registrants of this pass are the entries behind that position and the walk over the older ones -- one dependent 32-byte read
    // each -- is skipped; the note is cleared here.  Without marks (compacting rebuild: any order) every entry is looked at and
    // filtered by record id.  skip_single: cells of single-run bricks are left (with their note) to the streaming replay.
    __shared__ unsigned long long queue[4][kQueueRows * kQueueStride];
    unsigned long long* q = queue[threadIdx.x >> 6];
    const uint64_t n_touched = n_touched_arg == kCountOnDevice ? (uint64_t)t.ctr[C_TOUCHED] : n_touched_arg;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t j = gid / kChains;           // cell
    const uint32_t sub = (uint32_t)(gid % kChains);  // which of the cell's interleaved chains this lane walks
    uint32_t slot = 0, cnt = 0, head = 0;
    uint64_t off = 0;
    bool mine = j < n_touched;
    if (mine) {
        slot = cells[j];  // touched cells in slot (brick-major) order: adjacent lanes walk chains that share cache lines
        if (skip_single && t.run_cnt[slot >> 9] == 1u) mine = false;  // (with its note) left to the streaming replay
    }
    if (mine) {
        const uint64_t info = t.info[slot];
        cnt = (uint32_t)((info >> kDepCntShift) & kDepCntMask);
        off = info >> kDepOffShift;
        head = t.buf_head[(uint64_t)slot * kChains + sub];
    }
    {  // a cell none of whose chains holds a point (an unoccupied cell that gained its single dependant) has nothing to replay
        uint32_t any = head;
#pragma unroll
        for (uint32_t o = 1; o < kChains; o <<= 1) any |= (uint32_t)__shfl_xor((int)any, (int)o);
        if (any == 0u) cnt = 0;
    }
    uint32_t replayed = 0;
    uint32_t next = 0;  // next dependant entry to look at
    if (use_marks && mine) {
        const uint32_t m = t.dep_tmp[slot];  // the lanes of a cell read it in the same instruction, then lane 0 clears it
        if (m & kTouchedMark) {
            next = min(m & kDepOldMax, cnt);
            if (sub == 0) t.dep_tmp[slot] = 0;
        }
    }
    // wave-uniform outer loop: every lane keeps calling the flush helper until all lanes are done
    while (__ballot(next < cnt) != 0) {
        constexpr int B = HFPF_REPLAY_B;
        uint32_t sid[B];
        F3 la[B], lab[B];
        float ldd[B];
        LineDiv ldv[B];
        bool use[B];
        const float4* __restrict__ dep4 = reinterpret_cast<const float4*>(t.dep);
        float4 e0[B], e1[B];
#pragma unroll
        for (int k = 0; k < B; k++) {  // the next B entries, B independent reads in flight together
            e0[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            e1[k] = make_float4(0.f, 0.f, 1.f, 1.f);
            if (next + (uint32_t)k < cnt) {
                e0[k] = dep4[2 * (off + next + k)];
                e1[k] = dep4[2 * (off + next + k) + 1];
            }
        }
        bool any = false;
#pragma unroll
        for (int k = 0; k < B; k++) {
            sid[k] = __float_as_uint(e0[k].x);
            use[k] = next + (uint32_t)k < cnt && sid[k] > base;  // a registrant of this pass
            any = any || use[k];
            la[k] = F3{e0[k].y, e0[k].z, e0[k].w};
            lab[k] = F3{e1[k].x, e1[k].y, e1[k].z};
            ldd[k] = e1[k].w;
        }
        next = min(cnt, next + (uint32_t)B);
        StatDeltaT<COLOR> d[B];
#pragma unroll
        for (int k = 0; k < B; k++) {
            stat_delta_zero(d[k]);
            ldv[k] = line_div_of(ldd[k]);  // the divisor's share of the division, once per registrant (geometry.hpp)
        }
        if (any) {
            uint32_t e = head;
            // (Every link is a head that k_buffer / direct_buffer exchanged, i.e. the index of an entry they wrote.  A range check per
            // hop was measured in round 4: +12 % on this kernel, whose time is the chain of dependent reads; left out.)
            while (e) {
                const float4 p = t.log_pt[e];
                const uint32_t rgb = COLOR ? t.log_rgb[e] : 0u;
                const F3 pt = F3{p.x, p.y, p.z};
#pragma unroll
                for (int k = 0; k < B; k++) {
                    if (use[k]) {
                        float sp, distf;
                        if (line_member_hoisted(g, pt, la[k], lab[k], ldv[k], sp, distf)) stat_delta_add(d[k], pair_delta(g, sp, distf), rgb);
                    }
                }
                e = __float_as_uint(p.w);  // one 16-byte read per hop: the link travels with the point
            }
        }
#pragma unroll
        for (int k = 0; k < B; k++) {
            // sum the sub-chains of the cell (kChains adjacent lanes) before the flush: one record update per (cell, registrant)
#pragma unroll
            for (int w = 0; w < kStatUsed; w++) {
                long long v = d[k].v[w];
#pragma unroll
                for (uint32_t o = 1; o < kChains; o <<= 1) v += __shfl_xor(v, (int)o);
                d[k].v[w] = v;
            }
            if constexpr (COLOR) {
#pragma unroll
                for (int w = 0; w < 3; w++) {
                    long long v = d[k].rgb[w];
#pragma unroll
                    for (uint32_t o = 1; o < kChains; o <<= 1) v += __shfl_xor(v, (int)o);
                    d[k].rgb[w] = v;
                }
            }
            const bool member = sub == 0 && d[k].v[SW_COUNT] != 0;
            if (member) replayed += (uint32_t)d[k].v[SW_COUNT];
            wave_flush_members(t, q, member, d[k], sid[k]);
        }
    }
    // Diagnostic count of replayed members: reduced per workgroup and striped over the 64 counter lines of log_ctr (word 1 of
    // each line; the host sums them in read_counters).  One counter bumped once per wave would be ~1e5 same-address atomics
    // at ~12 ns each in the first pass -- most of this kernel's time.
    __shared__ unsigned int s_rep;
    if (threadIdx.x == 0) s_rep = 0;
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) replayed += __shfl_down(replayed, o);
    if ((threadIdx.x & 63u) == 0 && replayed) atomicAdd(&s_rep, replayed);
    __syncthreads();
    if (threadIdx.x == 0 && s_rep) atomicAdd(&t.log_ctr[(blockIdx.x & (kLogRegions - 1)) * 16 + 1], (unsigned long long)s_rep);
}

// K5c: the same replay, registration-centric: fed from what k_register left (reg_occ[reg_first .. C_REG): one (cell, new record)
// pair each) instead of the updated lists, so it needs neither info, dep[] nor the note in dep_tmp and can run before the
// dependant-table update -- beside the update kernel of the integrate call before the pass (hfpf.hip clean_locked).  kChains
// adjacent lanes take one registration: the record's line comes from nv_line (the two halves of its dependant entry), lane `sub`
// walks chain `sub` of the cell.  A cell that gains several registrants in a pass is walked once per registrant here (k_replay:
// once per three); the sums are integer atomics into records no list names yet, so neither the order nor the update kernel matters.
template <bool COLOR>
__global__ __launch_bounds__(256) void k_replay_reg(const GridParams g, const Tables t, const uint64_t reg_first, const uint64_t n_reg_arg)
{
    __shared__ unsigned long long queue[4][kQueueRows * kQueueStride];
    __shared__ unsigned int s_rep;
    const uint64_t n_reg = n_reg_arg == kCountOnDevice ? min((uint64_t)t.ctr[C_REG], t.max_reg) : n_reg_arg;
    if (reg_first + (uint64_t)blockIdx.x * (256u / kChains) >= n_reg) return;  // block-uniform: the grid is sized from an upper bound
    unsigned long long* q = queue[threadIdx.x >> 6];
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t j = reg_first + gid / kChains;    // registration
    const uint32_t sub = (uint32_t)(gid % kChains);  // which of the cell's interleaved chains this lane walks
    uint32_t nid = 0, head = 0;
    if (j < n_reg) {
        const uint2 r = t.reg_occ[j];  // (cell, record): neighbouring registrations are key-adjacent voxels at the same line step
        nid = r.y;
        head = t.buf_head[(uint64_t)r.x * kChains + sub];
    }
    uint32_t any = head;  // a cell none of whose chains holds a point costs no more than this
#pragma unroll
    for (uint32_t o = 1; o < kChains; o <<= 1) any |= (uint32_t)__shfl_xor((int)any, (int)o);
    StatDeltaT<COLOR> d;
    stat_delta_zero(d);
    if (any) {
        float4 e0, e1;
        pre_list_entry(t, nid, e0, e1);
        const F3 la = F3{e0.y, e0.z, e0.w}, lab = F3{e1.x, e1.y, e1.z};
        const LineDiv ldv = line_div_of(e1.w);
        uint32_t e = head;
        while (e) {  // (links: see k_replay)
            const float4 p = t.log_pt[e];
            const uint32_t rgb = COLOR ? t.log_rgb[e] : 0u;
            float sp, distf;
            if (line_member_hoisted(g, F3{p.x, p.y, p.z}, la, lab, ldv, sp, distf)) stat_delta_add(d, pair_delta(g, sp, distf), rgb);
            e = __float_as_uint(p.w);
        }
    }
    // sum the sub-chains of the cell (kChains adjacent lanes) before the flush: one record update per registration
#pragma unroll
    for (int w = 0; w < kStatUsed; w++) {
        long long v = d.v[w];
#pragma unroll
        for (uint32_t o = 1; o < kChains; o <<= 1) v += __shfl_xor(v, (int)o);
        d.v[w] = v;
    }
    if constexpr (COLOR) {
#pragma unroll
        for (int w = 0; w < 3; w++) {
            long long v = d.rgb[w];
#pragma unroll
            for (uint32_t o = 1; o < kChains; o <<= 1) v += __shfl_xor(v, (int)o);
            d.rgb[w] = v;
        }
    }
    const bool member = sub == 0 && d.v[SW_COUNT] != 0;
    uint32_t replayed = member ? (uint32_t)d.v[SW_COUNT] : 0u;
    wave_flush_members(t, q, member, d, nid);
    // replayed members, counted as k_replay counts them (word 1 of the striped counter lines)
    if (threadIdx.x == 0) s_rep = 0;
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) replayed += __shfl_down(replayed, o);
    if ((threadIdx.x & 63u) == 0 && replayed) atomicAdd(&s_rep, replayed);
    __syncthreads();
    if (threadIdx.x == 0 && s_rep) atomicAdd(&t.log_ctr[(blockIdx.x & (kLogRegions - 1)) * 16 + 1], (unsigned long long)s_rep);
}

// ---- dependant table rebuild --------------------------------------------------------------------
__device__ __forceinline__ uint32_t reg_slot(const Tables& t, uint64_t j, uint64_t n_reg) { return j < n_reg ? t.reg_occ[j].x : t.prereg_list[j - n_reg]; }

// A cell's dependant list owns a power-of-two number of entries (1, 2, 4, ...: dep_capacity of its length).  A clean pass that
// extends the list appends IN PLACE while the new length fits and relocates it -- into a block of the next capacity -- only when it
// does not, so a list that grows by an entry or two per pass moves a logarithmic number of times instead of once per pass (on the
// 0.5 mm workload a touched cell holds ~8 entries: relocating them all every pass was most of k_depinc_offsets' 32-byte traffic).
// Every writer of info words allocates by this rule: k_depinc_offsets, the compacting rebuild (k_dep_offsets), k_clean_begin (1).
__device__ __forceinline__ uint32_t dep_capacity(uint32_t cnt) { return cnt <= 1u ? cnt : 1u << (32 - __clz((int)(cnt - 1u))); }

__global__ __launch_bounds__(256) void k_dep_count(const Tables t, const uint64_t n_reg, const uint64_t n_pre)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool fresh = false;
    uint32_t slot = 0;
    if (j < n_reg + n_pre) {
        slot = reg_slot(t, j, n_reg);
        fresh = atomicAdd(&t.dep_tmp[slot], 1u) == 0u;
    }
    __shared__ BlockReserveScratch brs;
    const unsigned long long ti = block_reserve(&t.ctr[C_TOUCHED], fresh, brs);
    if (fresh) t.touched_list[ti] = slot;  // capacity max_touched = max_reg >= distinct cells among n_reg + n_pre entries (host-checked: n_reg + n_pre <= max_reg)
}

__global__ __launch_bounds__(256) void k_dep_offsets(const Tables t, const uint64_t n_touched)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = j < n_touched;
    const uint32_t slot = act ? t.touched_list[j] : 0u;
    uint32_t cnt = act ? t.dep_tmp[slot] : 0u;
    if (cnt > kDepCntMask) {
        atomicOr(&t.ctr[C_ERR], (unsigned long long)E_DEPCNT);
        cnt = (uint32_t)kDepCntMask;
    }
    const unsigned long long off = wave_reserve_n(&t.ctr[C_DEP], dep_capacity(cnt));
    if (!act) return;
    t.info[slot] = (t.info[slot] & 3ull) | ((uint64_t)cnt << kDepCntShift) | ((uint64_t)off << kDepOffShift);
    if (cnt) set_dep_flag(t, slot);
    t.dep_tmp[slot] = 0;
}

__global__ __launch_bounds__(256) void k_dep_fill(const Tables t, const uint64_t n_reg, const uint64_t n_pre)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_reg + n_pre) return;
    const uint32_t slot = reg_slot(t, j, n_reg);
    const uint32_t nid = j < n_reg ? t.reg_occ[j].y : t.pre_dep[slot];
    const uint64_t info = t.info[slot];
    const uint32_t k = atomicAdd(&t.dep_tmp[slot], 1u);
    if (k >= ((info >> kDepCntShift) & kDepCntMask)) return;  // clamped list
    t.dep[(info >> kDepOffShift) + k] = make_dep_entry(t, nid);
}

__global__ __launch_bounds__(256) void k_dep_reset(const Tables t, const uint64_t n_touched)
{
    const uint64_t n = n_touched == kCountOnDevice ? (uint64_t)t.ctr[C_TOUCHED] : n_touched;
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) t.dep_tmp[t.touched_list[j]] = 0;
}


// ---- incremental dependant-table update ---------------------------------------------------------------
// A clean pass only appends registrations to the lists of occupied cells, so only the cells touched by THIS pass are looked at
// (k_register counts the pass's registrations per cell and files the touched cells): k_depinc_offsets extends a list in place while it
// fits the power-of-two block it owns (dep_capacity) and otherwise copies it into a fresh block at the end of dep[], k_depinc_fill
// writes the new entries.  The space of a relocated list is garbage until the next full rebuild (k_dep_count / k_dep_offsets /
// k_dep_fill), which the host runs when dep[] fills up.

__global__ __launch_bounds__(256) void k_depinc_offsets(const Tables t, const uint64_t n_touched_arg)
{
    const uint64_t n_touched = n_touched_arg == kCountOnDevice ? (uint64_t)t.ctr[C_TOUCHED] : n_touched_arg;
    uint32_t slot_[kListTiles], old_cnt_[kListTiles], new_cnt_[kListTiles], take_[kListTiles];
    uint64_t info_[kListTiles];
#pragma unroll
    for (int tt = 0; tt < kListTiles; tt++) {
        const uint64_t j = ((uint64_t)blockIdx.x * kListTiles + tt) * 256u + threadIdx.x;
        slot_[tt] = 0, old_cnt_[tt] = 0, new_cnt_[tt] = 0, take_[tt] = 0, info_[tt] = 0;
        if (j < n_touched) {
            slot_[tt] = t.touched_list[j];
            info_[tt] = t.info[slot_[tt]];
            old_cnt_[tt] = (uint32_t)((info_[tt] >> kDepCntShift) & kDepCntMask);
            new_cnt_[tt] = old_cnt_[tt] + t.dep_tmp[slot_[tt]];
            // the list stays where it is while it fits the block it owns (dep_capacity); otherwise it moves into a block of the next capacity
            if (new_cnt_[tt] > dep_capacity(old_cnt_[tt])) take_[tt] = dep_capacity(min(new_cnt_[tt], (uint32_t)kDepCntMask));
        }
    }
    __shared__ TileReserveScratch<kListTiles> trs;
    unsigned long long off_[kListTiles];
    uint32_t n_single = 0;
    block_reserve_tiles<kListTiles>(&t.ctr[C_DEP], take_, off_, trs);  // one atomic per workgroup; lists of neighbouring cells stay adjacent
#pragma unroll
    for (int tt = 0; tt < kListTiles; tt++) {
        const uint64_t j = ((uint64_t)blockIdx.x * kListTiles + tt) * 256u + threadIdx.x;
        if (j >= n_touched) continue;
        const uint32_t slot = slot_[tt], old_cnt = old_cnt_[tt], new_cnt = new_cnt_[tt];
        const uint64_t info = info_[tt], old_off = info >> kDepOffShift;
        const bool moves = take_[tt] != 0;
        const unsigned long long off = moves ? off_[tt] : old_off;
        // No room left in dep[], or an old list too long for the 15-bit note of the cursor word (kDepOldMax; the info word itself
        // counts to 65535): E_DEP, which the host answers with the compacting rebuild (k_dep_*, no such limit).  More than 65535
        // entries on one cell fit nowhere: E_DEPCNT, a capacity error.  (A cell's registrants all lie within K cells of it along
        // their normals, a few hundred voxels at most, so neither limit is reachable by a real scene.)
        if ((moves && off + take_[tt] > t.max_dep) || new_cnt > kDepCntMask || old_cnt > kDepOldMax) {
            atomicOr(&t.ctr[C_ERR], (unsigned long long)(new_cnt > kDepCntMask ? E_DEPCNT : E_DEP));
            t.dep_tmp[slot] = kDepPoison;  // k_depinc_fill skips this cell
            continue;
        }
        n_single += t.run_cnt[slot >> 9] == 1u ? 1u : 0u;
        if (moves) {
            for (uint32_t k = 0; k < old_cnt; k++) t.dep[off + k] = t.dep[old_off + k];
        }
        t.info[slot] = (info & 3ull) | ((uint64_t)new_cnt << kDepCntShift) | ((uint64_t)off << kDepOffShift);
        if (old_cnt == 0 && new_cnt) set_dep_flag(t, slot);
        t.dep_tmp[slot] = (old_cnt << 16) | old_cnt;  // old length | append cursor
    }
    // cells in single-run bricks, for the host's choice of replay form: word 4 of the striped counter lines, one atomic per workgroup
    __shared__ unsigned int s_single;
    if (threadIdx.x == 0) s_single = 0;
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_single += __shfl_down(n_single, o);
    if ((threadIdx.x & 63u) == 0 && n_single) atomicAdd(&s_single, n_single);
    __syncthreads();
    if (threadIdx.x == 0 && s_single) atomicAdd(&t.log_ctr[(blockIdx.x & (kLogRegions - 1)) * 16 + 4], (unsigned long long)s_single);
}

__global__ __launch_bounds__(256) void k_depinc_fill(const Tables t, const uint64_t reg_first, const uint64_t n_reg_arg, const uint32_t leave_note)
{
    // leave_note = 0: the replay of this pass has been fed from reg_occ (k_replay_reg) and nobody will read the note: the scratch word
    // goes straight back to zero, what it has to be between passes.
    const uint64_t n_reg = n_reg_arg == kCountOnDevice ? min((uint64_t)t.ctr[C_REG], t.max_reg) : n_reg_arg;
    const uint64_t j = reg_first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_reg) return;
    const uint2 r = t.reg_occ[j];
    const uint32_t v = atomicAdd(&t.dep_tmp[r.x], 1u);
    if (v & kDepPoison) return;
    const uint32_t k = v & 0xFFFFu;
    const uint64_t info = t.info[r.x];
    t.dep[(info >> kDepOffShift) + k] = make_dep_entry(t, r.y);
    // exactly (new length - old length) tickets are drawn per cell: whoever draws the last one turns the cursor word into the
    // note for the replay -- this cell gained registrants, they sit behind entry `old length` -- which the replay clears again
    if (k + 1 == (uint32_t)((info >> kDepCntShift) & kDepCntMask)) t.dep_tmp[r.x] = leave_note ? kTouchedMark | ((v >> 16) & kDepOldMax) : 0u;
}


// ---- K6 extract -----------------------------------------------------------------------------------
// Keys of the records that downloadData would emit: x<xdim && y<ydim && z<zdim (grid.hpp:463-465);
// others get the all-ones key and sort to the end.
// The reference's alternate extractors (grid.hpp:491-601) are this one scan with two knobs (= hfpf_extract_opts):
//   min_count           downloadHQ(cloud, threshold): `if (data->count < threshold) continue;` -- applied HERE, so filtered
//                       rows never reach the sort's front, the row kernel or the host
//   classify / paint    downloadClassified / download(XYZRGB): colour coding in k_extract_rows
struct ExtractOpts {
    double min_count;
    int32_t classify_threshold;  // < 0: off; else rows with count > threshold are painted red, the others white (grid.hpp:527-534)
    int32_t paint_white;         // 1: r = g = b = 255 as downloadHQ / downloadClassified set it (grid.hpp:527-529,558-560)
};
constexpr int kExtractTiles = 8;  // 256-record tiles per workgroup of k_extract_keys: one atomic on the row counter per workgroup
__global__ __launch_bounds__(256) void k_extract_keys(const GridParams g, const Tables t, const unsigned long long* __restrict__ stats,
                                                      const uint64_t n_normals, const ExtractOpts opt, uint64_t* __restrict__ keys,
                                                      uint32_t* __restrict__ vals)
{
    __shared__ unsigned int s_rows;
    if (threadIdx.x == 0) s_rows = 0;
    __syncthreads();
    uint32_t n_valid = 0;
#pragma unroll
    for (int tt = 0; tt < kExtractTiles; tt++) {
        const uint64_t j = ((uint64_t)blockIdx.x * kExtractTiles + tt) * 256u + threadIdx.x;
        if (j >= n_normals) continue;
        const uint64_t nid = j + 1;
        const uint64_t key = t.nv_key[nid];
        int32_t x, y, z;
        key_coords(g, key, x, y, z);
        uint32_t valid = valid_coord(g, x, y, z) ? 1u : 0u;
        if (valid && opt.min_count > 0.0) {
            const long long cnt = (long long)stats[nid * kStatWords + SW_COUNT];
            if ((double)(int)cnt < opt.min_count) valid = 0;  // int count against a double threshold, grid.hpp:561
        }
        if (t.hidden && valid) {  // (uniform: a kernel argument) a record whose cell is HIDDEN is no row (hfpf_hide_*)
            uint64_t plane, bit;
            slot_plane_bit(t.nv_slot[nid], plane, bit);
            if (t.hidden[plane] & bit) valid = 0;
        }
        keys[j] = valid ? key : ~0ull;
        vals[j] = (uint32_t)nid;
        n_valid += valid;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_valid += __shfl_down(n_valid, o);
    if ((threadIdx.x & 63u) == 0 && n_valid) atomicAdd(&s_rows, n_valid);
    __syncthreads();
    if (threadIdx.x == 0 && s_rows) atomicAdd(&t.ctr[C_ROWS], (unsigned long long)s_rows);  // (one same-address device atomic costs ~12 ns)
}

struct Row {  // = hfpf_row
    int32_t ix, iy, iz;
    uint32_t count;
    float x, y, z;
    float nx, ny, nz;
    float sdx, sdy, sdz;
    float mean_dist, sd_dist;
    uint32_t rgb;
};
static_assert(sizeof(Row) == 64, "row is 64 bytes");

// The centroid of record nid (cnt = its count, > 0; s = its statistic words) and the mean em of its line parameter: every projection
// is a - s*ab (stats.hpp), so centroid = a - E[s]*ab.  Shared by k_extract_rows and k_query, which compares distances to it.
__device__ __forceinline__ void record_centroid(const GridParams& g, const Tables& t, const long long* s, const uint64_t nid, const long long cnt,
                                                double& em, float& x, float& y, float& z)
{
    const float4 l0 = t.nv_line[2 * nid], l1 = t.nv_line[2 * nid + 1];
    const double ax = l0.y, ay = l0.z, az = l0.w, abx = l1.x, aby = l1.y, abz = l1.z;
    const double inv = 1.0 / (double)cnt;
    em = ((double)s[SW_S] / (double)g.fs_scale) * inv;  // mean of s, or of u = s - 0.5 (stats.hpp)
    const double es = HFPF_CENTERED_MOMENTS ? 0.5 + em : em;
    x = (float)(ax - es * abx);
    y = (float)(ay - es * aby);
    z = (float)(az - es * abz);
}

// The row of record nid at cell (x, y, z), before any colour coding: the per-row body of k_extract_rows, also k_query's winner row.
__device__ __forceinline__ Row record_row(const GridParams& g, const Tables& t, const unsigned long long* __restrict__ stats, const uint64_t nid,
                                          const int32_t x, const int32_t y, const int32_t z)
{
    Row r;
    r.ix = x, r.iy = y, r.iz = z;
    const long long* s = reinterpret_cast<const long long*>(&stats[nid * kStatWords]);
    const long long cnt = s[SW_COUNT];
    r.count = (uint32_t)cnt;
    r.nx = t.nv_n[3 * nid];
    r.ny = t.nv_n[3 * nid + 1];
    r.nz = t.nv_n[3 * nid + 2];
    if (cnt <= 0) {  // count==0 rows emit the zero centroid (grid.hpp:472-476)
        r.x = r.y = r.z = 0.f;
        r.sdx = r.sdy = r.sdz = 0.f;
        r.mean_dist = r.sd_dist = 0.f;
        r.rgb = 0;
    } else {
        double em;
        record_centroid(g, t, s, nid, cnt, em, r.x, r.y, r.z);
        const float4 l1 = t.nv_line[2 * nid + 1];
        const double abx = l1.x, aby = l1.y, abz = l1.z;
        const double inv = 1.0 / (double)cnt;
        // per-axis variance = ab_i^2 * var(s)
        double vs = ((double)s[SW_SS] / (double)g.fss_scale) * inv - em * em;
        const double md = ((double)s[SW_D] / (double)g.fd_scale) * inv;
        double vd = ((double)s[SW_DD] / (double)g.fdd_scale) * inv - md * md;
        if (cnt == 1) vs = vd = 0.0;  // the recurrence gives exactly 0 for a single sample
        vs = fmax(vs, 0.0);
        r.sdx = (float)(abx * abx * vs);
        r.sdy = (float)(aby * aby * vs);
        r.sdz = (float)(abz * abz * vs);
        r.mean_dist = (float)md;
        r.sd_dist = (float)fmax(vd, 0.0);
        r.rgb = 0;
        if (t.color) {  // EXTENSION: mean colour of the cylinder members, round half up
            const uint32_t cr = (uint32_t)((2 * s[SW_R] + cnt) / (2 * cnt));  // exact integer form of floor(sum/cnt + 1/2)
            const uint32_t cg = (uint32_t)((2 * s[SW_G] + cnt) / (2 * cnt));
            const uint32_t cb = (uint32_t)((2 * s[SW_B] + cnt) / (2 * cnt));
            r.rgb = (min(cr, 255u) << 16) | (min(cg, 255u) << 8) | min(cb, 255u);
        }
    }
    return r;
}

__global__ __launch_bounds__(256) void k_extract_rows(const GridParams g, const Tables t, const unsigned long long* __restrict__ stats,
                                                      const uint64_t n_rows, const ExtractOpts opt, const uint64_t* __restrict__ keys,
                                                      const uint32_t* __restrict__ vals, Row* __restrict__ rows)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_rows) return;
    int32_t x, y, z;
    key_coords(g, keys[j], x, y, z);
    Row r = record_row(g, t, stats, vals[j], x, y, z);
    if (opt.paint_white) r.rgb = 0x00FFFFFFu;
    if (opt.classify_threshold >= 0) r.rgb = (int)r.count > opt.classify_threshold ? 0x00FF0000u : 0x00FFFFFFu;
    rows[j] = r;
}


// ---- render (hfpf_render*, include/hfpf.h) ----------------------------------------------------------------------------
// The rows are the extract row set (k_extract_keys -> sort -> k_extract_rows) with min_count raised to max(1, min_count): row j is
// the j-th in lexicographic (ix, iy, iz) order, so "smallest row index" is the contract's tie rule.  A z-buffer word is
// bits(depth32) << 32 | row: depth32 > 0 (zc > z_near > 0), so the unsigned order of the words is (depth, lex) order and the
// pixel's winner is the 64-bit minimum -- independent of the order the candidates arrive in.  The buffer starts all ones.
constexpr int kRenderChunkViews = 64;                 // views per splat launch (their poses sit in LDS: 6 KB)
constexpr size_t kRenderZbufBytes = 256ull << 20;     // z-buffer scratch of one chunk (one view may exceed it alone)
constexpr unsigned long long kRenderEmpty = ~0ull;

struct RenderParams {
    Pinhole cam;
    uint32_t n_views;        // views of this chunk
    uint32_t cull;           // HFPF_RENDER_CULL_BACKFACES
    uint32_t world_normals;  // HFPF_RENDER_WORLD_NORMALS
    int32_t radius;          // >= 0 fixed, -1 auto
    int32_t max_radius;
    double r_num;            // (0.5 * res) * max(fx, fy): the auto radius is floor(r_num / zc), evaluated as the contract writes it
};

// What every kernel with a camera shares beside view.hpp.  A chunk's n poses into LDS, before the block's first return:
__device__ __forceinline__ void stage_poses(double* s_pose, const double* __restrict__ poses, const uint32_t n)
{
    for (uint32_t i = threadIdx.x; i < n * 12u; i += blockDim.x) s_pose[i] = poses[i];
    __syncthreads();
}

// Of the 64-byte row a view reads the point and the normal: one 16-byte and one 8-byte load.
struct RowPN {
    double x, y, z, nx, ny, nz;
};
__device__ __forceinline__ RowPN row_point_normal(const Row& r)
{
    const float4 q0 = *reinterpret_cast<const float4*>(&r.x);   // x, y, z, nx
    const float2 q1 = *reinterpret_cast<const float2*>(&r.ny);  // ny, nz
    return RowPN{q0.x, q0.y, q0.z, q0.w, q1.x, q1.y};
}

// One candidate into the depth buffer zv of its view: `word` (64 bits with the row behind the depth, or the depth's 32 alone) into the
// window of radius r around (pu, pv), clipped to the image.  A candidate first reads the pixel's word with a plain load and skips the
// atomic when it is already <= its own: words only ever decrease, so a stale value is >= the current one and the skip is exact.
// Under overdraw most candidates end there.  |pu|, |pv| <= 2^30 and r <= 15: the window's bounds do not wrap.
template <typename Word>
__device__ __forceinline__ void view_splat(Word* __restrict__ zv, const Pinhole& k, const int pu, const int pv, const int r, const Word word)
{
    const int x0 = max(pu - r, 0), x1 = min(pu + r, (int)k.width - 1);
    const int y0 = max(pv - r, 0), y1 = min(pv + r, (int)k.height - 1);
    for (int py = y0; py <= y1; py++)
        for (int px = x0; px <= x1; px++) {
            Word* a = zv + (uint64_t)py * k.width + (uint64_t)px;
            if (__hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > word) atomicMin(a, word);
        }
}

// One thread per row, looping over the chunk's views.  The back-face cull sits between the two halves of the projection: behind a
// one-piece projection it costs this kernel two VGPRs.
__global__ __launch_bounds__(256) void k_render_splat(const Row* __restrict__ rows, const uint32_t n_rows, const double* __restrict__ poses,
                                                      const RenderParams p, unsigned long long* __restrict__ zbuf)
{
    __shared__ double s_pose[kRenderChunkViews * 12];
    stage_poses(s_pose, poses, p.n_views);
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_rows) return;
    const RowPN q = row_point_normal(rows[j]);
    const uint64_t WH = (uint64_t)p.cam.width * p.cam.height;
    for (uint32_t v = 0; v < p.n_views; v++) {
        const double* T = &s_pose[12 * v];
        double dx, dy, dz, zc;
        int pu, pv;
        if (!view_depth(T, p.cam, p.cam.z_near, q.x, q.y, q.z, dx, dy, dz, zc)) continue;
        if (p.cull && !(((q.nx * dx + q.ny * dy) + q.nz * dz) < 0.0)) continue;
        if (!view_pixel(T, p.cam, dx, dy, dz, zc, pu, pv)) continue;
        view_splat(zbuf + v * WH, p.cam, pu, pv, view_radius(p.radius, p.max_radius, p.r_num, zc), (unsigned long long)__float_as_uint((float)zc) << 32 | j);
    }
}

// One thread per pixel of the chunk: the winner's row is fetched once and the requested planes are written (NULL planes are
// skipped).  Plane pointers are already offset to the chunk's first view.
struct RenderPlanes {
    float* depth;
    float* normal;
    uint32_t* rgb;
    uint32_t* count;
    int32_t* voxel;
};
__global__ __launch_bounds__(256) void k_render_resolve(const Row* __restrict__ rows, const unsigned long long* __restrict__ zbuf,
                                                        const double* __restrict__ poses, const RenderParams p, const RenderPlanes o)
{
    const uint64_t WH = (uint64_t)p.cam.width * p.cam.height;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= WH * p.n_views) return;
    const unsigned long long word = zbuf[i];
    const float qnan = __uint_as_float(0x7FC00000u);
    if (word == kRenderEmpty) {
        if (o.depth) o.depth[i] = qnan;
        if (o.normal) o.normal[3 * i] = o.normal[3 * i + 1] = o.normal[3 * i + 2] = qnan;
        if (o.rgb) o.rgb[i] = 0u;
        if (o.count) o.count[i] = 0u;
        if (o.voxel) o.voxel[3 * i] = o.voxel[3 * i + 1] = o.voxel[3 * i + 2] = -1;
        return;
    }
    const Row& r = rows[(uint32_t)word];
    if (o.depth) o.depth[i] = __uint_as_float((uint32_t)(word >> 32));
    if (o.normal) {
        float n0 = r.nx, n1 = r.ny, n2 = r.nz;
        if (!p.world_normals) {
            const double* T = poses + 12 * (i / WH);
            const double nx = n0, ny = n1, nz = n2;
            n0 = (float)((T[0] * nx + T[4] * ny) + T[8] * nz);
            n1 = (float)((T[1] * nx + T[5] * ny) + T[9] * nz);
            n2 = (float)((T[2] * nx + T[6] * ny) + T[10] * nz);
        }
        o.normal[3 * i] = n0;
        o.normal[3 * i + 1] = n1;
        o.normal[3 * i + 2] = n2;
    }
    if (o.rgb) o.rgb[i] = r.rgb;
    if (o.count) o.count[i] = r.count;
    if (o.voxel) {
        o.voxel[3 * i] = r.ix;
        o.voxel[3 * i + 1] = r.iy;
        o.voxel[3 * i + 2] = r.iz;
    }
}


// ---- pose tracking (hfpf_track*, include/hfpf.h) ------------------------------------------------------------------------
// Frame-to-model point-to-plane ICP with projective association: one launch per iteration sums the 6x6 normal equations of every
// sampled point at the estimate T_k, the host solves them.  The model view is a render z-buffer (k_render_splat) at the input
// pose; a word's low 32 bits name the row whose centroid and normal a point is compared with.  Every term is quantised to an
// int64 and the sums are exact, so the result does not depend on how the points are scheduled.
constexpr int kTrackTerms = 30;        // 21 J_i J_j (i <= j, i outer), 6 J_i r, r r, inliers, points used
constexpr double kTrackScaleJJ = 16777216.0;    // 2^24
constexpr double kTrackScaleJR = 268435456.0;   // 2^28
constexpr double kTrackScaleRR = 4294967296.0;  // 2^32
constexpr double kTrackHeadroom = 32.0;         // metres: max(|a.x|, |a.y|, |a.z|) at or above it rejects the point
constexpr uint32_t kTrackMaxBlocks = 2048;

struct TrackParams {
    double T[12];          // the estimate T_k, camera -> fusion frame
    double V[12];          // the view pose (the input pose T0); c = (V[3], V[7], V[11])
    Pinhole cam;           // the view
    double max_d2;         // max_distance * max_distance
    float zc_lo, zc_hi;    // the handle's z-clip as float compares (GridParams)
    uint32_t n_samples;    // sampled points
    uint32_t stride;
    uint32_t cols;         // depth: sampled columns, ceil(image width / stride)
    uint32_t n_points;     // cloud: records in the frame
};

// 64-bit form of wave_inclusive_scan: the same DPP steps on both halves, a 64-bit add between them.  Lane 63 ends with the
// wave's total (mod 2^64; the int64 sums never wrap).
template <int CTRL, int ROW_MASK, bool BOUND_ZERO>
__device__ __forceinline__ unsigned long long dpp_u64(unsigned long long x)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)x, CTRL, ROW_MASK, 0xF, BOUND_ZERO);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(x >> 32), CTRL, ROW_MASK, 0xF, BOUND_ZERO);
    return (unsigned long long)hi << 32 | lo;
}
__device__ __forceinline__ unsigned long long wave_total_u64(unsigned long long x)
{
    x += dpp_u64<0x111, 0xF, true>(x);   // row_shr:1
    x += dpp_u64<0x112, 0xF, true>(x);   // row_shr:2
    x += dpp_u64<0x114, 0xF, true>(x);   // row_shr:4
    x += dpp_u64<0x118, 0xF, true>(x);   // row_shr:8
    x += dpp_u64<0x142, 0xA, false>(x);  // row_bcast:15 into rows 1 and 3
    x += dpp_u64<0x143, 0xC, false>(x);  // row_bcast:31 into rows 2 and 3
    return x;
}

__device__ __forceinline__ unsigned long long track_q(double v, double scale) { return (unsigned long long)(long long)rint(v * scale); }

// The ICP core that k_track_reduce and k_align_reduce share.  A thread's int64 sums travel by value, in and out of icp_accumulate:
// handed over by reference, the compiler keeps a second copy of all of them across the sample loop (150 VGPRs instead of 92).
template <int N>
struct IcpSums {
    unsigned long long v[N];  // 21 J_i J_j (i <= j, i outer), 6 J_i r, r r, inliers; beyond 28 the kernel's own counts
};

// One sample: the lever a (the point minus the centre the twist is taken about), the model normal n (the caller has checked
// |n|^2 <= 2), the difference d (the point minus the model point).  A lever outside the headroom rejects the sample; otherwise
// r = n . d, J = (a x n, n), the 28 quantised terms are added to v[0..27] and v[28] counts the inlier.
template <int N>
__device__ __forceinline__ IcpSums<N> icp_accumulate(IcpSums<N> sum, double ax, double ay, double az, double nx, double ny, double nz,
                                                     double dx, double dy, double dz)
{
    static_assert(N >= 29, "icp_accumulate: 21 + 6 + 1 terms and the inlier count");
    if (!(fmax(fmax(fabs(ax), fabs(ay)), fabs(az)) < kTrackHeadroom)) return sum;
    const double r = (nx * dx + ny * dy) + nz * dz;
    const double J[6] = {ay * nz - az * ny, az * nx - ax * nz, ax * ny - ay * nx, nx, ny, nz};
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) sum.v[k++] += track_q(J[i] * J[j], kTrackScaleJJ);
#pragma unroll
    for (int i = 0; i < 6; i++) sum.v[21 + i] += track_q(J[i] * r, kTrackScaleJR);
    sum.v[27] += track_q(r * r, kTrackScaleRR);
    sum.v[28] += 1;
    return sum;
}

// The 256-thread block's totals of the sums (DPP across the wave, LDS across the four waves) into acc, which the host zeroed before
// the launch: one 64-bit atomic per non-zero term.
template <int N>
__device__ __forceinline__ void icp_block_reduce(const IcpSums<N>& sum, unsigned long long* __restrict__ acc)
{
    __shared__ unsigned long long s_part[4][N];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; k++) {
        const unsigned long long t = wave_total_u64(sum.v[k]);
        if (lane == 63) s_part[wave][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const unsigned long long t = (s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + (s_part[2][threadIdx.x] + s_part[3][threadIdx.x]);
        if (t) atomicAdd(&acc[threadIdx.x], t);
    }
}

// The two poses as the loop body reads them: from the kernarg segment (TrackParams is k_track_reduce's FIRST argument), behind an
// empty asm as kernarg_tables() does.  Taken from the by-value argument, the compiler keeps all 24 doubles in scalar registers for
// the whole loop and spills some of them.
__device__ __forceinline__ const TrackParams& track_kernarg()
{
    kernarg_ptr p = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const TrackParams*)p;
}

// One sampled point per thread, grid-stride over at most kTrackMaxBlocks blocks, in any PointForm (load_point).  Sample s is pixel
// (su * stride, sv * stride) of a depth image, record s * stride of a cloud.  Each thread keeps its 30 sums in registers
// (icp_accumulate; v[29] counts the points used); icp_block_reduce adds them to acc.
template <int FORM>
__global__ __launch_bounds__(256) void k_track_reduce(const TrackParams p, const uint8_t* __restrict__ frame, const PointLayout<FORM> lay,
                                                      const Row* __restrict__ rows, const unsigned long long* __restrict__ zbuf,
                                                      unsigned long long* __restrict__ acc)
{
    IcpSums<kTrackTerms> sum;
#pragma unroll
    for (int k = 0; k < kTrackTerms; k++) sum.v[k] = 0;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < p.n_samples; s += gridDim.x * blockDim.x) {
        uint64_t i = (uint64_t)s * p.stride;
        if constexpr (FORM == kFormDepth) {
            const uint32_t sv = s / p.cols, su = s - sv * p.cols;
            i = (sv * p.stride) * lay.width + su * p.stride;
        }
        const F3 c = load_point<FORM>(frame, lay, i);
        const float x = c.x, y = c.y, z = c.z;
        if (!(__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z) && z < p.zc_hi && z > p.zc_lo)) continue;
        sum.v[29] += 1;
        const TrackParams& P = track_kernarg();
        const double* T = P.T;
        const double* V = P.V;
        const double px = x, py = y, pz = z;
        const double wx = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
        const double wy = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
        const double wz = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
        // a = pw - c: also the offset the view's projection starts from
        double ax, ay, az, zc;
        int pu, pv;
        // (the halves one by one: behind view_project's && this kernel takes four more VGPRs and its depth form loses a wave)
        if (!view_depth(V, p.cam, p.cam.z_near, wx, wy, wz, ax, ay, az, zc)) continue;
        if (!view_pixel(V, p.cam, ax, ay, az, zc, pu, pv)) continue;
        if (!view_inside(p.cam, pu, pv)) continue;
        const unsigned long long word = zbuf[(uint64_t)pv * p.cam.width + (uint64_t)pu];
        if (word == kRenderEmpty) continue;
        const RowPN m = row_point_normal(rows[(uint32_t)word]);
        const double dx = wx - m.x, dy = wy - m.y, dz = wz - m.z;
        if (!(((dx * dx + dy * dy) + dz * dz) <= p.max_d2)) continue;
        if (!(((m.nx * m.nx + m.ny * m.ny) + m.nz * m.nz) <= 2.0)) continue;
        sum = icp_accumulate(sum, ax, ay, az, m.nx, m.ny, m.nz, dx, dy, dz);
    }
    icp_block_reduce(sum, acc);
}


// ---- point queries (hfpf_query*, include/hfpf.h) ----------------------------------------------------------------------
// One lane per point of any PointForm (load_point): transform it as integrate does, read its own cell's occupancy bit, then walk
// the rows of the (2r+1)^3 window around its voxel.  r <= 4 makes the window span at most two bricks per axis: at most 8
// directory words, and per x-plane of a touched brick one nd_mask normal_found word ANDed with the window's (y, z) mask; the set
// bits are the cells with a record, stat_id names it.  Candidates are the rows extract would emit (valid cell, count >= max(1,
// min_count): the compare of k_extract_keys) and their centroid is record_centroid's, so the distances are those of the extracted
// rows.  The winner is the smallest d2 and then the smallest (x, y, z) key, independent of the walk order.
constexpr uint32_t kQHitUsed = 1u, kQHitInBbox = 2u, kQHitOccupied = 4u, kQHitHasRow = 8u, kQHitFound = 16u;
constexpr int kQueryMaxRadius = 4;

struct __attribute__((aligned(16))) QueryHit {  // = hfpf_query_hit
    int32_t voxel[3];
    uint32_t flags;
    int32_t row_voxel[3];
    uint32_t row_count;
    float p[3];
    float distance;
    float signed_distance;
    uint32_t reserved[3];
};
static_assert(sizeof(QueryHit) == 64, "query hit is 64 bytes");

struct QueryParams {
    double T[12];        // camera -> fusion frame
    double min_count;    // max(1, min_count)
    double max_d2;       // max_distance * max_distance (+inf allowed)
    uint64_t first;      // frame index of the launch's first point (hit k = point first + k)
    uint32_t n;          // points of the launch
    int32_t radius;      // 0..kQueryMaxRadius
    uint32_t zclip;      // 1: the handle's z-clip decides USED
};

// (y, z) window mask of one x-plane: bits ly * 8 + lz for ly in [ya, yb], lz in [za, zb] (0 <= a <= b <= 7)
__device__ __forceinline__ uint64_t plane_window(int ya, int yb, int za, int zb)
{
    const uint64_t ybytes = (yb - ya == 7 ? ~0ull : (1ull << (8 * (yb - ya + 1))) - 1ull) << (8 * ya);
    const uint64_t zbits = (uint64_t)(((1u << (zb - za + 1)) - 1u) << za) * 0x0101010101010101ull;
    return ybytes & zbits;
}

// The enumeration every window walk shares (query, mesh, raycast samples, component links): the cells with a record inside the
// box [lo, hi] (0 <= lo, hi <= dim - 1 per axis, at most two bricks an axis), brick by brick through the directory, per x-plane of a
// touched brick the nd_mask normal_found word ANDed with the box's (y, z) mask, less the plane's HIDDEN word while anything is hidden
// (Tables::hidden).  visit(cx, cy, cz, nid) sees each of them once.
template <typename Visit>
__device__ __forceinline__ void window_walk(const GridParams& g, const Tables& t, const int lo[3], const int hi[3], Visit&& visit)
{
    if (!(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) return;
    for (int bx = lo[0] >> kBrickShift; bx <= hi[0] >> kBrickShift; bx++)
        for (int by = lo[1] >> kBrickShift; by <= hi[1] >> kBrickShift; by++)
            for (int bz = lo[2] >> kBrickShift; bz <= hi[2] >> kBrickShift; bz++) {
                const uint32_t b = t.dir[((uint32_t)bx * (uint32_t)g.bdim[1] + (uint32_t)by) * (uint32_t)g.bdim[2] + (uint32_t)bz];
                if (b == 0 || b == kLock) continue;  // untouched (kLock cannot happen between kernels)
                const uint64_t wmask = plane_window(max(lo[1] - 8 * by, 0), min(hi[1] - 8 * by, 7), max(lo[2] - 8 * bz, 0),
                                                    min(hi[2] - 8 * bz, 7));
                const int x1 = min(hi[0], 8 * bx + 7);
                for (int cx = max(lo[0], 8 * bx); cx <= x1; cx++) {
                    const uint64_t plane = (uint64_t)b * 8u + (uint32_t)(cx & 7);
                    uint64_t w = t.nd_mask[plane * 2] & wmask;
                    if (t.hidden) w &= ~t.hidden[plane];  // (uniform: a kernel argument) HIDDEN cells hold no row (hfpf_hide_*)
                    while (w) {
                        const int bitn = __builtin_ctzll(w);
                        w &= w - 1;
                        const int32_t cy = 8 * by + (bitn >> 3), cz = 8 * bz + (bitn & 7);
                        const uint32_t nid = t.stat_id[b * kBrickCells + local_index(cx, cy, cz)];
                        if (nid == 0) continue;
                        visit(cx, cy, cz, nid);
                    }
                }
            }
}

// The window walk of a query (and of a mesh's corner samples): the candidate rows of the (2 radius + 1)^3 cells around voxel v,
// clipped to the valid cells 0..dim-1 (extract emits no other), and the winner among those within max_d2 of q.
struct WindowNearest {
    bool found, has_row;  // has_row: v's own cell holds a candidate
    uint32_t nid;         // the winner's record (found only)
    int32_t wx, wy, wz;   // its cell, -1 without a winner
    double d2, dx, dy, dz;  // q - its centroid, f64
};
__device__ __forceinline__ WindowNearest window_nearest(const GridParams& g, const Tables& t, const F3 q, const int32_t v[3], const int radius,
                                                        const double min_count, const double max_d2)
{
    WindowNearest r;
    r.found = r.has_row = false;
    r.nid = 0;
    r.wx = r.wy = r.wz = -1;
    r.d2 = r.dx = r.dy = r.dz = 0.0;
    uint64_t best_key = 0;
    int lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = max(v[a] - radius, 0);
        hi[a] = min(v[a] + radius, g.dim[a] - 1);
    }
    window_walk(g, t, lo, hi, [&](const int32_t cx, const int32_t cy, const int32_t cz, const uint32_t nid) {
        const long long* s = reinterpret_cast<const long long*>(&t.stats[(uint64_t)nid * kStatWords]);
        const long long cnt = s[SW_COUNT];
        if ((double)(int)cnt < min_count) return;  // min_count >= 1: cnt > 0 below
        if (cx == v[0] && cy == v[1] && cz == v[2]) r.has_row = true;
        double em;
        float rx, ry, rz;
        record_centroid(g, t, s, nid, cnt, em, rx, ry, rz);
        const double dx = (double)q.x - (double)rx, dy = (double)q.y - (double)ry, dz = (double)q.z - (double)rz;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (!(d2 <= max_d2)) return;
        const uint64_t key = make_key(g, cx, cy, cz);
        if (!r.found || d2 < r.d2 || (d2 == r.d2 && key < best_key)) {
            r.found = true;
            r.d2 = d2, best_key = key, r.nid = nid;
            r.dx = dx, r.dy = dy, r.dz = dz;
            r.wx = cx, r.wy = cy, r.wz = cz;
        }
    });
    return r;
}

template <int FORM>
__global__ __launch_bounds__(256) void k_query(const GridParams g, const Tables t, const QueryParams p, const uint8_t* __restrict__ frame,
                                               const PointLayout<FORM> lay, QueryHit* __restrict__ hits, Row* __restrict__ rows)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= p.n) return;
    const F3 c = load_point<FORM>(frame, lay, p.first + k);
    const float x = c.x, y = c.y, z = c.z;
    const float qnan = __builtin_bit_cast(float, 0x7FC00000u);
    QueryHit h;
    h.voxel[0] = h.voxel[1] = h.voxel[2] = INT_MIN;
    h.flags = 0;
    h.row_voxel[0] = h.row_voxel[1] = h.row_voxel[2] = -1;
    h.row_count = 0;
    h.p[0] = h.p[1] = h.p[2] = qnan;
    h.distance = h.signed_distance = qnan;
    h.reserved[0] = h.reserved[1] = h.reserved[2] = 0;
    bool found = false;
    uint32_t best_nid = 0;
    int32_t wx = -1, wy = -1, wz = -1;
    if (__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z) && (!p.zclip || zclip_pass(g, z))) {
        const F3 q = transform_point(p.T, x, y, z);
        int32_t v[3];
        voxel_coords(g, q, v[0], v[1], v[2]);
        h.flags = kQHitUsed;
        h.voxel[0] = v[0], h.voxel[1] = v[1], h.voxel[2] = v[2];
        h.p[0] = q.x, h.p[1] = q.y, h.p[2] = q.z;
        if (valid_point(g, q)) {
            h.flags |= kQHitInBbox;
            // own cell: inside the storage extent (0..dim) for every in-bbox point; checked all the same before the table reads
            if (v[0] >= 0 && v[1] >= 0 && v[2] >= 0 && v[0] <= g.dim[0] && v[1] <= g.dim[1] && v[2] <= g.dim[2]) {
                uint64_t plane, bit;
                slot_plane_bit(slot_lookup(g, t, v[0], v[1], v[2]), plane, bit);
                if (t.occ_mask[plane] & bit) h.flags |= kQHitOccupied;
            }
            const WindowNearest wn = window_nearest(g, t, q, v, p.radius, p.min_count, p.max_d2);
            if (wn.has_row) h.flags |= kQHitHasRow;
            found = wn.found;
            best_nid = wn.nid;
            wx = wn.wx, wy = wn.wy, wz = wn.wz;
            const double best_d2 = wn.d2, bdx = wn.dx, bdy = wn.dy, bdz = wn.dz;
            if (found) {
                const double nx = t.nv_n[3 * (uint64_t)best_nid], ny = t.nv_n[3 * (uint64_t)best_nid + 1], nz = t.nv_n[3 * (uint64_t)best_nid + 2];
                h.flags |= kQHitFound;
                h.row_voxel[0] = wx, h.row_voxel[1] = wy, h.row_voxel[2] = wz;
                h.row_count = (uint32_t)t.stats[(uint64_t)best_nid * kStatWords + SW_COUNT];
                h.distance = (float)sqrt(best_d2);
                h.signed_distance = (float)((nx * bdx + ny * bdy) + nz * bdz);
            }
        }
    }
    hits[k] = h;
    if (rows) {
        Row r;
        if (found) {
            r = record_row(g, t, t.stats, best_nid, wx, wy, wz);
        } else {
            r = Row{};
            r.ix = r.iy = r.iz = -1;
        }
        rows[k] = r;
    }
}

// ---- raycast (hfpf_raycast*, include/hfpf.h) ------------------------------------------------------------------------------
// The contract is a dense march of query samples; the kernel skips every run of samples it can PROVE undefined.  A sample is
// undefined when it lies outside the box or when its (2r+1)^3 window holds no row, and r <= 4 < 8 keeps the window of a point of
// brick b inside b's 27-neighbourhood.  Three byte maps, rebuilt per call from the directory and the normal_found words, say where
// rows cannot be: map 0 holds per brick "a brick of my 27-neighbourhood has a row", maps 1 and 2 its OR over 4^3 and 16^3 bricks.
// A sample whose own voxel lies in a zero cell of a map (side S = 8, 32 or 128 cells) is undefined, and so is every sample whose
// voxel lies in that cell grown by 8 - r cells: its window still stays inside the cell dilated by one brick.  From such a sample the
// march jumps to the first sample that may leave the grown cell, computed from the ray's cells-per-sample rate, rounded down, with
// a slack (one cell plus the f32 rounding of the ray's coordinates, in cells) taken off every bound; outside the box it jumps the same way
// to the face's plane.  Every sample that is evaluated is evaluated as k_query does (voxel_coords, window_nearest), so a skipped run
// changes no byte.  One lane per ray; view rays are mapped in 8 x 8 pixel tiles per wave so that a wave's rays stay together.
constexpr uint32_t kRayUsed = 1u, kRayHit = 2u, kRayBackface = 4u, kRayNear = 8u;
constexpr int kRayLevels = 3;  // map l: cells of 4^l bricks an axis

struct __attribute__((aligned(16))) RayHit {  // = hfpf_ray_hit
    float t;
    uint32_t flags;
    float p[3];
    float n[3];
    int32_t row_voxel[3];
    uint32_t rgb, count, sample;
    uint32_t reserved[2];
};
static_assert(sizeof(RayHit) == 64, "ray hit is 64 bytes");

struct RayParams {
    double T[12];        // camera -> fusion frame (general rays; view rays read their view's pose from device memory)
    double min_count;    // max(1, min_count)
    double max_d2;       // max_distance * max_distance (+inf allowed)
    double t0, dt;       // t_k = t0 + k * dt
    double fx, fy, cx, cy;  // views
    uint64_t n_rays;     // general rays of the launch
    uint32_t n_samples;  // <= 2^20
    int32_t radius;      // 1..kQueryMaxRadius
    uint32_t cull;       // 1: a back crossing does not end the ray
    uint32_t width, row0, rows;  // views: image width, first image row and rows of the launch (hit 0 = pixel (0, row0))
    uint64_t view_stride;        // hits between consecutive views (width * height)
    int32_t mdim[kRayLevels][3];
    const uint8_t* map[kRayLevels];
};

// has[i] = 1 iff directory entry i names a brick with a normal_found bit in one of its 8 x-planes
__global__ __launch_bounds__(256) void k_ray_map_bricks(const Tables t, const uint32_t n_dir, uint8_t* __restrict__ has)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_dir) return;
    const uint32_t b = t.dir[i];
    uint64_t w = 0;
    if (b != 0 && b != kLock)
        for (uint32_t x = 0; x < 8; x++) w |= t.nd_mask[((uint64_t)b * 8u + x) * 2];
    has[i] = w != 0;
}

// out = in dilated by one cell (the brick map: 27-neighbourhood)
__global__ __launch_bounds__(256) void k_ray_map_dilate(const uint8_t* __restrict__ in, const int dx, const int dy, const int dz, uint8_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)dx * (uint32_t)dy * (uint32_t)dz) return;
    const int z = (int)(i % (uint32_t)dz), y = (int)(i / (uint32_t)dz % (uint32_t)dy), x = (int)(i / ((uint32_t)dz * (uint32_t)dy));
    uint32_t any = 0;
    for (int a = max(x - 1, 0); a <= min(x + 1, dx - 1); a++)
        for (int b = max(y - 1, 0); b <= min(y + 1, dy - 1); b++)
            for (int c = max(z - 1, 0); c <= min(z + 1, dz - 1); c++) any |= in[((uint32_t)a * (uint32_t)dy + (uint32_t)b) * (uint32_t)dz + (uint32_t)c];
    out[i] = any != 0;
}

// out cell = OR of its 4^3 children of in (dims id*; od* = ceil(id* / 4))
__global__ __launch_bounds__(256) void k_ray_map_up(const uint8_t* __restrict__ in, const int idx_, const int idy, const int idz, const int odx,
                                                    const int ody, const int odz, uint8_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)odx * (uint32_t)ody * (uint32_t)odz) return;
    const int z = (int)(i % (uint32_t)odz), y = (int)(i / (uint32_t)odz % (uint32_t)ody), x = (int)(i / ((uint32_t)odz * (uint32_t)ody));
    uint32_t any = 0;
    for (int a = 4 * x; a < min(4 * x + 4, idx_); a++)
        for (int b = 4 * y; b < min(4 * y + 4, idy); b++)
            for (int c = 4 * z; c < min(4 * z + 4, idz); c++) any |= in[((uint32_t)a * (uint32_t)idy + (uint32_t)b) * (uint32_t)idz + (uint32_t)c];
    out[i] = any != 0;
}

__device__ __forceinline__ RayHit ray_no_hit()
{
    const float qnan = __builtin_bit_cast(float, 0x7FC00000u);
    RayHit h;
    h.t = qnan;
    h.flags = 0;
    h.p[0] = h.p[1] = h.p[2] = qnan;
    h.n[0] = h.n[1] = h.n[2] = qnan;
    h.row_voxel[0] = h.row_voxel[1] = h.row_voxel[2] = -1;
    h.rgb = h.count = h.sample = 0;
    h.reserved[0] = h.reserved[1] = 0;
    return h;
}

// Samples after the current one (cell coordinate c, `rate` cells a sample, inv = 1 / rate) that stay inside [lo, hi] on this axis.
__device__ __forceinline__ double ray_axis_run(const double c, const double rate, const double inv, const double lo, const double hi)
{
    if (!__builtin_isfinite(c)) return 0.0;  // (a coordinate beyond f32: no claim)
    if (rate > 0.0) return (hi - c) * inv;
    if (rate < 0.0) return (lo - c) * inv;
    return __builtin_inf();
}

// The march of one USED ray O + t * D (fusion frame).
__device__ __forceinline__ RayHit ray_march(const GridParams& g, const Tables& t, const RayParams& p, const double O[3], const double D[3])
{
    RayHit h = ray_no_hit();
    h.flags = kRayUsed;
    double rate[3], inv[3], top[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        rate[a] = (D[a] * p.dt) * g.inv_res;
        inv[a] = rate[a] != 0.0 ? 1.0 / rate[a] : 0.0;
        top[a] = (g.max[a] - g.min[a]) * g.inv_res;
    }
    // cells taken off every bound of a jump: one, plus twice the f32 spacing of the largest coordinate the ray reaches
    double reach = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) reach = fmax(reach, fabs(O[a]) + fabs(D[a]) * (p.t0 + (double)(p.n_samples - 1u) * p.dt));
    const double slack = 1.0 + (reach * 0x1p-22) * g.inv_res;
    const double grow = (double)(8 - p.radius) - slack;  // cells by which a zero map cell may be left
    const double inf = __builtin_inf();
    bool prev_def = false, near = false;
    float prev_s = 0.f;
    uint32_t prev_nid = 0;
    int32_t pwx = -1, pwy = -1, pwz = -1;
    uint32_t k = 0;
    while (k < p.n_samples) {
        const double tk = p.t0 + (double)k * p.dt;
        F3 q;
        q.x = (float)(O[0] + tk * D[0]);
        q.y = (float)(O[1] + tk * D[1]);
        q.z = (float)(O[2] + tk * D[2]);
        const double c[3] = {((double)q.x - g.min[0]) * g.inv_res, ((double)q.y - g.min[1]) * g.inv_res, ((double)q.z - g.min[2]) * g.inv_res};
        double run = -1.0;  // >= 0: this sample is undefined, and so are the next floor(run)
        int32_t v[3] = {0, 0, 0};
        if (!valid_point(g, q)) {
            // beyond a face of the box: undefined up to that face's plane (the best of the faces it lies beyond)
            run = 0.0;
            const float qa[3] = {q.x, q.y, q.z};
#pragma unroll
            for (int a = 0; a < 3; a++) {
                if (qa[a] <= g.bb_lo[a]) run = fmax(run, ray_axis_run(c[a], rate[a], inv[a], -inf, -slack));
                else if (qa[a] >= g.bb_hi[a]) run = fmax(run, ray_axis_run(c[a], rate[a], inv[a], top[a] + slack, inf));
            }
        } else {
            voxel_coords(g, q, v[0], v[1], v[2]);
            if (v[0] >= 0 && v[1] >= 0 && v[2] >= 0 && v[0] <= g.dim[0] && v[1] <= g.dim[1] && v[2] <= g.dim[2]) {
                int lvl = -1;
#pragma unroll
                for (int l = 0; l < kRayLevels; l++) {
                    if (lvl != l - 1) continue;  // the finer map's cell holds rows: so does the coarser one's
                    const int sh = kBrickShift + 2 * l;
                    const uint32_t i = ((uint32_t)(v[0] >> sh) * (uint32_t)p.mdim[l][1] + (uint32_t)(v[1] >> sh)) * (uint32_t)p.mdim[l][2] + (uint32_t)(v[2] >> sh);
                    if (p.map[l][i] == 0) lvl = l;
                }
                if (lvl >= 0) {
                    const int sh = kBrickShift + 2 * lvl;
                    run = inf;
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        const double base = (double)((v[a] >> sh) << sh);
                        run = fmin(run, ray_axis_run(c[a], rate[a], inv[a], base - grow, base + (double)(1 << sh) + grow));
                    }
                    run = fmax(run, 0.0);  // (the sample itself is undefined whatever the slack leaves of the cell)
                }
            }
        }
        if (run >= 0.0) {
            prev_def = false;
            if (!(run < (double)p.n_samples)) break;  // (an infinite run: the ray never comes back)
            k += 1u + (run >= 1.0 ? (uint32_t)run : 0u);
            continue;
        }
        const WindowNearest wn = window_nearest(g, t, q, v, p.radius, p.min_count, p.max_d2);
        if (!wn.found) {
            prev_def = false;
            k++;
            continue;
        }
        near = true;
        const double nx = t.nv_n[3 * (uint64_t)wn.nid], ny = t.nv_n[3 * (uint64_t)wn.nid + 1], nz = t.nv_n[3 * (uint64_t)wn.nid + 2];
        const float s = (float)((nx * wn.dx + ny * wn.dy) + nz * wn.dz);
        if (prev_def && ((prev_s < 0.f) != (s < 0.f))) {
            const bool back = prev_s < 0.f;
            if (!(back && p.cull)) {
                const double w = (double)prev_s / ((double)prev_s - (double)s);
                const double th = (p.t0 + (double)(k - 1u) * p.dt) + w * p.dt;
                const bool cur = fabsf(s) < fabsf(prev_s);  // the endpoint with the smaller |s|; a tie goes to k - 1
                const Row r = record_row(g, t, t.stats, cur ? wn.nid : prev_nid, 0, 0, 0);
                h.t = (float)th;
                h.flags |= kRayHit | (back ? kRayBackface : 0u);
                h.p[0] = (float)(O[0] + th * D[0]);
                h.p[1] = (float)(O[1] + th * D[1]);
                h.p[2] = (float)(O[2] + th * D[2]);
                h.n[0] = r.nx, h.n[1] = r.ny, h.n[2] = r.nz;
                h.row_voxel[0] = cur ? wn.wx : pwx, h.row_voxel[1] = cur ? wn.wy : pwy, h.row_voxel[2] = cur ? wn.wz : pwz;
                h.rgb = r.rgb;
                h.count = r.count;
                h.sample = k;
                break;
            }
        }
        prev_def = true;
        prev_s = s;
        prev_nid = wn.nid;
        pwx = wn.wx, pwy = wn.wy, pwz = wn.wz;
        k++;
    }
    if (near) h.flags |= kRayNear;
    return h;
}

// General rays: packed {o, d} f32 records in the camera frame, one lane per ray.
__global__ __launch_bounds__(256) void k_raycast(const GridParams g, const Tables t, const RayParams p, const float* __restrict__ rays,
                                                 RayHit* __restrict__ hits)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n_rays) return;
    float in[6];
#pragma unroll
    for (int a = 0; a < 6; a++) in[a] = rays[6 * i + a];
    bool used = true;
#pragma unroll
    for (int a = 0; a < 6; a++) used = used && __builtin_isfinite(in[a]);
    RayHit h = ray_no_hit();
    if (used) {
        const double ox = in[0], oy = in[1], oz = in[2], dx = in[3], dy = in[4], dz = in[5];
        double O[3], W[3], D[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            O[a] = ((p.T[4 * a] * ox + p.T[4 * a + 1] * oy) + p.T[4 * a + 2] * oz) + p.T[4 * a + 3];
            W[a] = (p.T[4 * a] * dx + p.T[4 * a + 1] * dy) + p.T[4 * a + 2] * dz;
        }
        const double L = sqrt((W[0] * W[0] + W[1] * W[1]) + W[2] * W[2]);
        if (__builtin_isfinite(L) && L > 0.0) {
#pragma unroll
            for (int a = 0; a < 3; a++) D[a] = W[a] / L;
            h = ray_march(g, t, p, O, D);
        }
    }
    hits[i] = h;
}

// View rays: a wave takes an 8 x 8 pixel tile of view blockIdx.y; the rows p.row0 .. p.row0 + p.rows - 1 of the image.
__global__ __launch_bounds__(256) void k_raycast_view(const GridParams g, const Tables t, const RayParams p, const double* __restrict__ poses,
                                                      RayHit* __restrict__ hits)
{
    const uint64_t tile = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tiles_x = (p.width + 7u) >> 3;
    const uint32_t u = (uint32_t)(tile % tiles_x) * 8u + (lane & 7u);
    const uint64_t vr = (tile / tiles_x) * 8u + (lane >> 3);
    if (u >= p.width || vr >= p.rows) return;
    const double* T = poses + 12ull * blockIdx.y;
    const double xn = ((double)u - p.cx) / p.fx;
    const double yn = ((double)(uint32_t)(p.row0 + vr) - p.cy) / p.fy;
    double O[3], D[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        O[a] = T[4 * a + 3];
        D[a] = (T[4 * a] * xn + T[4 * a + 1] * yn) + T[4 * a + 2];
    }
    hits[(uint64_t)blockIdx.y * p.view_stride + vr * p.width + u] = ray_march(g, t, p, O, D);
}

// ---- surface mesh (hfpf_extract_mesh*, include/hfpf.h) --------------------------------------------------------------------
// Lattice and cube keys are x << 42 | y << 21 | z (21 bits an axis: lattice points reach dim, which make_key's widths do not cover).
// The cube set is the candidate rows' cells dilated by 1 (three 1-D dilations, each emit -> sort -> unique), the corner set the cubes
// dilated by (0, +1) the same way; both stay sorted, so a corner's index is a binary search and the scans run in key order.
constexpr int kMeshKeyBits = 21;
constexpr uint64_t kMeshKeyMask = (1ull << kMeshKeyBits) - 1ull;

__host__ __device__ constexpr uint64_t mesh_key(const int32_t x, const int32_t y, const int32_t z)
{
    return ((uint64_t)x << (2 * kMeshKeyBits)) | ((uint64_t)y << kMeshKeyBits) | (uint64_t)z;
}

__device__ __forceinline__ int32_t mesh_key_axis(const uint64_t k, const int a) { return (int32_t)((k >> (kMeshKeyBits * (2 - a))) & kMeshKeyMask); }

// The winding table of the Kuhn tetrahedra, derived at compile time.  Cube corner codes are 4 dx + 2 dy + dz; tetrahedron T of the
// permutation pi (xyz, xzy, yxz, yzx, zxy, zyx) has the corners 0, e_pi1, e_pi1 + e_pi2, 7.  Case m (bit i: corner i inside) gives
// n triangles; a triangle vertex is the lattice edge (origin code << 3) | direction code, direction = the far corner's code minus
// the origin's (0 < d <= 7: the corners of a tetrahedron are ordered componentwise).  Edges are (I-th inside, O-th outside) corner
// pairs; the winding makes the face normal of the edge-midpoint triangle point from the inside corners to the outside ones.
struct MeshCase {
    uint8_t n;
    uint8_t e[2][3];
};
struct MeshTable {
    uint8_t tet[6][4];
    MeshCase c[6][16];
};

constexpr MeshTable make_mesh_table()
{
    MeshTable m{};
    const uint8_t tets[6][4] = {{0, 4, 6, 7}, {0, 4, 5, 7}, {0, 2, 6, 7}, {0, 2, 3, 7}, {0, 1, 5, 7}, {0, 1, 3, 7}};
    for (int t = 0; t < 6; t++) {
        for (int i = 0; i < 4; i++) m.tet[t][i] = tets[t][i];
        for (int mask = 0; mask < 16; mask++) {
            int in[4] = {}, out[4] = {}, ni = 0, no = 0;
            for (int i = 0; i < 4; i++) {
                if (mask >> i & 1) in[ni++] = i;
                else out[no++] = i;
            }
            int tri[2][3][2] = {};  // (inside, outside) local corners per triangle vertex
            int n = 0;
            if (ni == 1) {
                n = 1;
                for (int k = 0; k < 3; k++) tri[0][k][0] = in[0], tri[0][k][1] = out[k];
            } else if (ni == 3) {
                n = 1;
                for (int k = 0; k < 3; k++) tri[0][k][0] = in[k], tri[0][k][1] = out[0];
            } else if (ni == 2) {  // (e00, e01, e11) and (e00, e11, e10)
                n = 2;
                const int q[2][3][2] = {{{0, 0}, {0, 1}, {1, 1}}, {{0, 0}, {1, 1}, {1, 0}}};
                for (int r = 0; r < 2; r++)
                    for (int k = 0; k < 3; k++) tri[r][k][0] = in[q[r][k][0]], tri[r][k][1] = out[q[r][k][1]];
            }
            m.c[t][mask].n = (uint8_t)n;
            // the direction the normal should take: |I| * sum(outside corners) - |O| * sum(inside corners)
            int want[3] = {0, 0, 0};
            for (int a = 0; a < 3; a++) {
                for (int k = 0; k < no; k++) want[a] += ni * (tets[t][out[k]] >> (2 - a) & 1);
                for (int k = 0; k < ni; k++) want[a] -= no * (tets[t][in[k]] >> (2 - a) & 1);
            }
            for (int r = 0; r < n; r++) {
                int mid[3][3] = {};  // twice the edge midpoints
                uint8_t code[3] = {};
                for (int k = 0; k < 3; k++) {
                    const int u = tets[t][tri[r][k][0]], w = tets[t][tri[r][k][1]];
                    for (int a = 0; a < 3; a++) mid[k][a] = (u >> (2 - a) & 1) + (w >> (2 - a) & 1);
                    const int lo = u < w ? u : w, hi = u < w ? w : u;
                    code[k] = (uint8_t)(lo << 3 | (hi - lo));
                }
                int ab[3] = {}, ac[3] = {};
                for (int a = 0; a < 3; a++) ab[a] = mid[1][a] - mid[0][a], ac[a] = mid[2][a] - mid[0][a];
                const int nrm[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
                const int dot = nrm[0] * want[0] + nrm[1] * want[1] + nrm[2] * want[2];
                m.c[t][mask].e[r][0] = code[0];
                m.c[t][mask].e[r][1] = dot > 0 ? code[1] : code[2];
                m.c[t][mask].e[r][2] = dot > 0 ? code[2] : code[1];
            }
        }
    }
    return m;
}
__constant__ MeshTable kMeshTable = make_mesh_table();

struct MeshParams {
    double min_count;  // max(1, min_count)
    double max_d2;     // max_distance * max_distance
    int32_t radius;    // 1..4
};

struct MeshVertex {  // = hfpf_mesh_vertex
    float x, y, z, nx, ny, nz;
    uint32_t rgb, count;
};
static_assert(sizeof(MeshVertex) == 32, "mesh vertex is 32 bytes");

// The index of key in the sorted unique keys[0, n).  The callers look up keys the construction puts there; a miss would be a broken
// invariant: it sets *miss (the host then fails the call) and returns 0, an index that is safe to read.
__device__ __forceinline__ uint32_t mesh_find(const uint64_t* __restrict__ keys, const uint32_t n, const uint64_t key, uint32_t* __restrict__ miss)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    if (lo < n && keys[lo] == key) return lo;
    atomicOr(miss, 1u);
    return 0;
}

// Lattice coordinate c[a] = (float)(bbox_min[a] + (double)i * res): one f64 multiply and add (never contracted), one rounding.
__device__ __forceinline__ F3 mesh_lattice_point(const GridParams& g, const uint64_t k)
{
    F3 c;
    c.x = (float)(g.min[0] + (double)mesh_key_axis(k, 0) * g.res);
    c.y = (float)(g.min[1] + (double)mesh_key_axis(k, 1) * g.res);
    c.z = (float)(g.min[2] + (double)mesh_key_axis(k, 2) * g.res);
    return c;
}

// The candidate rows' cells (extract order: already sorted and unique).
__global__ __launch_bounds__(256) void k_mesh_row_keys(const Row* __restrict__ rows, const uint64_t n, uint64_t* __restrict__ keys)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    keys[j] = mesh_key(rows[j].ix, rows[j].iy, rows[j].iz);
}

// One 1-D dilation along axis a: key j emits its neighbours at offsets lo..hi, clamped into 0..lim.  A clamped neighbour repeats the
// offset-0 key or one inside the range (lo <= 0 <= hi and the input lies in 0..lim), so the unique pass drops it.
__global__ __launch_bounds__(256) void k_mesh_dilate(const uint64_t* __restrict__ in, const uint64_t n, const int a, const int lo, const int hi,
                                                     const int32_t lim, uint64_t* __restrict__ out)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t k = in[j];
    const int sh = kMeshKeyBits * (2 - a);
    const int32_t c = (int32_t)((k >> sh) & kMeshKeyMask);
    const uint64_t rest = k & ~(kMeshKeyMask << sh);
    const int w = hi - lo + 1;
    for (int o = lo; o <= hi; o++) out[j * w + (o - lo)] = rest | ((uint64_t)min(max(c + o, 0), lim) << sh);
}

// One lane per corner: the hfpf_query hit of lattice point c under the identity pose (transform_point of the identity is c itself).
// Defined iff FOUND: nid != 0 (record 0 is never a row) and s = its signed distance.
__global__ __launch_bounds__(256) void k_mesh_sample(const GridParams g, const Tables t, const MeshParams p, const uint64_t* __restrict__ corners,
                                                     const uint32_t n, float* __restrict__ s_out, uint32_t* __restrict__ nid_out)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const F3 q = mesh_lattice_point(g, corners[k]);
    float s = 0.f;
    uint32_t nid = 0;
    if (valid_point(g, q)) {
        int32_t v[3];
        voxel_coords(g, q, v[0], v[1], v[2]);
        const WindowNearest wn = window_nearest(g, t, q, v, p.radius, p.min_count, p.max_d2);
        if (wn.found) {
            const double nx = t.nv_n[3 * (uint64_t)wn.nid], ny = t.nv_n[3 * (uint64_t)wn.nid + 1], nz = t.nv_n[3 * (uint64_t)wn.nid + 2];
            s = (float)((nx * wn.dx + ny * wn.dy) + nz * wn.dz);
            nid = wn.nid;
        }
    }
    s_out[k] = s;
    nid_out[k] = nid;
}

// The 8 corner indices of cube key ck and its 6 tetrahedron cases; false when a corner is undefined (the cube is not meshed).
__device__ __forceinline__ bool mesh_cube(const uint64_t ck, const uint64_t* __restrict__ corners, const uint32_t nk, const float* __restrict__ s,
                                          const uint32_t* __restrict__ nid, uint32_t* __restrict__ miss, uint32_t idx[8], uint32_t cases[6])
{
    uint32_t inside = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        idx[c] = mesh_find(corners, nk, ck + mesh_key(c >> 2, (c >> 1) & 1, c & 1), miss);
        if (nid[idx[c]] == 0) return false;
        inside |= (s[idx[c]] < 0.f ? 1u : 0u) << c;
    }
#pragma unroll
    for (int tt = 0; tt < 6; tt++) {
        uint32_t m = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) m |= (inside >> kMeshTable.tet[tt][i] & 1u) << i;
        cases[tt] = m;
    }
    return true;
}

// One lane per cube (plus one that zeroes the scan's extra element): OR each crossing edge's direction bit (bit d - 1) into its
// origin corner's mark, and count the cube's triangles.  The marks are ORs, so they do not depend on the order cubes run in.
__global__ __launch_bounds__(256) void k_mesh_mark(const uint64_t* __restrict__ cubes, const uint32_t nc, const uint64_t* __restrict__ corners,
                                                   const uint32_t nk, const float* __restrict__ s, const uint32_t* __restrict__ nid,
                                                   uint32_t* __restrict__ marks, uint32_t* __restrict__ tri_count, uint32_t* __restrict__ miss)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > nc) return;
    if (j == nc) {
        tri_count[nc] = 0;
        return;
    }
    uint32_t idx[8], cases[6];
    uint32_t n_tri = 0;
    if (mesh_cube(cubes[j], corners, nk, s, nid, miss, idx, cases)) {
        uint32_t local[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int tt = 0; tt < 6; tt++) {
            const MeshCase& mc = kMeshTable.c[tt][cases[tt]];
            n_tri += mc.n;
            for (int r = 0; r < mc.n; r++)
#pragma unroll
                for (int v = 0; v < 3; v++) local[mc.e[r][v] >> 3] |= 1u << ((mc.e[r][v] & 7) - 1);
        }
#pragma unroll
        for (int c = 0; c < 8; c++)
            if (local[c]) atomicOr(&marks[idx[c]], local[c]);
    }
    tri_count[j] = n_tri;
}

// Per corner its vertex count (the popcount of its marks); element nk is 0, so element nk of the exclusive scan is the total.
__global__ __launch_bounds__(256) void k_mesh_vcount(const uint32_t* __restrict__ marks, const uint32_t nk, uint32_t* __restrict__ vcount)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nk) return;
    vcount[k] = k < nk ? (uint32_t)__builtin_popcount(marks[k]) : 0u;
}

// One lane per corner: its vertices in direction order.  t and p in f64, left to right, never contracted; the attributes come from
// the row of the endpoint with the smaller |s| (a tie goes to the origin).
__global__ __launch_bounds__(256) void k_mesh_vertices(const GridParams g, const Tables t, const uint64_t* __restrict__ corners, const uint32_t nk,
                                                       const float* __restrict__ s, const uint32_t* __restrict__ nid, const uint32_t* __restrict__ marks,
                                                       const uint32_t* __restrict__ vbase, MeshVertex* __restrict__ out, uint32_t* __restrict__ miss)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nk) return;
    uint32_t m = marks[k];
    if (!m) return;
    uint32_t o = vbase[k];
    const uint64_t ka = corners[k];
    const F3 ca = mesh_lattice_point(g, ka);
    const float sa = s[k];
    while (m) {
        const int d = __builtin_ctz(m) + 1;
        m &= m - 1;
        const uint64_t kb = ka + mesh_key(d >> 2, (d >> 1) & 1, d & 1);
        const uint32_t b = mesh_find(corners, nk, kb, miss);
        const F3 cb = mesh_lattice_point(g, kb);
        const float sb = s[b];
        const double tt = (double)sa / ((double)sa - (double)sb);
        MeshVertex v;
        v.x = (float)((double)ca.x + tt * ((double)cb.x - (double)ca.x));
        v.y = (float)((double)ca.y + tt * ((double)cb.y - (double)ca.y));
        v.z = (float)((double)ca.z + tt * ((double)cb.z - (double)ca.z));
        const uint32_t w = fabsf(sb) < fabsf(sa) ? nid[b] : nid[k];
        const Row r = record_row(g, t, t.stats, w, 0, 0, 0);
        v.nx = r.nx, v.ny = r.ny, v.nz = r.nz;
        v.rgb = r.rgb;
        v.count = r.count;
        out[o++] = v;
    }
}

// One lane per cube: its triangles from tbase[j] on, by tetrahedron 0..5 and triangle 0..1.  A vertex id is its origin corner's
// vbase plus the number of marks below its direction bit.
__global__ __launch_bounds__(256) void k_mesh_triangles(const uint64_t* __restrict__ cubes, const uint32_t nc, const uint64_t* __restrict__ corners,
                                                        const uint32_t nk, const float* __restrict__ s, const uint32_t* __restrict__ nid,
                                                        const uint32_t* __restrict__ marks, const uint32_t* __restrict__ vbase,
                                                        const uint32_t* __restrict__ tbase, uint32_t* __restrict__ tris, uint32_t* __restrict__ miss)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nc) return;
    if (tbase[j + 1] == tbase[j]) return;
    uint32_t idx[8], cases[6];
    if (!mesh_cube(cubes[j], corners, nk, s, nid, miss, idx, cases)) return;
    uint64_t o = (uint64_t)tbase[j] * 3;
    for (int tt = 0; tt < 6; tt++) {
        const MeshCase& mc = kMeshTable.c[tt][cases[tt]];
        for (int r = 0; r < mc.n; r++)
#pragma unroll
            for (int v = 0; v < 3; v++) {
                const uint32_t e = mc.e[r][v], c = idx[e >> 3], d = e & 7;
                tris[o++] = vbase[c] + (uint32_t)__builtin_popcount(marks[c] & ((1u << (d - 1)) - 1u));
            }
    }
}

// ---- connected components (hfpf_extract_components*, include/hfpf.h) -------------------------------------------------------
// The rows are the extract row set of opts.min_count (k_extract_keys -> sort -> k_extract_rows), row j the j-th in lexicographic
// order; row_of[] maps a record to its row.  k_comp_link unites every row with its adjacent rows of smaller index in a lock-free
// union-find over parent[] (parent[x] <= x always: the smaller root wins, so a component's root is its smallest row whatever the
// schedule), k_comp_flatten names every row's root, a scan over the root flags numbers the components by ascending representative,
// k_comp_reduce sums them up with integer atomics, and after the keep decision two more scans compact rows, labels and records.
constexpr uint32_t kCompNone = 0xFFFFFFFFu;

struct __attribute__((aligned(8))) Component {  // = hfpf_component
    uint32_t first_row, n_rows;
    unsigned long long points;
    int32_t lo[3], hi[3];
    uint32_t source_row, reserved;
};
static_assert(sizeof(Component) == 48, "component is 48 bytes");

struct CompParams {
    double min_dot;                 // min_normal_dot
    unsigned long long min_points;
    uint32_t min_rows, keep_largest;
    int32_t reach;                  // 1..kQueryMaxRadius
};

// row_of[nid] = j for the records of the sorted row set (row_of is all kCompNone before), parent[j] = j.
__global__ __launch_bounds__(256) void k_comp_index(const uint32_t* __restrict__ vals, const uint32_t n_rows, uint32_t* __restrict__ row_of,
                                                    uint32_t* __restrict__ parent)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_rows) return;
    row_of[vals[j]] = j;
    parent[j] = j;
}

__device__ __forceinline__ uint32_t comp_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x as far as this lane can see, with path halving.  Every value parent[x] ever holds is a row of x's component not
// above x, so a stale read costs a step and an atomicMin never loses a link.
__device__ __forceinline__ uint32_t comp_find(uint32_t* parent, uint32_t x)
{
    for (;;) {
        const uint32_t p = comp_load(&parent[x]);
        if (p == x) return x;
        const uint32_t gp = comp_load(&parent[p]);
        if (gp != p) atomicMin(&parent[x], gp);
        x = gp;
    }
}

// Hook the larger root under the smaller.  atomicMin returns what the larger one pointed to: itself, and the hook is done; or
// another row `old` that got in first.  parent[a] is then min(old, b), which keeps a with one of them, and the pair (old, b) is what
// remains to be united.
__device__ __forceinline__ void comp_unite(uint32_t* parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = comp_find(parent, a);
        b = comp_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t s = a;
            a = b, b = s;
        }
        const uint32_t old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;
    }
}

// One lane per row j, in row order: the rows of the (2 reach + 1)^3 window that precede j lexicographically all have x <= j's x, so
// only that half of the window is walked.
__global__ __launch_bounds__(256) void k_comp_link(const GridParams g, const Tables t, const CompParams p, const Row* __restrict__ rows,
                                                   const uint32_t n_rows, const uint32_t* __restrict__ row_of, const uint32_t n_records,
                                                   uint32_t* __restrict__ parent)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_rows) return;
    const int32_t v[3] = {rows[j].ix, rows[j].iy, rows[j].iz};
    const double nx = rows[j].nx, ny = rows[j].ny, nz = rows[j].nz;
    int lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = max(v[a] - p.reach, 0);
        hi[a] = min(v[a] + (a == 0 ? 0 : p.reach), g.dim[a] - 1);
    }
    window_walk(g, t, lo, hi, [&](const int32_t, const int32_t, const int32_t, const uint32_t nid) {
        if (nid > n_records) return;  // (row_of has n_records + 1 entries; every record of the tables is below that)
        const uint32_t i = row_of[nid];
        if (i >= j) return;  // later rows unite with j themselves; kCompNone: a record without a row
        const double dot = (nx * (double)t.nv_n[3 * (uint64_t)nid] + ny * (double)t.nv_n[3 * (uint64_t)nid + 1]) + nz * (double)t.nv_n[3 * (uint64_t)nid + 2];
        if (!(dot >= p.min_dot)) return;
        comp_unite(parent, i, j);
    });
}

// root[j] = the root of j (k_comp_link has finished: the forest is final), flag[j] = 1 for a root.  flag has n_rows + 1 entries, the
// last one 0 for the scan.
__global__ __launch_bounds__(256) void k_comp_flatten(const uint32_t* __restrict__ parent, const uint32_t n_rows, uint32_t* __restrict__ root,
                                                      uint32_t* __restrict__ flag)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n_rows) return;
    if (j == n_rows) {
        flag[j] = 0;
        return;
    }
    uint32_t r = j;
    for (uint32_t q = parent[r]; q != r; q = parent[r]) r = q;
    root[j] = r;
    flag[j] = r == j ? 1u : 0u;
}

// comp_of[j] = the number of j's component (cbase = the exclusive scan of the root flags); a root also sets up its record.
__global__ __launch_bounds__(256) void k_comp_init(const uint32_t* __restrict__ root, const uint32_t* __restrict__ cbase, const uint32_t n_rows,
                                                   uint32_t* __restrict__ comp_of, Component* __restrict__ comps)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_rows) return;
    const uint32_t r = root[j], c = cbase[r];
    comp_of[j] = c;
    if (r != j) return;
    Component k;
    k.first_row = 0, k.n_rows = 0, k.points = 0;
    k.lo[0] = k.lo[1] = k.lo[2] = INT_MAX;
    k.hi[0] = k.hi[1] = k.hi[2] = INT_MIN;
    k.source_row = j, k.reserved = 0;
    comps[c] = k;
}

// n_rows, points and the index box of every component.  Rows are in lexicographic order, so most waves hold rows of one component:
// such a wave reduces in registers and issues one set of atomics, a mixed wave one set per lane.
__global__ __launch_bounds__(256) void k_comp_reduce(const Row* __restrict__ rows, const uint32_t* __restrict__ comp_of, const uint32_t n_rows,
                                                     Component* __restrict__ comps)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = j < n_rows;
    const uint32_t jj = live ? j : n_rows - 1;  // (n_rows > 0) a dead lane mirrors the last row and adds nothing
    const uint32_t c = comp_of[jj];
    uint32_t n = live ? 1u : 0u;
    unsigned long long pts = live ? (unsigned long long)rows[jj].count : 0ull;
    int32_t lo[3] = {rows[jj].ix, rows[jj].iy, rows[jj].iz}, hi[3] = {lo[0], lo[1], lo[2]};
    const bool uniform = __all(c == __shfl(c, 0));
    if (uniform) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            n += __shfl_down(n, o);
            pts += __shfl_down(pts, o);
#pragma unroll
            for (int a = 0; a < 3; a++) {
                lo[a] = min(lo[a], __shfl_down(lo[a], o));
                hi[a] = max(hi[a], __shfl_down(hi[a], o));
            }
        }
        if ((threadIdx.x & 63u) != 0) return;
    } else if (!live) {
        return;
    }
    Component* k = &comps[c];
    atomicAdd(&k->n_rows, n);
    atomicAdd(&k->points, pts);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        atomicMin(&k->lo[a], lo[a]);
        atomicMax(&k->hi[a], hi[a]);
    }
}

__device__ __forceinline__ bool comp_passes(const Component& k, const CompParams& p) { return k.n_rows >= p.min_rows && k.points >= p.min_points; }

// keep[c] without keep_largest (keep has n_comps + 1 entries, the last one 0 for the scan) ...
__global__ __launch_bounds__(256) void k_comp_keep(const Component* __restrict__ comps, const uint32_t n_comps, const CompParams p, uint32_t* __restrict__ keep)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n_comps) return;
    keep[c] = c < n_comps && comp_passes(comps[c], p) ? 1u : 0u;
}
// ... and with it: the sort key puts the passing components in front, n_rows descending, then representative ascending; the others get
// the all-ones key (a representative is below 2^32 - 1, so no passing key is all ones).
__global__ __launch_bounds__(256) void k_comp_rank_keys(const Component* __restrict__ comps, const uint32_t n_comps, const CompParams p,
                                                        uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t* __restrict__ keep)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n_comps) return;
    keep[c] = 0;
    if (c == n_comps) return;
    const Component k = comps[c];
    keys[c] = comp_passes(k, p) ? ((uint64_t)(~k.n_rows) << 32) | k.source_row : ~0ull;
    vals[c] = c;
}
__global__ __launch_bounds__(256) void k_comp_rank_keep(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, const uint32_t n_front,
                                                        uint32_t* __restrict__ keep)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_front && keys[r] != ~0ull) keep[vals[r]] = 1;
}

// rkeep[j] = 1 for a row of a kept component (n_rows + 1 entries, the last one 0 for the scan)
__global__ __launch_bounds__(256) void k_comp_row_keep(const uint32_t* __restrict__ comp_of, const uint32_t* __restrict__ keep, const uint32_t n_rows,
                                                       uint32_t* __restrict__ rkeep)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n_rows) return;
    rkeep[j] = j < n_rows ? keep[comp_of[j]] : 0u;
}

// The outputs: kept rows (out_rows may be null) and their labels at rbase[j], kept records at kbase[c] (written by the representative).
__global__ __launch_bounds__(256) void k_comp_compact(const Row* __restrict__ rows, const uint32_t n_rows, const uint32_t* __restrict__ comp_of,
                                                      const uint32_t* __restrict__ keep, const uint32_t* __restrict__ kbase,
                                                      const uint32_t* __restrict__ rbase, const Component* __restrict__ comps,
                                                      Row* __restrict__ out_rows, uint32_t* __restrict__ out_labels, Component* __restrict__ out_comps)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_rows) return;
    const uint32_t c = comp_of[j];
    if (!keep[c]) return;
    const uint32_t o = rbase[j], label = kbase[c];
    if (out_rows) out_rows[o] = rows[j];
    out_labels[o] = label;
    if (comps[c].source_row != j) return;
    Component k = comps[c];
    k.first_row = o;
    out_comps[label] = k;
}


// ---- multi-GPU epoch exchange ----------------------------------------------------------
// Frames shard across ranks; what must be agreed before a clean pass is the occupancy set and, per cell, the
// smallest frame id that touched it (the viewpoint latch).  Each rank exports the cells IT occupied since
// the last exchange and imports everybody else's; normals and registrations are then computed redundantly
// and deterministically on every rank, while buffers and statistic sums stay private partial state.
// One 16-byte record per newly occupied cell (key, smallest frame id that touched it) and TWO per frame the rank has integrated since
// the last exchange (the frame's viewpoint: ranks only know their own frames' poses, and a cell's latch may name anybody's frame).
// Until round 4 every cell record carried its frame's viewpoint: 32 bytes a cell, 338 MB received per rank in the first epoch of
// eight cameras (profiles/r04_virtual_ranks.md); the viewpoints now travel once per frame.
struct __attribute__((aligned(16))) EpochRec {
    uint64_t key;  // cell key (below 2^63), or kEpochFrame | half << 62 | frame id
    union {
        struct {
            uint32_t first_frame, pad;
        };
        struct {
            float a, b;  // half 0: viewpoint x, y; half 1: viewpoint z, 0
        };
    };
};
static_assert(sizeof(EpochRec) == 16, "EpochRec is 16 bytes");
constexpr uint64_t kEpochFrame = 1ull << 63, kEpochFrameHalf = 1ull << 62;

// Records [0, n_cells): the cells occ_list[first .. first + n_cells); behind them two records per frame of frame_list[frame_first .. + n_frames).
__global__ __launch_bounds__(256) void k_epoch_export(const GridParams g, const Tables t, const uint64_t first, const uint64_t n_cells, const uint64_t frame_first,
                                                      const uint64_t n_frames, EpochRec* __restrict__ out)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_cells + 2 * n_frames) return;
    EpochRec r;
    if (j < n_cells) {
        const uint32_t slot = t.occ_list[first + j];
        int32_t x, y, z;
        slot_coords(g, t, slot, x, y, z);
        r.key = make_key(g, x, y, z);
        r.first_frame = t.first_frame[slot];
        r.pad = 0;
    } else {
        const uint64_t k = j - n_cells;
        const uint32_t fid = t.frame_list[frame_first + (k >> 1)];
        const uint32_t half = (uint32_t)(k & 1u);
        r.key = kEpochFrame | (half ? kEpochFrameHalf : 0ull) | fid;
        r.a = t.frame_vp[3 * (uint64_t)fid + 2 * half];
        r.b = half ? 0.f : t.frame_vp[3 * (uint64_t)fid + 1];
    }
    out[j] = r;
}

__global__ __launch_bounds__(256) void k_epoch_import(const GridParams g, const Tables t, const EpochRec* __restrict__ in, const uint64_t n)
{
    // kImportTiles tiles per workgroup, one occ_list reservation (hot counter: see k_register)
    uint32_t slot_[kImportTiles];
    uint32_t f_first = 0;
#pragma unroll
    for (int tt = 0; tt < kImportTiles; tt++) {
        const uint64_t j = ((uint64_t)blockIdx.x * kImportTiles + tt) * 256u + threadIdx.x;
        bool want = j < n;
        EpochRec r;
        r.key = 0;
        r.first_frame = kNoFrame;
        r.pad = 0;
        int32_t x = 0, y = 0, z = 0;
        if (want) {
            r = in[j];
            if (r.key & kEpochFrame) {  // a frame's viewpoint (the same value from every exporter)
                const uint32_t fid = (uint32_t)r.key;
                if (fid < t.max_frames) {
                    if (r.key & kEpochFrameHalf) {
                        t.frame_vp[3 * (uint64_t)fid + 2] = r.a;
                    } else {
                        t.frame_vp[3 * (uint64_t)fid] = r.a;
                        t.frame_vp[3 * (uint64_t)fid + 1] = r.b;
                    }
                }
                want = false;
            } else {
                key_coords(g, r.key, x, y, z);
                // storage extent is dim+1 (grid.hpp:626): 0..dim is kept.  x is judged on the key's own bits: key_coords narrows
                // them to int32, and a transport's key with more than 31 bits there would come out negative or as another cell's x
                want = (r.key >> g.key_sx) <= (uint64_t)g.dim[0] && y <= g.dim[1] && z <= g.dim[2];
            }
        }
        const uint32_t bidx = want ? brick_index(g, x, y, z) : 0u;
        const uint32_t b = brick_acquire_wave(t, bidx, want);
        want = want && b != 0;
        const uint32_t slot = b * kBrickCells + local_index(x, y, z);
        slot_[tt] = slot;
        if (want) {
            const unsigned long long bit = 1ull << (((y & 7) << 3) | (z & 7));
            const unsigned long long old = atomicOr(reinterpret_cast<unsigned long long*>(&t.occ_mask[(uint64_t)b * 8 + (x & 7)]), bit);
            if (!(old & bit)) f_first |= 1u << tt;  // (joins occ_list: the clean pass this import opens files its pre-dependant, k_clean_begin)
            if (r.first_frame < t.max_frames) atomicMin(&t.first_frame[slot], r.first_frame);
        }
    }
    __shared__ BlockReserveScratch brs;
    unsigned long long oi = block_reserve_n(&t.ctr[C_OCC], (uint32_t)__popc(f_first), brs);
    bool overflow = false;
#pragma unroll
    for (int tt = 0; tt < kImportTiles; tt++) {
        if (f_first & (1u << tt)) {
            if (oi < t.max_occ) t.occ_list[oi] = slot_[tt];
            else overflow = true;
            oi++;
        }
    }
    if (overflow) atomicOr(&t.ctr[C_ERR], (unsigned long long)E_OCC);
}

// Diagnostic: keys of every occupied cell.
__global__ __launch_bounds__(256) void k_occupied_keys(const GridParams g, const Tables t, const uint64_t n_occ, uint64_t* __restrict__ keys)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_occ) return;
    int32_t x, y, z;
    slot_coords(g, t, t.occ_list[j], x, y, z);
    keys[j] = make_key(g, x, y, z);
}

// ---- hidden rows (hfpf_hide_*, include/hfpf.h) -------------------------------------------------------------------------------
// H is Tables::hidden, one word per (brick, x-plane).  A call marks the matched cells M in a scratch array of the same shape (from a
// list: k_hide_mark; from a box: k_hide_box), then k_hide_apply turns every word of the used bricks into op(old, mark, normal_found)
// and counts.  Word w = brick * 8 + (x & 7); the words of brick 0 (the null brick) are never touched.
struct HideCounts {  // one call's counters, zeroed in front of it
    unsigned long long n_selected, n_matched;
    unsigned long long n_changed, n_hidden, n_full, n_bad;  // k_hide_apply; n_bad: words whose HIDDEN bits leave F (a restored blob)
};
struct HideList {  // the entries of one launch
    const uint8_t* voxels;  // entry i: three int32 at voxels + i * voxel_stride
    const uint8_t* select;  // NULL: every entry is selected; else a uint32 at select + i * select_stride
    uint64_t n;
    uint32_t voxel_stride, select_stride, select_mask, select_value;
    uint32_t n_bricks;      // brick ids the mark array covers (1..n_bricks)
};
struct HideBoxArgs {
    int32_t lo[3], hi[3];  // inclusive, inside 0..dim-1 (host_plan.hpp clip_hide_box)
};

// dst[k] += the workgroup's sum of v[k]: reduced per wave (wave64), then in LDS, then ONE device atomic per workgroup and counter, as
// k_extract_keys counts its rows.  Every thread of the workgroup calls it (barriers).
template <int N>
__device__ __forceinline__ void hide_block_count(const uint32_t (&v)[N], unsigned long long* dst)
{
    __shared__ unsigned int s[N];
    if (threadIdx.x < N) s[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) {
        uint32_t x = v[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
        if ((threadIdx.x & 63u) == 0 && x) atomicAdd(&s[k], x);
    }
    __syncthreads();
    if (threadIdx.x < N && s[threadIdx.x]) atomicAdd(&dst[threadIdx.x], (unsigned long long)s[threadIdx.x]);
}

// One lane per entry: select test, range test, directory lookup (32-bit unsigned linear index, window_walk's arithmetic), the cell's
// record and normal_found bit; a matched entry sets its cell's bit in mark.
__global__ __launch_bounds__(256) void k_hide_mark(const GridParams g, const Tables t, const HideList L, unsigned long long* __restrict__ mark,
                                                   HideCounts* __restrict__ cnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t c[2] = {0, 0};  // selected, matched
    if (i < L.n) {
        bool sel = true;
        if (L.select) sel = (*reinterpret_cast<const uint32_t*>(L.select + i * L.select_stride) & L.select_mask) == L.select_value;
        if (sel) {
            c[0] = 1;
            const int32_t* v = reinterpret_cast<const int32_t*>(L.voxels + i * L.voxel_stride);
            const int32_t x = v[0], y = v[1], z = v[2];
            if (valid_coord(g, x, y, z)) {
                const uint32_t b = t.dir[brick_index(g, x, y, z)];
                if (b != 0 && b != kLock && b <= L.n_bricks) {
                    const uint64_t plane = (uint64_t)b * 8u + ((uint32_t)x & 7u);
                    const uint64_t bit = 1ull << ((((uint32_t)y & 7u) << 3) | ((uint32_t)z & 7u));
                    if ((t.nd_mask[plane * 2] & bit) && t.stat_id[b * kBrickCells + local_index(x, y, z)] != 0) {
                        c[1] = 1;
                        atomicOr(&mark[plane], (unsigned long long)bit);
                    }
                }
            }
        }
    }
    hide_block_count(c, &cnt->n_selected);
}

// F on plane word w: the normal_found bits of the cells extract emits, and the word's brick coordinates.  The storage has dim + 1 cells
// an axis, and a cell at index == dim may hold a record; it is no row (k_extract_keys' valid_coord), so it is no part of F.
__device__ __forceinline__ uint64_t hide_full_word(const GridParams& g, const Tables& t, const uint64_t w, int& bx, int& by, int& bz)
{
    const uint32_t lin = t.brick_lin[w >> 3];
    bz = (int)(lin % (uint32_t)g.bdim[2]);
    const uint32_t r = lin / (uint32_t)g.bdim[2];
    by = (int)(r % (uint32_t)g.bdim[1]), bx = (int)(r / (uint32_t)g.bdim[1]);
    const int yb = min(g.dim[1] - 1 - 8 * by, 7), zb = min(g.dim[2] - 1 - 8 * bz, 7);
    if (8 * bx + (int)(w & 7u) >= g.dim[0] || yb < 0 || zb < 0) return 0ull;
    return t.nd_mask[w * 2] & plane_window(0, yb, 0, zb);
}

// One lane per (brick, x-plane) word of the used bricks: the box's (y, z) window on that plane, ANDed with F.
__global__ __launch_bounds__(256) void k_hide_box(const GridParams g, const Tables t, const HideBoxArgs B, const uint32_t n_bricks,
                                                  unsigned long long* __restrict__ mark, HideCounts* __restrict__ cnt)
{
    const uint64_t w = 8u + (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t c[1] = {0};
    if (w < ((uint64_t)n_bricks + 1) * 8u) {
        int bx, by, bz;
        const uint64_t full = hide_full_word(g, t, w, bx, by, bz);
        const int x = 8 * bx + (int)(w & 7u);
        const int ya = max(B.lo[1] - 8 * by, 0), yb = min(B.hi[1] - 8 * by, 7), za = max(B.lo[2] - 8 * bz, 0), zb = min(B.hi[2] - 8 * bz, 7);
        if (x >= B.lo[0] && x <= B.hi[0] && ya <= yb && za <= zb) {
            const uint64_t m = plane_window(ya, yb, za, zb) & full;
            if (m) mark[w] = m;
            c[0] = (uint32_t)__popcll(m);
        }
    }
    hide_block_count(c, &cnt->n_matched);
}

// One lane per word of the used bricks: new = op(old, mark, F) (host_plan.hpp hide_word_op).  mark == NULL: nothing is
// marked; hid_in == NULL: H is empty; hid_out == NULL: count only.
__global__ __launch_bounds__(256) void k_hide_apply(const GridParams g, const Tables t, const uint32_t op, const uint32_t n_bricks, const unsigned long long* __restrict__ mark,
                                                    const uint64_t* hid_in, uint64_t* hid_out, HideCounts* __restrict__ cnt)
{
    const uint64_t w = 8u + (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t c[4] = {0, 0, 0, 0};  // changed, hidden, full, bad
    if (w < ((uint64_t)n_bricks + 1) * 8u) {
        int bx, by, bz;
        const uint64_t found = hide_full_word(g, t, w, bx, by, bz);
        const uint64_t old = hid_in ? hid_in[w] : 0ull;
        const uint64_t nw = hide_word_op(op, old, mark ? (uint64_t)mark[w] : 0ull, found);
        if (hid_out && nw != old) hid_out[w] = nw;
        c[0] = (uint32_t)__popcll(old ^ nw);
        c[1] = (uint32_t)__popcll(nw);
        c[2] = (uint32_t)__popcll(found);
        c[3] = (old & ~found) ? 1u : 0u;
    }
    hide_block_count(c, &cnt->n_changed);
}

// hfpf_get_hidden: the key of every record whose cell is HIDDEN, all ones for the others (they sort behind).  t.hidden != NULL.
__global__ __launch_bounds__(256) void k_hidden_keys(const Tables t, const uint64_t n_normals, uint64_t* __restrict__ keys)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_normals) return;
    uint64_t plane, bit;
    slot_plane_bit(t.nv_slot[j + 1], plane, bit);
    keys[j] = (t.hidden[plane] & bit) ? t.nv_key[j + 1] : ~0ull;
}

// ---- deviation from a triangle mesh (hfpf_compare_mesh*; contract in include/hfpf.h, numpy restatement tests/deviation_ref.py) ---------
// The rows are binned by the 8 x 8 x 8-voxel brick their own point P falls in (dev_cell: a monotone function of P, clamped to the
// grid's bricks, so a point outside the bounding box lands in a rim brick).  A triangle is listed in every such brick that its box,
// inflated by max_distance and a margin (dev_tri_setup), reaches: monotonicity turns "P inside the inflated box" into "P's brick
// inside the box's brick range" without a further argument.  Every row then meets the triangles of its brick in ascending index
// order and keeps the first smallest dd: the contract's winner.
struct Deviation {  // = hfpf_deviation
    float signed_distance, distance;
    uint32_t tri, flags;
    float q[3];
    uint32_t reserved;
};
static_assert(sizeof(Deviation) == 32, "deviation record is 32 bytes");

struct DevSummary {  // = hfpf_deviation_summary; max_abs as the bits of a non-negative float, which order as the floats do
    unsigned long long n_rows, n_found, n_negative, n_tris_valid, n_tris_invalid;
    uint32_t max_abs_bits, pad;
    long long sum_abs_q30, sum_sq_q30;
};
static_assert(sizeof(DevSummary) == 64, "deviation summary is 64 bytes");

struct DevTri {  // a valid triangle in the fusion frame
    double A[3], B[3], C[3], N[3];
};
static_assert(sizeof(DevTri) == 96, "triangle record is 96 bytes");

enum : int { DC_PAIRS = 0, DC_CURSOR = 1, DC_INVALID = 2, DC_WORDS = 4 };  // the counters of one call

struct DevParams {
    double T[12];        // mesh frame -> fusion frame
    double md, md2;      // max_distance and its square, as the contract compares
    double reach;        // an upper bound on |P - X| for any row point P and any point X of a triangle that can matter (host: compare_locked)
    double face_cap;     // a triangle whose face-region error bound exceeds it is listed in every brick
    uint64_t n_verts;
    uint32_t n_tris, stride;
    uint32_t nb;         // bricks that hold rows
    int32_t tile;        // triangles per LDS tile of k_dev_rows
};

constexpr int kDevTileMax = 256, kDevTileDefault = 128;
constexpr uint32_t kDevFound = 1u, kDevOnEdge = 2u, kDevOnVertex = 4u;

__device__ __forceinline__ double dev_dot(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// Brick coordinate of p on axis a.  Monotone non-decreasing in p: a rounded subtraction, a product with a positive constant, floor
// and the clamp all are.  NaN goes to brick 0.
__device__ __forceinline__ int32_t dev_cell(const GridParams& g, const int a, const double p)
{
    const double c = floor((p - g.min[a]) * (g.inv_res * 0.125));
    const int32_t top = g.bdim[a] - 1;
    return !(c > 0.0) ? 0 : (c > (double)top ? top : (int32_t)c);
}
__device__ __forceinline__ uint64_t dev_cell_key(const GridParams& g, const int32_t cx, const int32_t cy, const int32_t cz)
{
    return ((uint64_t)cx * (uint64_t)g.bdim[1] + (uint64_t)cy) * (uint64_t)g.bdim[2] + (uint64_t)cz;
}

__global__ __launch_bounds__(256) void k_dev_verts(const DevParams p, const uint8_t* __restrict__ verts, double* __restrict__ V)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= p.n_verts) return;
    const float* v = (const float*)(verts + i * p.stride);
    const double x = v[0], y = v[1], z = v[2];
#pragma unroll
    for (int a = 0; a < 3; a++) V[3 * i + a] = ((p.T[4 * a] * x + p.T[4 * a + 1] * y) + p.T[4 * a + 2] * z) + p.T[4 * a + 3];
}

// The validity rules of a triangle, shared by compare and cover (include/hfpf.h, the deviation section), in the contract's order:
// indices, finite coordinates, NN.  False when triangle k is invalid; else tr, its edges, NN and L2 = the longest edge squared.
__device__ inline bool dev_tri_valid(const uint64_t n_verts, const uint32_t* __restrict__ tris, const double* __restrict__ V, const uint32_t k, DevTri& tr,
                                     double (&ab)[3], double (&ac)[3], double& NN, double& L2)
{
    const uint32_t i0 = tris[3ull * k], i1 = tris[3ull * k + 1], i2 = tris[3ull * k + 2];
    if (i0 >= n_verts || i1 >= n_verts || i2 >= n_verts) return false;  // before anything is loaded through them
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        tr.A[a] = V[3ull * i0 + a], tr.B[a] = V[3ull * i1 + a], tr.C[a] = V[3ull * i2 + a];
        finite = finite && isfinite(tr.A[a]) && isfinite(tr.B[a]) && isfinite(tr.C[a]);
    }
    if (!finite) return false;
    double bc[3];
#pragma unroll
    for (int a = 0; a < 3; a++) ab[a] = tr.B[a] - tr.A[a], ac[a] = tr.C[a] - tr.A[a], bc[a] = tr.C[a] - tr.B[a];
    tr.N[0] = ab[1] * ac[2] - ab[2] * ac[1];
    tr.N[1] = ab[2] * ac[0] - ab[0] * ac[2];
    tr.N[2] = ab[0] * ac[1] - ab[1] * ac[0];
    NN = dev_dot(tr.N, tr.N);
    if (!(isfinite(NN) && NN > 0.0)) return false;
    L2 = fmax(dev_dot(ab, ab), fmax(dev_dot(ac, ac), dev_dot(bc, bc)));
    return true;
}

// Triangle k: false when it is invalid.  Else tr, the range lo..hi of bricks its inflated box reaches, and everywhere = list it in
// every brick.
//
// THE MARGIN.  Binning must not lose a pair whose COMPUTED dd passes dd <= md^2.  dd = (rx^2 + ry^2) + rz^2 is a rounded sum of
// non-negative terms, so dd >= fl(r_a^2) for each axis a, and dd <= md^2 implies |r_a| <= md (1 + 2^-51) with r_a = fl(P_a - Q_a),
// hence |P_a - Q_a| <= md (1 + 2^-50) for the computed Q.  It remains to bound how far the computed Q can lie outside the box of A,
// B, C per axis.  With u = 2^-53, M = the largest |coordinate| of the three vertices, L = the longest edge:
//   vertex regions: Q is a vertex, exactly.
//   edge regions: the parameter is d/(d - d') with d >= 0 >= d' as computed; fl(d - d') >= d by monotonicity, so the rounded
//     quotient lies in [0, 1] (0/0 gives NaN: dd is NaN and the triangle is not kept).  Q_a = fl(X_a + fl(t fl(Y_a - X_a))) for an edge
//     X -> Y: t fl(Y_a - X_a) lies between 0 and Y_a - X_a up to 2u|Y_a - X_a| <= 4uM, the sum rounds by at most u 3M: Q_a leaves
//     [min, max] of the box by less than 8uM = 2^-50 M.
//   face region (first order in u, not a proof): the six dots are bounded by L D, D = the largest distance from P to a vertex, and carry
//     an error of at most 6u L D; a product of two of them 13u L^2 D^2; va, vb, vc 27u L^2 D^2 each; s, whose exact value is NN, 85u
//     L^2 D^2.  With |v|, |w| <= 1 that moves v and w by at most 112u L^2 D^2 / NN each and Q by 224u L^3 D^2 / NN.  A face region
//     reached only through a rounded region test is covered too: the exact (v, w) then lies that close to the simplex.  The kernel
//     takes four times as much, 2^-43 L^3 D^2 / NN, with D replaced by p.reach, a bound over every row; where even that exceeds
//     p.face_cap (a sliver: NN tiny against L^4) the triangle goes to every brick and needs no bound.
// The 2^-49 (M + md) term of the inflation covers the edge bound and the rounding of the box itself, fl(min_a - I) and fl(max_a + I).
__device__ inline bool dev_tri_setup(const GridParams& g, const DevParams& p, const uint32_t* __restrict__ tris, const double* __restrict__ V, const uint32_t k,
                                     DevTri& tr, int32_t (&lo)[3], int32_t (&hi)[3], bool& everywhere)
{
    double ab[3], ac[3], NN, L2;
    if (!dev_tri_valid(p.n_verts, tris, V, k, tr, ab, ac, NN, L2)) return false;
    double M = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) M = fmax(M, fmax(fabs(tr.A[a]), fmax(fabs(tr.B[a]), fabs(tr.C[a]))));
    const double face = 0x1p-43 * ((L2 * sqrt(L2)) * (p.reach * p.reach)) / NN;
    everywhere = !(face <= p.face_cap);  // also an overflow to inf or NaN
    const double infl = (p.md * (1.0 + 0x1p-40) + face) + 0x1p-49 * (M + p.md);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = dev_cell(g, a, fmin(tr.A[a], fmin(tr.B[a], tr.C[a])) - infl);
        hi[a] = dev_cell(g, a, fmax(tr.A[a], fmax(tr.B[a], tr.C[a])) + infl);
    }
    return true;
}

// One wave per triangle.  EMIT = false: the triangle's record, the count of invalid triangles and of (brick, triangle) pairs.  EMIT =
// true: the pairs themselves, (brick << 32 | triangle), in any order (a sort follows).  The wave walks the smaller of the brick range
// and the list of bricks that hold rows, so two triangles through a 125^3-brick grid cost as many steps as there are bricks with rows.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_dev_tris(const GridParams g, const DevParams p, const uint32_t* __restrict__ tris, const double* __restrict__ V,
                                                  const uint64_t* __restrict__ ub_key, DevTri* __restrict__ recs, unsigned long long* __restrict__ ctr,
                                                  uint64_t* __restrict__ pairs, const uint64_t cap)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t kk = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 6;
    if (kk >= p.n_tris) return;  // the whole wave
    const uint32_t k = (uint32_t)kk;
    DevTri tr;
    int32_t lo[3], hi[3];
    bool everywhere = false;
    const bool valid = dev_tri_setup(g, p, tris, V, k, tr, lo, hi, everywhere);  // the same in every lane
    if (!valid) {
        if (!EMIT && lane == 0) atomicAdd(&ctr[DC_INVALID], 1ull);
        return;
    }
    if (!EMIT && lane < 12) ((double*)&recs[k])[lane] = lane < 3 ? tr.A[lane] : lane < 6 ? tr.B[lane - 3] : lane < 9 ? tr.C[lane - 6] : tr.N[lane - 9];
    const uint64_t ey = (uint64_t)(hi[1] - lo[1] + 1), ez = (uint64_t)(hi[2] - lo[2] + 1);
    const uint64_t vol = (uint64_t)(hi[0] - lo[0] + 1) * ey * ez;
    const bool by_list = everywhere || vol > p.nb;
    const uint64_t n_it = by_list ? p.nb : vol;
    unsigned long long cnt = 0;
    for (uint64_t i0 = 0; i0 < n_it; i0 += 64) {
        const uint64_t i = i0 + lane;
        bool hit = false;
        uint32_t b = 0;
        if (i < n_it) {
            if (by_list) {
                b = (uint32_t)i;
                hit = everywhere;
                if (!everywhere) {
                    const uint64_t key = ub_key[i];
                    const int32_t cz = (int32_t)(key % (uint64_t)g.bdim[2]);
                    const uint64_t r = key / (uint64_t)g.bdim[2];
                    const int32_t cy = (int32_t)(r % (uint64_t)g.bdim[1]), cx = (int32_t)(r / (uint64_t)g.bdim[1]);
                    hit = cx >= lo[0] && cx <= hi[0] && cy >= lo[1] && cy <= hi[1] && cz >= lo[2] && cz <= hi[2];
                }
            } else {
                const uint64_t r = i / ez;
                const uint64_t key = dev_cell_key(g, lo[0] + (int32_t)(r / ey), lo[1] + (int32_t)(r % ey), lo[2] + (int32_t)(i % ez));
                uint32_t l = 0, h = p.nb;
                while (l < h) {
                    const uint32_t mid = (l + h) >> 1;
                    if (ub_key[mid] < key) l = mid + 1;
                    else h = mid;
                }
                hit = l < p.nb && ub_key[l] == key;
                b = l;
            }
        }
        if (EMIT) {
            const unsigned long long m = __ballot(hit);
            if (m) {
                unsigned long long base = 0;
                if (lane == 0) base = atomicAdd(&ctr[DC_CURSOR], (unsigned long long)__popcll(m));
                base = __shfl(base, 0);
                const unsigned long long at = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
                if (hit && at < cap) pairs[at] = ((uint64_t)b << 32) | k;
            }
        } else {
            cnt += hit ? 1ull : 0ull;
        }
    }
    if (!EMIT) {
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
        if (lane == 0 && cnt) atomicAdd(&ctr[DC_PAIRS], cnt);
    }
}

// keys[i] = the brick of row i's point, vals[i] = i
__global__ __launch_bounds__(256) void k_dev_row_keys(const GridParams g, const Row* __restrict__ rows, const uint32_t n, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const Row& r = rows[i];
    keys[i] = dev_cell_key(g, dev_cell(g, 0, (double)r.x), dev_cell(g, 1, (double)r.y), dev_cell(g, 2, (double)r.z));
    vals[i] = i;
}

// flag[i] = sorted position i opens a brick (i < n); flag[n] = 0 for the scan
__global__ __launch_bounds__(256) void k_dev_row_flags(const uint64_t* __restrict__ keys, const uint32_t n, uint32_t* __restrict__ flag)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > n) return;
    flag[i] = i < n && (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// ub_key[b] / ub_start[b] = the key and first sorted position of brick b (base = the exclusive scan of flag); ub_start[nb] = n
__global__ __launch_bounds__(256) void k_dev_bricks(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ base,
                                                    const uint32_t n, const uint32_t nb, uint64_t* __restrict__ ub_key, uint32_t* __restrict__ ub_start)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > n) return;
    if (i == n) ub_start[nb] = n;
    else if (flag[i]) ub_key[base[i]] = keys[i], ub_start[base[i]] = i;
}

// tstart[b] .. tend[b] = the sorted pairs of brick b (both arrays zeroed before: a brick without triangles keeps an empty range)
__global__ __launch_bounds__(256) void k_dev_tri_ranges(const uint64_t* __restrict__ pairs, const uint32_t n, const uint32_t nb, uint32_t* __restrict__ tstart,
                                                        uint32_t* __restrict__ tend)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t b = (uint32_t)(pairs[i] >> 32);
    if (b >= nb) return;  // cannot happen: the pairs are k_dev_tris' own
    if (i == 0 || (uint32_t)(pairs[i - 1] >> 32) != b) tstart[b] = i;
    if (i + 1 == n || (uint32_t)(pairs[i + 1] >> 32) != b) tend[b] = i + 1;
}

// The contract's closest point of triangle t (12 doubles: A, B, C, N) to P: Q, the region's flag bits, and dd as the return value.
__device__ __forceinline__ double dev_closest(const double (&P)[3], const double* __restrict__ t, double (&Q)[3], uint32_t& region)
{
    const double* A = t;
    const double* B = t + 3;
    const double* C = t + 6;
    const double ab[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
    const double ac[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
    const double ap[3] = {P[0] - A[0], P[1] - A[1], P[2] - A[2]};
    const double d1 = dev_dot(ab, ap), d2 = dev_dot(ac, ap);
    region = kDevOnVertex;
    bool done = false;
    if (d1 <= 0.0 && d2 <= 0.0) {
        Q[0] = A[0], Q[1] = A[1], Q[2] = A[2];
        done = true;
    }
    double d3 = 0, d4 = 0, d5 = 0, d6 = 0, vc = 0, vb = 0;
    if (!done) {
        const double bp[3] = {P[0] - B[0], P[1] - B[1], P[2] - B[2]};
        d3 = dev_dot(ab, bp), d4 = dev_dot(ac, bp);
        if (d3 >= 0.0 && d4 <= d3) {
            Q[0] = B[0], Q[1] = B[1], Q[2] = B[2];
            done = true;
        }
    }
    if (!done) {
        vc = d1 * d4 - d3 * d2;
        if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
            const double v = d1 / (d1 - d3);
            Q[0] = A[0] + v * ab[0], Q[1] = A[1] + v * ab[1], Q[2] = A[2] + v * ab[2];
            region = kDevOnEdge;
            done = true;
        }
    }
    if (!done) {
        const double cp[3] = {P[0] - C[0], P[1] - C[1], P[2] - C[2]};
        d5 = dev_dot(ab, cp), d6 = dev_dot(ac, cp);
        if (d6 >= 0.0 && d5 <= d6) {
            Q[0] = C[0], Q[1] = C[1], Q[2] = C[2];
            done = true;
        }
    }
    if (!done) {
        vb = d5 * d2 - d1 * d6;
        if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
            const double w = d2 / (d2 - d6);
            Q[0] = A[0] + w * ac[0], Q[1] = A[1] + w * ac[1], Q[2] = A[2] + w * ac[2];
            region = kDevOnEdge;
            done = true;
        }
    }
    if (!done) {
        const double va = d3 * d6 - d5 * d4, e = d4 - d3, f = d5 - d6;
        if (va <= 0.0 && e >= 0.0 && f >= 0.0) {
            const double w = e / (e + f);
            Q[0] = B[0] + w * (C[0] - B[0]), Q[1] = B[1] + w * (C[1] - B[1]), Q[2] = B[2] + w * (C[2] - B[2]);
            region = kDevOnEdge;
        } else {
            const double s = (va + vb) + vc, v = vb / s, w = vc / s;
            Q[0] = (A[0] + v * ab[0]) + w * ac[0], Q[1] = (A[1] + v * ab[1]) + w * ac[1], Q[2] = (A[2] + v * ab[2]) + w * ac[2];
            region = 0u;
        }
    }
    const double r[3] = {P[0] - Q[0], P[1] - Q[1], P[2] - Q[2]};
    return dev_dot(r, r);
}

// One workgroup per brick that holds rows; a lane holds one row at a time.  The brick's triangles stream through LDS in tiles of
// `tile` (<= kDevTileMax) and every lane reads them as broadcasts, in ascending index order; a strict "smaller" keeps the first of
// equal dd.  The deviation record is written once per row; the summary is reduced per wave, then with vector atomics.
__global__ __launch_bounds__(256) void k_dev_rows(const Row* __restrict__ rows, const uint32_t* __restrict__ srow, const uint32_t* __restrict__ ub_start,
                                                  const uint32_t* __restrict__ tstart, const uint32_t* __restrict__ tend, const uint64_t* __restrict__ pairs,
                                                  const DevTri* __restrict__ recs, const double md2, const uint32_t tile, Deviation* __restrict__ out,
                                                  DevSummary* __restrict__ sum)
{
    __shared__ double s_tri[kDevTileMax * 12];
    __shared__ uint32_t s_idx[kDevTileMax];
    const uint32_t b = blockIdx.x;
    const uint32_t r0 = ub_start[b], r1 = ub_start[b + 1];
    const uint32_t t0 = tstart[b], t1 = tend[b];
    unsigned long long n_found = 0, n_neg = 0;
    long long sum_abs = 0, sum_sq = 0;
    uint32_t max_bits = 0;
    for (uint32_t rb = r0; rb < r1; rb += 256u) {
        const uint32_t r = rb + threadIdx.x;
        const bool have = r < r1;
        uint32_t row = 0;
        double P[3] = {0.0, 0.0, 0.0};
        if (have) {
            row = srow[r];
            P[0] = (double)rows[row].x, P[1] = (double)rows[row].y, P[2] = (double)rows[row].z;
        }
        bool found = false, neg = false;
        double best = 0.0, bq[3] = {0.0, 0.0, 0.0};
        uint32_t btri = 0, breg = 0;
        for (uint32_t tb = t0; tb < t1; tb += tile) {
            const uint32_t nt = min(tile, t1 - tb);
            __syncthreads();  // the previous tile is done with
            if (threadIdx.x < nt) s_idx[threadIdx.x] = (uint32_t)pairs[tb + threadIdx.x];
            __syncthreads();
            for (uint32_t e = threadIdx.x; e < nt * 12u; e += 256u) s_tri[e] = ((const double*)recs)[(uint64_t)s_idx[e / 12u] * 12u + e % 12u];
            __syncthreads();
            if (have) {
                for (uint32_t j = 0; j < nt; j++) {
                    double Q[3];
                    uint32_t region;
                    const double dd = dev_closest(P, &s_tri[j * 12u], Q, region);
                    if (dd <= md2 && (!found || dd < best)) {
                        const double* N = &s_tri[j * 12u + 9u];
                        const double rr[3] = {P[0] - Q[0], P[1] - Q[1], P[2] - Q[2]};
                        found = true, best = dd, btri = s_idx[j], breg = region, neg = dev_dot(N, rr) < 0.0;
                        bq[0] = Q[0], bq[1] = Q[1], bq[2] = Q[2];
                    }
                }
            }
        }
        if (have) {
            Deviation d;
            if (found) {
                d.distance = (float)sqrt(best);
                d.signed_distance = neg ? -d.distance : d.distance;
                d.tri = btri, d.flags = kDevFound | breg;
                d.q[0] = (float)bq[0], d.q[1] = (float)bq[1], d.q[2] = (float)bq[2];
                const double w = (double)d.distance;
                n_found++;
                n_neg += d.signed_distance < 0.f ? 1u : 0u;
                max_bits = max(max_bits, __float_as_uint(d.distance));
                sum_abs += llrint(w * 0x1p30);
                sum_sq += llrint((w * w) * 0x1p30);
            } else {
                d.distance = d.signed_distance = d.q[0] = d.q[1] = d.q[2] = __uint_as_float(0x7FC00000u);
                d.tri = 0xFFFFFFFFu, d.flags = 0u;
            }
            d.reserved = 0u;
            out[row] = d;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        n_found += __shfl_down(n_found, o);
        n_neg += __shfl_down(n_neg, o);
        sum_abs += __shfl_down(sum_abs, o);
        sum_sq += __shfl_down(sum_sq, o);
        max_bits = max(max_bits, __shfl_down(max_bits, o));
    }
    if ((threadIdx.x & 63u) == 0 && n_found) {
        atomicAdd(&sum->n_found, n_found);
        if (n_neg) atomicAdd(&sum->n_negative, n_neg);
        atomicAdd((unsigned long long*)&sum->sum_abs_q30, (unsigned long long)sum_abs);
        atomicAdd((unsigned long long*)&sum->sum_sq_q30, (unsigned long long)sum_sq);
        atomicMax(&sum->max_abs_bits, max_bits);
    }
}


// ---- best-fitting a mesh to the model (hfpf_align_mesh*; contract in include/hfpf.h, numpy restatement tests/align_ref.py) --------------
// Mesh-to-model point-to-plane ICP: per iteration compare's mesh kernels give every row its deviation record at the estimate T_k,
// one launch of k_align_reduce sums the 6x6 normal equations of the sampled rows from those records, and the host solves them as a
// track does.  The terms, their scales and the headroom are track's, so the sums are exact and do not depend on scheduling.
constexpr int kAlignTerms = 29;  // 21 J_i J_j (i <= j, i outer), 6 J_i r, r r, inliers: the first 29 of kTrackTerms
constexpr uint32_t kAlignSkipBoundary = 1u;  // = HFPF_ALIGN_SKIP_BOUNDARY

struct AlignParams {
    double c[3];     // the centre the twist is taken about: the middle of the bounding box
    uint32_t flags;  // HFPF_ALIGN_*
    uint32_t stride; // row j is sampled iff j % stride == 0
    uint32_t n;      // sampled rows: sample s is row s * stride
};

// One sampled row per thread, grid-stride over at most kTrackMaxBlocks blocks.  The row's point and normal come in through
// row_point_normal, its deviation record as two 16-byte loads.  Each thread keeps its 29 sums in registers (icp_accumulate);
// icp_block_reduce adds them to acc.
__global__ __launch_bounds__(256) void k_align_reduce(const AlignParams p, const Row* __restrict__ rows, const Deviation* __restrict__ dev,
                                                      unsigned long long* __restrict__ acc)
{
    IcpSums<kAlignTerms> sum;
#pragma unroll
    for (int k = 0; k < kAlignTerms; k++) sum.v[k] = 0;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < p.n; s += gridDim.x * blockDim.x) {
        const uint32_t j = s * p.stride;  // < the row count, which is below 2^32 - 1
        const uint4 d0 = *reinterpret_cast<const uint4*>(&dev[j].signed_distance);  // signed_distance, distance, tri, flags
        const uint32_t flags = d0.w;
        if (!(flags & kDevFound)) continue;
        if ((p.flags & kAlignSkipBoundary) && (flags & (kDevOnEdge | kDevOnVertex))) continue;
        const float4 d1 = *reinterpret_cast<const float4*>(&dev[j].q[0]);  // q, reserved
        const RowPN m = row_point_normal(rows[j]);
        if (!(((m.nx * m.nx + m.ny * m.ny) + m.nz * m.nz) <= 2.0)) continue;
        const double qx = d1.x, qy = d1.y, qz = d1.z;
        sum = icp_accumulate(sum, qx - p.c[0], qy - p.c[1], qz - p.c[2], m.nx, m.ny, m.nz, qx - m.x, qy - m.y, qz - m.z);
    }
    icp_block_reduce(sum, acc);
}


// ---- coverage of a triangle mesh by the model (hfpf_cover_mesh*; contract in include/hfpf.h, numpy restatement tests/cover_ref.py) -----
// A triangle holds 1 to 4096 samples, so the work is laid out per SAMPLE: k_cov_setup gives every triangle its record, its geometry
// and its sample count, an exclusive scan turns the counts into offsets, and k_cov_samples runs one lane per sample, whatever the
// mix of triangle sizes.  A sample is a query (voxel_coords, valid_point, window_nearest: k_query's own calls); the per-triangle
// counts are summed over the runs of equal triangle inside a wave and then with integer atomics, so nothing depends on the order.
struct TriCoverage {  // = hfpf_tri_coverage; max_distance as the bits of a non-negative float, which order as the floats do
    uint32_t n_samples, n_in_bbox, n_covered, flags;
    float area;
    uint32_t max_distance_bits;
    long long sum_dist_q30;
};
static_assert(sizeof(TriCoverage) == 32, "coverage record is 32 bytes");

struct CovSummary {  // = hfpf_coverage_summary, max_distance as bits
    unsigned long long n_tris_valid, n_tris_invalid, n_tris_huge, n_samples, n_in_bbox, n_covered;
    long long sum_dist_q30;
    unsigned long long area_q40_lo, area_q40_hi, covered_q40_lo, covered_q40_hi;
    uint32_t max_distance_bits, pad;
};
static_assert(sizeof(CovSummary) == 96, "coverage summary is 96 bytes");

struct CovTri {  // a valid triangle as k_cov_samples reads it
    double A[3], ab[3], ac[3], N[3];
    double s;  // sqrt(NN)
    uint32_t n, pad;
};
static_assert(sizeof(CovTri) == 112, "sampled triangle is 112 bytes");

struct CovParams {
    double spacing;
    double min_count;  // max(1, min_count)
    double max_d2;     // max_distance * max_distance
    double min_dot;    // min_normal_dot; -2 = gate off
    uint64_t n_verts;
    uint32_t n_tris, max_sub;
    uint32_t abs_normal;  // HFPF_COVER_ABS_NORMAL
    int32_t radius;
};

constexpr uint32_t kCovValid = 1u, kCovCapped = 2u, kCovHuge = 4u;

// One thread per triangle, and one more that zeroes the scan's extra element: the record (all zero for an invalid triangle), the
// geometry and count[k] = n^2 (0 for an invalid one).  total += the counts, as 64 bits: the u32 scan cannot say that it overflowed.
__global__ __launch_bounds__(256) void k_cov_setup(const CovParams p, const uint32_t* __restrict__ tris, const double* __restrict__ V,
                                                   TriCoverage* __restrict__ cov, CovTri* __restrict__ geo, uint32_t* __restrict__ count,
                                                   unsigned long long* __restrict__ total)
{
    const uint64_t kk = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    unsigned long long mine = 0;
    if (kk < p.n_tris) {
        const uint32_t k = (uint32_t)kk;
        DevTri tr;
        double ab[3], ac[3], NN = 0.0, L2 = 0.0;
        TriCoverage c{};
        if (dev_tri_valid(p.n_verts, tris, V, k, tr, ab, ac, NN, L2)) {
            const double q = sqrt(L2) / p.spacing;
            const uint32_t n = !(q > 1.0) ? 1u : q >= (double)p.max_sub ? p.max_sub : (uint32_t)ceil(q);
            const double s = sqrt(NN), area_d = 0.5 * s;
            c.n_samples = n * n;
            c.flags = kCovValid | (q > (double)p.max_sub ? kCovCapped : 0u) | (!(area_d < 0x1p23) ? kCovHuge : 0u);
            c.area = (float)area_d;
            CovTri t;
#pragma unroll
            for (int a = 0; a < 3; a++) t.A[a] = tr.A[a], t.ab[a] = ab[a], t.ac[a] = ac[a], t.N[a] = tr.N[a];
            t.s = s, t.n = n, t.pad = 0;
            geo[k] = t;
        }
        cov[k] = c;
        count[k] = c.n_samples;
        mine = c.n_samples;
    } else if (kk == p.n_tris) {
        count[kk] = 0;
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(total, mine);
}

// One lane per sample g of `total` (offset = the exclusive scan of the counts, n_tris + 1 entries, the last one = total): its
// triangle k is the one with offset[k] <= g < offset[k + 1] -- triangles without samples have an empty range and are never found --,
// its sub-triangle the one numbered l = g - offset[k]: strip m = isqrt(l) holds i = n - 1 - m and 2 m + 1 sub-triangles, t = l - m^2
// of them has kind = t & 1 and j = t >> 1.  Lanes of a wave hold ascending k, so a run of equal k is a contiguous stretch of lanes:
// a segmented shuffle reduction leaves the run's sums in its first lane, which issues the atomics.
// Sample s_idx < total: its triangle k (the first with offset[k + 1] > s_idx; offset[n_tris] = total > s_idx) and its f32 point p.
// Shared by k_cov_samples and the plan kernels, which meet the same samples again.
__device__ __forceinline__ F3 cov_sample_point(const uint32_t* __restrict__ offset, const CovTri* __restrict__ geo, const uint32_t n_tris, const uint32_t s_idx,
                                               uint32_t& k)
{
    uint32_t lo = 0, hi = n_tris;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (offset[mid + 1] <= s_idx) lo = mid + 1;
        else hi = mid;
    }
    k = lo;
    const CovTri* tr = &geo[k];
    const uint32_t n = tr->n, l = s_idx - offset[k];  // l < n^2 <= 4096
    uint32_t m = (uint32_t)sqrtf((float)l);
    m -= m * m > l ? 1u : 0u;
    m += (m + 1u) * (m + 1u) <= l ? 1u : 0u;
    const uint32_t tt = l - m * m, kind = tt & 1u, i = n - 1u - m, j = tt >> 1;
    const double v = (double)(3u * i + 1u + kind) / (double)(3u * n), w = (double)(3u * j + 1u + kind) / (double)(3u * n);
    F3 q;
    q.x = (float)((tr->A[0] + v * tr->ab[0]) + w * tr->ac[0]);
    q.y = (float)((tr->A[1] + v * tr->ab[1]) + w * tr->ac[1]);
    q.z = (float)((tr->A[2] + v * tr->ab[2]) + w * tr->ac[2]);
    return q;
}

// EMIT (hfpf_plan_views*): target[s] = 1 for a sample that is IN_BBOX and not COVERED, else 0.  Without it `target` is not touched.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_cov_samples(const GridParams g, const Tables t, const CovParams p, const uint32_t* __restrict__ offset,
                                                     const CovTri* __restrict__ geo, const uint32_t total, TriCoverage* __restrict__ cov,
                                                     uint32_t* __restrict__ target)
{
    const uint64_t gg = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool live = gg < total;
    uint32_t k = 0xFFFFFFFFu;  // a dead lane: a run of its own that adds nothing
    uint32_t in_bbox = 0, covered = 0, dist_bits = 0;
    long long sum_dist = 0;
    if (live) {
        const F3 q = cov_sample_point(offset, geo, p.n_tris, (uint32_t)gg, k);
        const CovTri* tr = &geo[k];
        if (__builtin_isfinite(q.x) && __builtin_isfinite(q.y) && __builtin_isfinite(q.z) && valid_point(g, q)) {  // USED, then IN_BBOX: k_query's tests
            in_bbox = 1u;
            int32_t vx[3];
            voxel_coords(g, q, vx[0], vx[1], vx[2]);
            const WindowNearest wn = window_nearest(g, t, q, vx, p.radius, p.min_count, p.max_d2);
            if (wn.found) {
                const double nx = t.nv_n[3 * (uint64_t)wn.nid], ny = t.nv_n[3 * (uint64_t)wn.nid + 1], nz = t.nv_n[3 * (uint64_t)wn.nid + 2];
                const double c = (tr->N[0] * nx + tr->N[1] * ny) + tr->N[2] * nz, bound = p.min_dot * tr->s;
                if (p.min_dot == -2.0 || c >= bound || (p.abs_normal && fabs(c) >= bound)) {
                    const float d = (float)sqrt(wn.d2);
                    covered = 1u;
                    dist_bits = __float_as_uint(d);
                    sum_dist = llrint((double)d * 0x1p30);
                }
            }
        }
        if (EMIT) target[gg] = in_bbox & ~covered;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t k2 = __shfl_down(k, o);
        const uint32_t b2 = __shfl_down(in_bbox, o), c2 = __shfl_down(covered, o), d2 = __shfl_down(dist_bits, o);
        const long long s2 = __shfl_down(sum_dist, o);
        if (lane + o < 64u && k2 == k) in_bbox += b2, covered += c2, dist_bits = max(dist_bits, d2), sum_dist += s2;
    }
    const uint32_t k_prev = __shfl_up(k, 1);
    if (!live || (lane != 0 && k_prev == k)) return;  // not the first lane of a run
    TriCoverage* c = &cov[k];
    if (in_bbox) atomicAdd(&c->n_in_bbox, in_bbox);
    if (covered) {
        atomicAdd(&c->n_covered, covered);
        atomicAdd((unsigned long long*)&c->sum_dist_q30, (unsigned long long)sum_dist);
        atomicMax(&c->max_distance_bits, dist_bits);
    }
}

// One thread per triangle: its share of the summary, reduced per wave, then u64 adds and a u32 max on the distance's bits.
__global__ __launch_bounds__(256) void k_cov_finish(const uint32_t n_tris, const TriCoverage* __restrict__ cov, const CovTri* __restrict__ geo,
                                                    CovSummary* __restrict__ sum)
{
    const uint64_t kk = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    unsigned long long w[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // the summary's 64-bit words in order
    uint32_t bits = 0;
    if (kk < n_tris) {
        const TriCoverage c = cov[kk];
        if (c.flags & kCovValid) {
            w[0] = 1, w[3] = c.n_samples, w[4] = c.n_in_bbox, w[5] = c.n_covered, w[6] = (unsigned long long)c.sum_dist_q30;
            bits = c.max_distance_bits;
            if (c.flags & kCovHuge) {
                w[2] = 1;
            } else {
                const double area_d = 0.5 * geo[kk].s;
                const unsigned long long ta = (unsigned long long)rint(area_d * 0x1p40);
                const unsigned long long tc = (unsigned long long)rint(((area_d * (double)c.n_covered) / (double)c.n_samples) * 0x1p40);
                w[7] = ta & 0xFFFFFFFFull, w[8] = ta >> 32, w[9] = tc & 0xFFFFFFFFull, w[10] = tc >> 32;
            }
        } else {
            w[1] = 1;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int i = 0; i < 11; i++) w[i] += __shfl_down(w[i], o);
        bits = max(bits, __shfl_down(bits, o));
    }
    if ((threadIdx.x & 63u) != 0) return;
    unsigned long long* out = &sum->n_tris_valid;
#pragma unroll
    for (int i = 0; i < 11; i++)
        if (w[i]) atomicAdd(&out[i], w[i]);
    if (bits) atomicMax(&sum->max_distance_bits, bits);
}


// ---- view planning (hfpf_plan_views*; contract in include/hfpf.h, numpy restatement tests/plan_ref.py) -----------------------------
// The cover kernels above mark the TARGETS (k_cov_samples<true>); a scan of the marks numbers them and k_plan_compact stores each
// target's point, triangle and weight.  Per chunk of at most 64 views: every sample of the mesh (k_plan_splat_samples) and, on
// request, every drawn row of the model (k_plan_splat_rows) is an occluder in a 32-bit depth buffer -- the bits of a positive f32
// order as integers, so the pixel's nearest depth is an atomicMin that does not depend on the order --, then k_plan_visible runs one
// lane per (target, view): a wave's ballot is one 64-bit word of the view's visibility bitset.  The greedy rounds (k_plan_gain,
// k_plan_argmax, k_plan_take) are enqueued without a host wait; a device-side `done` word makes the rounds behind the last useful
// one fall through.  Everything summed is an integer, so nothing depends on scheduling or on the chunking of the views.
struct PlanScore {  // = hfpf_view_score
    int32_t rank;
    uint32_t n_in_view, n_facing, n_visible;
    unsigned long long visible_q40, gain_q40, gain_samples;
};
static_assert(sizeof(PlanScore) == 40, "view score is 40 bytes");

struct TriPlan {  // = hfpf_tri_plan
    uint32_t n_targets, n_reachable, n_planned, flags;
};
static_assert(sizeof(TriPlan) == 16, "triangle plan record is 16 bytes");

struct PlanState {  // the words of one call, zeroed together
    unsigned long long n_reachable, n_planned, target_q40, reachable_q40, planned_q40;  // n_targets is the scan's total
    uint32_t done, best, n_selected, pad;
};

struct PlanParams {
    Pinhole cam;
    uint32_t n_views;      // views of this chunk
    uint32_t cull;         // HFPF_RENDER_CULL_BACKFACES, on the rows
    uint32_t two_sided;    // HFPF_PLAN_TWO_SIDED
    int32_t radius;        // >= 0 fixed, -1 auto
    int32_t max_radius;
    double occ_near;
    double r_num_samples;  // (0.5 * cover.spacing) * max(fx, fy)
    double r_num_rows;     // (0.5 * res) * max(fx, fy)
    double min_cos, tolerance, slope;
};

// One lane per sample of `total`, looping over the chunk's views (their poses in LDS, as in k_render_splat): every sample of a valid
// triangle with a finite point occludes, in the box or not, target or not.  A depth buffer word is the bits of (float)zc.
__global__ __launch_bounds__(256) void k_plan_splat_samples(const uint32_t* __restrict__ offset, const CovTri* __restrict__ geo, const uint32_t n_tris,
                                                            const uint32_t total, const double* __restrict__ poses, const PlanParams p,
                                                            uint32_t* __restrict__ zbuf)
{
    __shared__ double s_pose[kRenderChunkViews * 12];
    stage_poses(s_pose, poses, p.n_views);
    const uint64_t gg = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (gg >= total) return;
    uint32_t k;
    const F3 q = cov_sample_point(offset, geo, n_tris, (uint32_t)gg, k);
    if (!(__builtin_isfinite(q.x) && __builtin_isfinite(q.y) && __builtin_isfinite(q.z))) return;
    const uint64_t WH = (uint64_t)p.cam.width * p.cam.height;
    for (uint32_t v = 0; v < p.n_views; v++) {
        double dx, dy, dz, zc;
        int pu, pv;
        if (!view_project(&s_pose[12 * v], p.cam, p.occ_near, q.x, q.y, q.z, dx, dy, dz, zc, pu, pv)) continue;
        view_splat(zbuf + v * WH, p.cam, pu, pv, view_radius(p.radius, p.max_radius, p.r_num_samples, zc), __float_as_uint((float)zc));
    }
}

// HFPF_PLAN_MODEL_OCCLUDES: one lane per drawn row of the model, with the rows' own splat rule and the back-face cull of the view,
// between the halves of the projection as in k_render_splat.
__global__ __launch_bounds__(256) void k_plan_splat_rows(const Row* __restrict__ rows, const uint32_t n_rows, const double* __restrict__ poses,
                                                         const PlanParams p, uint32_t* __restrict__ zbuf)
{
    __shared__ double s_pose[kRenderChunkViews * 12];
    stage_poses(s_pose, poses, p.n_views);
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_rows) return;
    const RowPN q = row_point_normal(rows[j]);
    const uint64_t WH = (uint64_t)p.cam.width * p.cam.height;
    for (uint32_t v = 0; v < p.n_views; v++) {
        const double* T = &s_pose[12 * v];
        double dx, dy, dz, zc;
        int pu, pv;
        if (!view_depth(T, p.cam, p.occ_near, q.x, q.y, q.z, dx, dy, dz, zc)) continue;
        if (p.cull && !(((q.nx * dx + q.ny * dy) + q.nz * dz) < 0.0)) continue;
        if (!view_pixel(T, p.cam, dx, dy, dz, zc, pu, pv)) continue;
        view_splat(zbuf + v * WH, p.cam, pu, pv, view_radius(p.radius, p.max_radius, p.r_num_rows, zc), __float_as_uint((float)zc));
    }
}

// One lane per sample: a target stores its point with its triangle in the fourth word, and its weight, at its number toff[s].
__global__ __launch_bounds__(256) void k_plan_compact(const uint32_t* __restrict__ offset, const CovTri* __restrict__ geo, const uint32_t n_tris,
                                                      const uint32_t total, const uint32_t* __restrict__ target, const uint32_t* __restrict__ toff,
                                                      float4* __restrict__ tp, unsigned long long* __restrict__ tw)
{
    const uint64_t gg = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (gg >= total || !target[gg]) return;
    uint32_t k;
    const F3 q = cov_sample_point(offset, geo, n_tris, (uint32_t)gg, k);
    const uint32_t n = geo[k].n;
    const double area_d = 0.5 * geo[k].s;
    const uint32_t at = toff[gg];
    tp[at] = make_float4(q.x, q.y, q.z, __uint_as_float(k));
    tw[at] = !(area_d < 0x1p23) ? 0ull : (unsigned long long)rint((area_d / (double)(n * n)) * 0x1p40);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;  // in lane 0
}

// Grid (target tiles, views of the chunk): one lane per (target, view), a wave = 64 consecutive targets = one word of the view's
// bitset bits[(v0 + v) * n_words + word], stored by lane 0 with a plain store.  The counts are the ballots' popcounts, visible_q40 a
// wave sum: one integer atomic per wave, view and non-zero figure.  No lane leaves before the ballots.
__global__ __launch_bounds__(256) void k_plan_visible(const float4* __restrict__ tp, const unsigned long long* __restrict__ tw, const uint32_t n_targets,
                                                      const CovTri* __restrict__ geo, const double* __restrict__ poses, const PlanParams p,
                                                      const uint32_t* __restrict__ zbuf, const uint32_t v0, const uint64_t n_words,
                                                      unsigned long long* __restrict__ bits, PlanScore* __restrict__ score)
{
    const uint32_t v = blockIdx.y;
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const double* T = poses + 12ull * v;  // wave-uniform
    bool in_view = false, facing = false, visible = false;
    unsigned long long w = 0;
    if (i < n_targets) {
        const float4 q = tp[i];
        double dx, dy, dz, zc;
        int pu, pv;
        if (view_project(T, p.cam, p.cam.z_near, q.x, q.y, q.z, dx, dy, dz, zc, pu, pv) && view_inside(p.cam, pu, pv)) {
            in_view = true;
            const double* N = geo[__float_as_uint(q.w)].N;
            const double NN = dev_dot(N, N);
            const double c = -((N[0] * dx + N[1] * dy) + N[2] * dz), d2 = (dx * dx + dy * dy) + dz * dz;
            facing = p.min_cos < 0.0 || ((c > 0.0 || p.two_sided) && c * c >= ((p.min_cos * p.min_cos) * NN) * d2);
            if (facing) {
                const float depth32 = (float)zc;
                const float zmin = __uint_as_float(zbuf[v * ((uint64_t)p.cam.width * p.cam.height) + (uint64_t)pv * p.cam.width + (uint64_t)pu]);
                visible = (double)depth32 - (double)zmin <= p.tolerance + p.slope * zc;
                if (visible) w = tw[i];
            }
        }
    }
    const unsigned long long b_view = __ballot(in_view), b_face = __ballot(facing), b_vis = __ballot(visible);
    const unsigned long long sum_w = b_vis ? wave_sum_u64(w) : 0ull;  // (b_vis is wave-uniform)
    if ((threadIdx.x & 63u) != 0 || i >= n_targets) return;
    bits[(uint64_t)(v0 + v) * n_words + (i >> 6)] = b_vis;
    PlanScore* s = &score[v0 + v];
    if (b_view) atomicAdd(&s->n_in_view, (uint32_t)__popcll(b_view));
    if (b_face) atomicAdd(&s->n_facing, (uint32_t)__popcll(b_face));
    if (b_vis) {
        atomicAdd(&s->n_visible, (uint32_t)__popcll(b_vis));
        if (sum_w) atomicAdd(&s->visible_q40, sum_w);
    }
}

// remaining = every target: all ones, the last word cut to n_targets bits.  rank = -1 for every view.
__global__ __launch_bounds__(256) void k_plan_begin(const uint32_t n_targets, const uint64_t n_words, unsigned long long* __restrict__ remaining,
                                                    const uint32_t n_views, PlanScore* __restrict__ score)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n_words) remaining[i] = (i + 1 < n_words || (n_targets & 63u) == 0) ? ~0ull : (1ull << (n_targets & 63u)) - 1ull;
    if (i < n_views) score[i].rank = -1;
}

// Grid (target tiles, views): G(v) and C(v) of the views not yet selected, as u64 sums gain[2 v], gain[2 v + 1] (zero on entry:
// k_plan_argmax clears them behind its read).
__global__ __launch_bounds__(256) void k_plan_gain(const unsigned long long* __restrict__ tw, const uint32_t n_targets, const uint64_t n_words,
                                                   const unsigned long long* __restrict__ bits, const unsigned long long* __restrict__ remaining,
                                                   const PlanScore* __restrict__ score, const PlanState* __restrict__ st, unsigned long long* __restrict__ gain)
{
    const uint32_t v = blockIdx.y;
    if (st->done || score[v].rank >= 0) return;  // block-uniform
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t wi = (i >> 6) < n_words ? (i >> 6) : n_words - 1;  // wave-uniform; a wave beyond the targets reads the last word and adds nothing
    const unsigned long long word = i < n_targets ? bits[(uint64_t)v * n_words + wi] & remaining[wi] : 0ull;
    if (!__ballot(word != 0ull)) return;  // wave-uniform
    const unsigned long long w = (word >> (threadIdx.x & 63u)) & 1ull ? tw[i] : 0ull;
    const unsigned long long sum_w = wave_sum_u64(w);
    if ((threadIdx.x & 63u) != 0) return;
    if (sum_w) atomicAdd(&gain[2 * v], sum_w);
    atomicAdd(&gain[2 * v + 1], (unsigned long long)__popcll(word));
}

// One workgroup: the best unselected view of round `round` -- the largest G, then the larger C, then the smaller index --; below
// max(1, min_gain) the selection is done.
__global__ __launch_bounds__(256) void k_plan_argmax(const uint32_t round, const uint32_t n_views, const unsigned long long min_gain,
                                                     PlanScore* __restrict__ score, unsigned long long* __restrict__ gain, PlanState* __restrict__ st)
{
    __shared__ unsigned long long s_g[256], s_c[256];
    __shared__ uint32_t s_v[256];
    if (st->done) return;  // uniform: nobody has written it yet
    unsigned long long bg = 0, bc = 0;
    uint32_t bv = 0xFFFFFFFFu;
    for (uint32_t v = threadIdx.x; v < n_views; v += 256u) {  // ascending v per thread: a strict > keeps the smaller index
        if (score[v].rank >= 0) continue;
        const unsigned long long G = gain[2 * v], Cn = gain[2 * v + 1];
        gain[2 * v] = 0, gain[2 * v + 1] = 0;
        if (bv == 0xFFFFFFFFu || G > bg || (G == bg && Cn > bc)) bg = G, bc = Cn, bv = v;
    }
    s_g[threadIdx.x] = bg, s_c[threadIdx.x] = bc, s_v[threadIdx.x] = bv;
    __syncthreads();
    for (uint32_t o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            const unsigned long long g2 = s_g[threadIdx.x + o], c2 = s_c[threadIdx.x + o];
            const uint32_t v2 = s_v[threadIdx.x + o], v1 = s_v[threadIdx.x];
            const unsigned long long g1 = s_g[threadIdx.x], c1 = s_c[threadIdx.x];
            if (v2 != 0xFFFFFFFFu && (v1 == 0xFFFFFFFFu || g2 > g1 || (g2 == g1 && (c2 > c1 || (c2 == c1 && v2 < v1)))))
                s_g[threadIdx.x] = g2, s_c[threadIdx.x] = c2, s_v[threadIdx.x] = v2;
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const unsigned long long need = min_gain > 1ull ? min_gain : 1ull;
    if (s_v[0] == 0xFFFFFFFFu || s_g[0] < need) {
        st->done = 1u;
        return;
    }
    PlanScore* s = &score[s_v[0]];
    s->rank = (int32_t)round, s->gain_q40 = s_g[0], s->gain_samples = s_c[0];
    st->best = s_v[0], st->n_selected = round + 1u;
}

// R_{k+1} = R_k \ VIS(best).
__global__ __launch_bounds__(256) void k_plan_take(const uint64_t n_words, const unsigned long long* __restrict__ bits, unsigned long long* __restrict__ remaining,
                                                   const PlanState* __restrict__ st)
{
    if (st->done) return;
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n_words) remaining[i] &= ~bits[(uint64_t)st->best * n_words + i];
}

__global__ __launch_bounds__(256) void k_plan_tri_begin(const uint32_t n_tris, const TriCoverage* __restrict__ cov, TriPlan* __restrict__ plan)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k < n_tris) plan[k] = TriPlan{0u, 0u, 0u, cov[k].flags};
}

// One lane per target: reachable = its bit in the union of every view's bitset (the word is wave-uniform), planned = its bit has
// left `remaining`.  The triangle records (plan may be NULL) take one atomic per set figure, the totals one per wave.
__global__ __launch_bounds__(256) void k_plan_finish(const float4* __restrict__ tp, const unsigned long long* __restrict__ tw, const uint32_t n_targets,
                                                     const uint64_t n_words, const uint32_t n_views, const unsigned long long* __restrict__ bits,
                                                     const unsigned long long* __restrict__ remaining, TriPlan* __restrict__ plan, PlanState* __restrict__ st)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool live = i < n_targets;
    const uint64_t wi = (i >> 6) < n_words ? (i >> 6) : n_words - 1;
    unsigned long long any = 0;
    for (uint32_t v = 0; v < n_views; v++) any |= bits[(uint64_t)v * n_words + wi];
    const unsigned long long lane_bit = 1ull << (threadIdx.x & 63u);
    const bool reach = live && (any & lane_bit), planned = live && !(remaining[wi] & lane_bit);
    const unsigned long long w = live ? tw[i] : 0ull;
    if (live && plan) {
        TriPlan* t = &plan[__float_as_uint(tp[i].w)];
        atomicAdd(&t->n_targets, 1u);
        if (reach) atomicAdd(&t->n_reachable, 1u);
        if (planned) atomicAdd(&t->n_planned, 1u);
    }
    const unsigned long long b_reach = __ballot(reach), b_plan = __ballot(planned);
    const unsigned long long s_all = wave_sum_u64(w), s_reach = wave_sum_u64(reach ? w : 0ull), s_plan = wave_sum_u64(planned ? w : 0ull);
    if ((threadIdx.x & 63u) != 0) return;
    if (b_reach) atomicAdd(&st->n_reachable, (unsigned long long)__popcll(b_reach));
    if (b_plan) atomicAdd(&st->n_planned, (unsigned long long)__popcll(b_plan));
    if (s_all) atomicAdd(&st->target_q40, s_all);
    if (s_reach) atomicAdd(&st->reachable_q40, s_reach);
    if (s_plan) atomicAdd(&st->planned_q40, s_plan);
}


// ---- depth consistency (hfpf_depth_consistency*, include/hfpf.h) ---------------------------------------------------------
// The inverse of the splat: per (row, frame) one depth pixel (or a window of them) is gathered where k_render_splat scatters a row.
// The grid is (row tiles) x (frame chunks, plan_consistency in host_plan.hpp); the depth pointer, the frame stride, the
// intrinsics and the loop over the chunk's frames are wave-uniform, only the pixel address is per lane.
struct ConsRec {  // = hfpf_row_consistency
    uint32_t n_in_view, n_tested, n_support, n_through, n_occluded, first_through, flags, reserved;
};
static_assert(sizeof(ConsRec) == 32, "a consistency record is 32 bytes");
struct ConsSummary {  // = hfpf_consistency_summary
    unsigned long long n_rows, n_seen, n_supported, n_contradicted, n_kept, pairs_tested, pairs_support, pairs_through;
};
constexpr uint32_t kConsSeen = 1u, kConsSupported = 2u, kConsContradicted = 4u, kConsNone = 0xFFFFFFFFu;

struct ConsParams {
    const uint8_t* depth;   // frame 0 of this span
    uint64_t frame_stride;  // bytes between two frames
    uint32_t depth_step, depth_f32;
    uint32_t n_frames;      // frames of this span
    uint32_t per_chunk;     // frames per chunk (<= kConsChunkFrames)
    uint32_t chunk0;        // first chunk of this launch
    uint32_t frame_base;    // index of the span's frame 0 in the call: what first_through counts from
    uint32_t plain;         // one launch of one chunk covers the call: plain stores of whole records, no atomics
    uint32_t gate;          // min_cos >= 0
    int32_t window;
    float unit;             // (float)depth_scale
    Pinhole cam;            // the depth images' intrinsics and size, the call's z range
    double tolerance, slope, min_cos2;
    // what k_cons_finish reads
    double through_ratio;
    uint32_t min_through;   // max(1, min_through)
    uint32_t drop;
};

// Every record of a call that accumulates with atomics (and of one without frames): zero counters, first_through = none.
__global__ __launch_bounds__(256) void k_cons_init(const uint32_t n_rows, ConsRec* __restrict__ recs)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_rows) return;
    uint4* r = reinterpret_cast<uint4*>(&recs[j]);
    r[0] = make_uint4(0u, 0u, 0u, 0u);
    r[1] = make_uint4(0u, kConsNone, 0u, 0u);
}

// One thread per row, looping over its chunk's frames with the five counters and first_through in registers.  `poses`: the span's.
__global__ __launch_bounds__(256) void k_consistency(const Row* __restrict__ rows, const uint32_t n_rows, const double* __restrict__ poses,
                                                     const ConsParams p, ConsRec* __restrict__ recs)
{
    __shared__ double s_pose[kConsChunkFrames * 12];
    const uint32_t f0 = (p.chunk0 + blockIdx.y) * p.per_chunk;  // < p.n_frames: the host launches no empty chunk
    const uint32_t nf = min(p.per_chunk, p.n_frames - f0);
    stage_poses(s_pose, poses + 12ull * f0, nf);
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_rows) return;
    const RowPN q = row_point_normal(rows[j]);
    uint32_t n_in_view = 0, n_tested = 0, n_support = 0, n_through = 0, n_occluded = 0, first_through = kConsNone;
    const int W = (int)p.cam.width, H = (int)p.cam.height, win = p.window;
    for (uint32_t f = 0; f < nf; f++) {
        double dx, dy, dz, zc;
        int pu, pv;
        const double* T = &s_pose[12 * f];
        if (!view_depth(T, p.cam, p.cam.z_near, q.x, q.y, q.z, dx, dy, dz, zc)) continue;
        if (!view_pixel(T, p.cam, dx, dy, dz, zc, pu, pv)) continue;
        if (!view_inside(p.cam, pu, pv)) continue;
        n_in_view++;
        if (p.gate) {
            const double c = -((q.nx * dx + q.ny * dy) + q.nz * dz), d2 = (dx * dx + dy * dy) + dz * dz;
            if (!(c > 0.0 && c * c >= p.min_cos2 * d2)) continue;
        }
        n_tested++;
        const double tol = p.tolerance + p.slope * zc;
        const uint8_t* img = p.depth + (uint64_t)(f0 + f) * p.frame_stride;  // wave-uniform
        const int x0 = max(pu - win, 0), x1 = min(pu + win, W - 1), y0 = max(pv - win, 0), y1 = min(pv + win, H - 1);
        bool support = false, any = false, occluded = false;
        for (int py = y0; py <= y1 && !support; py++) {
            const uint8_t* line = img + (uint64_t)py * p.depth_step;
            for (int px = x0; px <= x1; px++) {
                double zd;
                if (p.depth_f32) {
                    const float d = reinterpret_cast<const float*>(line)[px];
                    if (!__builtin_isfinite(d)) continue;
                    zd = (double)d;
                } else {
                    const uint16_t d = reinterpret_cast<const uint16_t*>(line)[px];
                    if (d == 0) continue;
                    zd = (double)((float)d * p.unit);
                }
                const double g = zd - zc;
                if (fabs(g) <= tol) {  // rule 1 wins whatever else the window holds: leaving here is exact
                    support = true;
                    break;
                }
                any = true;
                occluded = occluded || g < -tol;
            }
        }
        if (support) {
            n_support++;
        } else if (any) {
            if (occluded) {
                n_occluded++;
            } else {
                n_through++;
                first_through = min(first_through, p.frame_base + f0 + f);
            }
        }
    }
    ConsRec* r = &recs[j];
    if (p.plain) {
        uint4* o = reinterpret_cast<uint4*>(r);
        o[0] = make_uint4(n_in_view, n_tested, n_support, n_through);
        o[1] = make_uint4(n_occluded, first_through, 0u, 0u);
        return;
    }
    if (n_in_view) atomicAdd(&r->n_in_view, n_in_view);
    if (n_tested) atomicAdd(&r->n_tested, n_tested);
    if (n_support) atomicAdd(&r->n_support, n_support);
    if (n_through) atomicAdd(&r->n_through, n_through);
    if (n_occluded) atomicAdd(&r->n_occluded, n_occluded);
    if (first_through != kConsNone) atomicMin(&r->first_through, first_through);
}

// One thread per row (n_rows + 1 entries of keep, the last one 0 for the scan): the record's flags, the keep mark, and the row's
// share of the summary, reduced per wave, then u64 adds.
__global__ __launch_bounds__(256) void k_cons_finish(const uint32_t n_rows, const ConsParams p, ConsRec* __restrict__ recs, uint32_t* __restrict__ keep,
                                                     ConsSummary* __restrict__ sum)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    unsigned long long w[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the summary's words in order
    if (j < n_rows) {
        const ConsRec r = recs[j];
        const bool contra = r.n_through >= p.min_through && (double)r.n_through > p.through_ratio * (double)r.n_support;
        const uint32_t flags = (r.n_tested ? kConsSeen : 0u) | (r.n_support ? kConsSupported : 0u) | (contra ? kConsContradicted : 0u);
        recs[j].flags = flags;
        keep[j] = (p.drop && contra) ? 0u : 1u;
        w[0] = 1, w[1] = r.n_tested ? 1 : 0, w[2] = r.n_support ? 1 : 0, w[3] = contra ? 1 : 0, w[4] = contra ? 0 : 1;
        w[5] = r.n_tested, w[6] = r.n_support, w[7] = r.n_through;
    } else if (j == n_rows) {
        keep[j] = 0u;
    }
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] += __shfl_down(w[i], o);
    }
    if ((threadIdx.x & 63u) != 0) return;
    unsigned long long* out = &sum->n_rows;
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (w[i]) atomicAdd(&out[i], w[i]);
}

// HFPF_CONSISTENCY_DROP: kept rows (out_rows may be null) and their records at base[j], the scan of keep.
__global__ __launch_bounds__(256) void k_cons_compact(const Row* __restrict__ rows, const uint32_t n_rows, const ConsRec* __restrict__ recs,
                                                      const uint32_t* __restrict__ keep, const uint32_t* __restrict__ base,
                                                      Row* __restrict__ out_rows, ConsRec* __restrict__ out_recs)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_rows || !keep[j]) return;
    const uint32_t o = base[j];
    if (out_rows) out_rows[o] = rows[j];
    out_recs[o] = recs[j];
}

// ---- planar sections of a mesh (hfpf_section_mesh*; contract in include/hfpf.h, numpy restatement tests/section_ref.py) --------------
// k_dev_verts transforms the vertices.  k_section meets every triangle with a chunk of planes, first to count the crossings per
// plane, then to append them: a 64-bit segment key (plane | triangle), the append position as the sort's value, and the keys of the
// two points in segment orientation.  The sort of the segment keys gives the (plane, triangle) order whatever the append order was;
// the sort and unique of the point keys number the points; k_sec_points computes a point from its key alone; k_sec_link finds a
// segment's two points by binary search, counts the degrees and unites the two in comp_unite's forest (a contour's root is its
// smallest point); k_comp_flatten and a scan of the root flags number the contours; k_sec_label, k_sec_measure and k_sec_finish are
// the reductions per point, per segment and per contour.  Integer atomics only: nothing depends on the schedule.
struct SecPoint {  // = hfpf_section_point
    float x, y, z;
    uint32_t plane, va, vb, contour, ends;
};
struct SecSegment {  // = hfpf_section_segment
    uint32_t p0, p1, tri, contour;
};
struct __attribute__((aligned(8))) SecContour {  // = hfpf_section_contour
    uint32_t plane, first_point, n_points, n_segments, n_ends, flags;
    long long length_q32, area_q28;
    unsigned long long reserved;
};
struct __attribute__((aligned(8))) SecPlane {  // = hfpf_section_plane (the three first_* words are the host's prefix sums)
    uint32_t first_segment, n_segments, first_point, n_points, first_contour, n_contours, n_closed, n_branched;
    long long length_q32, area_q28;
    unsigned long long reserved[2];
};
struct SecCounters {  // zeroed in front of the count pass
    unsigned long long n_valid, n_invalid, n_far, n_closed;
};
static_assert(sizeof(SecPoint) == 32 && sizeof(SecSegment) == 16 && sizeof(SecContour) == 48 && sizeof(SecPlane) == 64, "the section records");

constexpr uint32_t kSecClosed = 1u, kSecBranched = 2u;
constexpr uint32_t kSecOpenMark = 0x80000000u;  // a contour's flags between k_sec_label and k_sec_finish: some point is not (1 in, 1 out)
constexpr double kSecHeadroom = 32.0;           // metres about the box's centre: the IN RANGE rule

struct SecParams {
    double c[3];        // the centre of the bounding box
    uint64_t n_verts;
    uint32_t n_tris;
    uint32_t plane0, np;   // this chunk: its first plane and how many (0..kSecChunkPlanes)
    uint32_t count_tris;   // 1: this launch also counts the valid, invalid and far triangles (one launch per call)
    uint32_t n_total;      // EMIT: the segments of the call (the bound of every append)
};

// The IN RANGE rule of a valid triangle: each of its nine coordinates within kSecHeadroom of the box's centre c.
__device__ __forceinline__ bool sec_in_range(const DevTri& tr, const double (&c)[3])
{
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; a++) in = in && fabs(tr.A[a] - c[a]) < kSecHeadroom && fabs(tr.B[a] - c[a]) < kSecHeadroom && fabs(tr.C[a] - c[a]) < kSecHeadroom;
    return in;
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_section(const SecParams p, const uint32_t* __restrict__ tris, const double* __restrict__ V,
                                                 const double* __restrict__ planes, uint32_t* __restrict__ count, const uint32_t* __restrict__ first,
                                                 uint64_t* __restrict__ seg_key, uint32_t* __restrict__ seg_val, uint64_t* __restrict__ pt_key,
                                                 SecCounters* __restrict__ ctr)
{
    __shared__ double s_plane[kSecChunkPlanes * 4];
    for (uint32_t i = threadIdx.x; i < 4u * p.np; i += 256u) s_plane[i] = planes[4ull * p.plane0 + i];
    __syncthreads();
    const uint64_t k64 = (uint64_t)blockIdx.x * kSecTriTile + threadIdx.x;
    const bool live = k64 < p.n_tris;  // no lane leaves before the last ballot
    const uint32_t k = live ? (uint32_t)k64 : 0u;
    const unsigned lane = threadIdx.x & 63u;
    DevTri tr;
    bool valid = false, act = false;
    if (live) {
        double ab[3], ac[3], NN, L2;
        valid = dev_tri_valid(p.n_verts, tris, V, k, tr, ab, ac, NN, L2);
        act = valid && sec_in_range(tr, p.c);
    }
    if (!EMIT && p.count_tris) {
        const unsigned long long mv = __ballot(valid), mi = __ballot(live && !valid), mf = __ballot(valid && !act);
        if (lane == 0) {
            if (mv) atomicAdd(&ctr->n_valid, (unsigned long long)__popcll(mv));
            if (mi) atomicAdd(&ctr->n_invalid, (unsigned long long)__popcll(mi));
            if (mf) atomicAdd(&ctr->n_far, (unsigned long long)__popcll(mf));
        }
    }
    uint32_t idx[3] = {0u, 0u, 0u};
    if (EMIT && act) idx[0] = tris[3ull * k], idx[1] = tris[3ull * k + 1], idx[2] = tris[3ull * k + 2];
    for (uint32_t j = 0; j < p.np; j++) {
        const double* q = &s_plane[4u * j];
        uint32_t in_mask = 0u;
        if (act) {
            const double sa = dev_dot(q, tr.A) - q[3], sb = dev_dot(q, tr.B) - q[3], sc = dev_dot(q, tr.C) - q[3];
            in_mask = (sa < 0.0 ? 1u : 0u) | (sb < 0.0 ? 2u : 0u) | (sc < 0.0 ? 4u : 0u);
        }
        const bool cross = in_mask != 0u && in_mask != 7u;
        const unsigned long long m = __ballot(cross);
        if (m == 0ull) continue;  // wave-uniform
        const uint32_t plane = p.plane0 + j;
        const unsigned leader = (unsigned)__ffsll((long long)m) - 1u;
        uint32_t base = 0u;
        if (lane == leader) base = atomicAdd(&count[plane], (uint32_t)__popcll(m));  // one atomic per wave and plane
        if (!EMIT) continue;
        base = __shfl(base, (int)leader);
        if (!cross) continue;
        const uint64_t pos = (uint64_t)first[plane] + base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (pos >= p.n_total) continue;  // the count pass sized the arrays for exactly these appends
        const bool lone_in = __popc(in_mask) == 1;
        const uint32_t bit = lone_in ? in_mask : (in_mask ^ 7u);  // the vertex that differs from the other two
        const int L = bit == 1u ? 0 : (bit == 2u ? 1 : 2);
        const uint32_t vL = idx[L], vN = idx[(L + 1) % 3], vP = idx[(L + 2) % 3];
        const uint64_t k_prev = sec_point_key(plane, vP, vL), k_next = sec_point_key(plane, vL, vN);
        seg_key[pos] = sec_segment_key(plane, k);
        seg_val[pos] = (uint32_t)pos;
        pt_key[2ull * pos] = lone_in ? k_prev : k_next;
        pt_key[2ull * pos + 1] = lone_in ? k_next : k_prev;
    }
}

// One lane per unique point: P from its key alone, always from the lower index to the higher.  Also the point's entry in the forest
// and its two degree words.
__global__ __launch_bounds__(256) void k_sec_points(const uint64_t* __restrict__ ukeys, const uint32_t n_points, const double* __restrict__ planes,
                                                    const uint32_t n_planes, const double* __restrict__ V, const uint64_t n_verts, double* __restrict__ Pd,
                                                    uint32_t* __restrict__ parent, uint32_t* __restrict__ deg_out, uint32_t* __restrict__ deg_in)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_points) return;
    const uint64_t key = ukeys[i];
    const uint32_t plane = sec_key_plane(key), va = sec_key_va(key), vb = sec_key_vb(key);
    parent[i] = i;
    deg_out[i] = 0u;
    deg_in[i] = 0u;
    if (plane >= n_planes || va >= n_verts || vb >= n_verts) {  // no key the emit pass writes; nothing is loaded through such a key
        Pd[3ull * i] = Pd[3ull * i + 1] = Pd[3ull * i + 2] = 0.0;
        return;
    }
    const double* q = planes + 4ull * plane;
    const double* A = V + 3ull * va;
    const double* B = V + 3ull * vb;
    const double sa = dev_dot(q, A) - q[3], sb = dev_dot(q, B) - q[3];
    const double t = sa / (sa - sb);
#pragma unroll
    for (int a = 0; a < 3; a++) Pd[3ull * i + a] = A[a] + t * (B[a] - A[a]);
}

// The rank of `key` in the sorted, distinct ukeys[0, n): every key searched for is in the list.
__device__ __forceinline__ uint32_t sec_rank(const uint64_t* __restrict__ ukeys, const uint32_t n, const uint64_t key)
{
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ukeys[mid] < key) lo = mid + 1u;
        else hi = mid;
    }
    return lo < n ? lo : n - 1u;
}

// One lane per segment, in sorted order: its two points (seg_ends: p0 | p1 << 32), their degrees and their union.
__global__ __launch_bounds__(256) void k_sec_link(const uint32_t* __restrict__ val_sorted, const uint32_t n_segs, const uint64_t* __restrict__ pt_key,
                                                  const uint64_t* __restrict__ ukeys, const uint32_t n_points, uint64_t* __restrict__ seg_ends,
                                                  uint32_t* __restrict__ parent, uint32_t* __restrict__ deg_out, uint32_t* __restrict__ deg_in)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_segs) return;
    const uint32_t src = val_sorted[i];
    if (src >= n_segs) {  // (the values are a permutation of 0 .. n_segs - 1)
        seg_ends[i] = 0ull;
        return;
    }
    const uint32_t p0 = sec_rank(ukeys, n_points, pt_key[2ull * src]), p1 = sec_rank(ukeys, n_points, pt_key[2ull * src + 1]);
    seg_ends[i] = (uint64_t)p0 | ((uint64_t)p1 << 32);
    atomicAdd(&deg_out[p0], 1u);
    atomicAdd(&deg_in[p1], 1u);
    comp_unite(parent, p0, p1);
}

// One lane per point: its record, and its share of its contour's record (zeroed before).  A root writes the words nobody adds to.
// Points are in (plane, va, vb) order, so many waves hold one contour: such a wave reduces in registers first.
__global__ __launch_bounds__(256) void k_sec_label(const uint32_t* __restrict__ root, const uint32_t* __restrict__ cbase, const uint32_t n_points,
                                                   const uint64_t* __restrict__ ukeys, const double* __restrict__ Pd, const uint32_t* __restrict__ deg_out,
                                                   const uint32_t* __restrict__ deg_in, SecPoint* __restrict__ pts, SecContour* __restrict__ conts)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    const bool live = j < n_points;
    const uint32_t jj = live ? j : n_points - 1u;  // (n_points > 0) a dead lane mirrors the last point and adds nothing
    const uint32_t r = root[jj], c = cbase[r];
    const uint32_t n_out = deg_out[jj], n_in = deg_in[jj];
    if (live) {
        const uint64_t key = ukeys[j];
        pts[j] = SecPoint{(float)Pd[3ull * j], (float)Pd[3ull * j + 1], (float)Pd[3ull * j + 2], sec_key_plane(key), sec_key_va(key), sec_key_vb(key), c,
                          min(n_out, 65535u) | (min(n_in, 65535u) << 16)};
        if (r == j) conts[c].plane = sec_key_plane(key), conts[c].first_point = j;
    }
    uint32_t n = live ? 1u : 0u, ends = (live && n_in + n_out == 1u) ? 1u : 0u;
    uint32_t flags = !live ? 0u : ((n_in == 1u && n_out == 1u) ? 0u : kSecOpenMark) | ((n_in > 1u || n_out > 1u) ? kSecBranched : 0u);
    const bool uniform = __all(c == __shfl(c, 0));
    if (uniform) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            n += __shfl_down(n, o);
            ends += __shfl_down(ends, o);
            flags |= __shfl_down(flags, o);
        }
        if ((threadIdx.x & 63u) != 0) return;
    } else if (!live) {
        return;
    }
    SecContour* k = &conts[c];
    atomicAdd(&k->n_points, n);
    if (ends) atomicAdd(&k->n_ends, ends);
    if (flags) atomicOr(&k->flags, flags);
}

// One lane per segment: its record, and its terms of its contour's length and area about the representative's point.
__global__ __launch_bounds__(256) void k_sec_measure(const uint64_t* __restrict__ seg_sorted, const uint64_t* __restrict__ seg_ends, const uint32_t n_segs,
                                                     const double* __restrict__ planes, const SecPoint* __restrict__ pts, const double* __restrict__ Pd,
                                                     SecSegment* __restrict__ segs, SecContour* __restrict__ conts)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool live = i < n_segs;
    const uint32_t ii = live ? i : n_segs - 1u;  // (n_segs > 0)
    const uint64_t key = seg_sorted[ii], ends = seg_ends[ii];
    SecSegment s{(uint32_t)ends, (uint32_t)(ends >> 32), sec_seg_tri(key), 0u};
    const uint32_t c = pts[s.p0].contour;
    s.contour = c;
    if (live) segs[i] = s;
    const double* q = planes + 4ull * sec_seg_plane(key);
    const double* P0 = Pd + 3ull * s.p0;
    const double* P1 = Pd + 3ull * s.p1;
    const double* Pr = Pd + 3ull * conts[c].first_point;
    double e[3], a[3], b[3], U[3];
    const double root_nn = sqrt(dev_dot(q, q));
#pragma unroll
    for (int x = 0; x < 3; x++) e[x] = P1[x] - P0[x], a[x] = P0[x] - Pr[x], b[x] = P1[x] - Pr[x], U[x] = q[x] / root_nn;
    const double X[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    long long len = live ? (long long)rint(sqrt(dev_dot(e, e)) * 4294967296.0) : 0ll;
    long long area = live ? (long long)rint((0.5 * dev_dot(U, X)) * 268435456.0) : 0ll;
    uint32_t n = live ? 1u : 0u;
    const bool uniform = __all(c == __shfl(c, 0));
    if (uniform) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            n += __shfl_down(n, o);
            len += __shfl_down(len, o);
            area += __shfl_down(area, o);
        }
        if ((threadIdx.x & 63u) != 0) return;
    } else if (!live) {
        return;
    }
    SecContour* k = &conts[c];
    atomicAdd(&k->n_segments, n);
    atomicAdd((unsigned long long*)&k->length_q32, (unsigned long long)len);
    atomicAdd((unsigned long long*)&k->area_q28, (unsigned long long)area);
}

// One lane per contour: its final flags, and its share of its plane's record (zeroed before).
__global__ __launch_bounds__(256) void k_sec_finish(const uint32_t n_conts, SecContour* __restrict__ conts, SecPlane* __restrict__ recs,
                                                    unsigned long long* __restrict__ n_closed)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= n_conts) return;
    const SecContour k = conts[c];
    const bool closed = (k.flags & kSecOpenMark) == 0u, branched = (k.flags & kSecBranched) != 0u;
    conts[c].flags = (closed ? kSecClosed : 0u) | (branched ? kSecBranched : 0u);
    SecPlane* r = &recs[k.plane];
    atomicAdd(&r->n_segments, k.n_segments);
    atomicAdd(&r->n_points, k.n_points);
    atomicAdd(&r->n_contours, 1u);
    if (branched) atomicAdd(&r->n_branched, 1u);
    atomicAdd((unsigned long long*)&r->length_q32, (unsigned long long)k.length_q32);
    if (closed) {
        atomicAdd(&r->n_closed, 1u);
        atomicAdd((unsigned long long*)&r->area_q28, (unsigned long long)k.area_q28);
        atomicAdd(n_closed, 1ull);
    }
}

// ---- open edges of a mesh (hfpf_mesh_topology*; contract in include/hfpf.h, numpy restatement tests/topology_ref.py) ----------------
// The section's contour stage in vertex-index space.  k_dev_verts transforms the vertices.  k_top_emit writes a used triangle's three
// half-edges at slots 3k .. 3k + 2 (key: va | vb with the direction above the sorted bits; value: the slot), marks its vertices
// and unites them in the shells' forest (comp_unite: a shell's root is its smallest vertex).  The stable sort brings an edge's
// half-edges together in ascending id; k_top_classify has the lane at the start of each run walk it, count the two directions and, for
// a boundary edge, count the degrees of its ends and unite them in the loops' forest.  k_comp_flatten, k_top_mask and a scan of the
// root flags number shells and loops by ascending representative; a scan of the listed flags places the edge records.  Behind the one
// allocation of the results k_top_vertices, k_top_tris, k_top_edges, k_top_loops and k_top_finish are the reductions per vertex,
// triangle, edge, listed edge and record.  Integer atomics only: nothing depends on the schedule.  A mesh is mostly one shell, so
// every sum is first reduced over the wave's runs of lanes with the same label (top_run): one atomic per run, not per lane.
struct TopEdge {  // = hfpf_topology_edge
    uint32_t p0, p1, tri, kind, uses, loop, shell, reserved;
};
struct __attribute__((aligned(8))) TopLoop {  // = hfpf_topology_loop
    uint32_t first_vertex, n_verts, n_edges, n_ends, flags, shell;
    long long length_q32, area_q28[3];
    unsigned long long reserved;
};
struct __attribute__((aligned(8))) TopShell {  // = hfpf_topology_shell
    uint32_t first_vertex, n_verts, n_tris, flags, n_edges, n_boundary, n_nonmanifold, n_miswound, n_loops, reserved0;
    long long area_q32, volume_q40;
    unsigned long long reserved;
};
struct TopCounters {  // zeroed in front of the emit pass
    unsigned long long n_valid, n_invalid, n_far, n_verts_used, n_edges, n_interior, n_boundary, n_nonmanifold, n_miswound, n_closed_loops, n_watertight;
};
static_assert(sizeof(TopEdge) == 32 && sizeof(TopLoop) == 64 && sizeof(TopShell) == 64, "the topology records");

constexpr uint32_t kTopLoopClosed = 1u, kTopLoopBranched = 2u;
constexpr uint32_t kTopLoopOpenMark = 0x80000000u;  // a loop's flags between k_top_vertices and k_top_finish: some vertex is not (1 in, 1 out)
constexpr uint32_t kTopShellOpen = 1u, kTopShellNonManifold = 2u, kTopShellMiswound = 4u, kTopShellWatertight = 8u;

struct TopParams {
    double c[3];       // the centre of the bounding box
    uint64_t n_verts;
    uint32_t n_tris;
};

// The wave's lanes in runs of neighbours with the same label: `end` = the lane behind this lane's run, head = its first lane.  Every
// lane of the wave calls it.
struct TopRun {
    unsigned end;
    bool head;
};
__device__ __forceinline__ TopRun top_run(const uint32_t label, const unsigned lane)
{
    const uint32_t prev = __shfl_up(label, 1);
    const unsigned long long heads = __ballot(lane == 0u || prev != label);
    const unsigned long long above = heads & ~((2ull << lane) - 1ull);  // (lane 63: 2 << 63 is 0, the mask is empty)
    return TopRun{above ? (unsigned)__ffsll((long long)above) - 1u : 64u, ((heads >> lane) & 1ull) != 0ull};
}
// v summed over the lanes from this one to the end of its run: the head ends with the run's total.  After the step of offset o a
// lane holds the sum over [lane, min(lane + 2 o, end)).
template <typename T>
__device__ __forceinline__ T top_run_sum(T v, const TopRun r, const unsigned lane)
{
#pragma unroll
    for (unsigned o = 1; o < 64u; o <<= 1) {
        const T w = __shfl_down(v, o);
        if (lane + o < r.end) v += w;
    }
    return v;
}

// Every vertex a root of both forests, unused, without a boundary edge.
__global__ __launch_bounds__(256) void k_top_init(const uint64_t n_verts, uint32_t* __restrict__ parent_s, uint32_t* __restrict__ parent_l,
                                                  uint32_t* __restrict__ used, uint32_t* __restrict__ deg_out, uint32_t* __restrict__ deg_in)
{
    const uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (v >= n_verts) return;
    parent_s[v] = (uint32_t)v, parent_l[v] = (uint32_t)v;
    used[v] = 0u, deg_out[v] = 0u, deg_in[v] = 0u;
}

// One lane per triangle: its class (k_section's tests), its three half-edges or three skipped slots, its vertices' marks and union.
__global__ __launch_bounds__(256) void k_top_emit(const TopParams p, const uint32_t* __restrict__ tris, const double* __restrict__ V,
                                                  uint64_t* __restrict__ key, uint32_t* __restrict__ val, uint32_t* __restrict__ used,
                                                  uint32_t* __restrict__ parent, TopCounters* __restrict__ ctr)
{
    const uint64_t k64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool live = k64 < p.n_tris;  // no lane leaves before the ballots
    const uint32_t k = live ? (uint32_t)k64 : 0u;
    DevTri tr;
    bool valid = false, act = false;
    if (live) {
        double ab[3], ac[3], NN, L2;
        valid = dev_tri_valid(p.n_verts, tris, V, k, tr, ab, ac, NN, L2);
        act = valid && sec_in_range(tr, p.c);
    }
    const unsigned long long mv = __ballot(valid), mi = __ballot(live && !valid), mf = __ballot(valid && !act);
    if ((threadIdx.x & 63u) == 0u) {
        if (mv) atomicAdd(&ctr->n_valid, (unsigned long long)__popcll(mv));
        if (mi) atomicAdd(&ctr->n_invalid, (unsigned long long)__popcll(mi));
        if (mf) atomicAdd(&ctr->n_far, (unsigned long long)__popcll(mf));
    }
    if (!live) return;
    const uint64_t s = 3ull * k;
    val[s] = (uint32_t)s, val[s + 1] = (uint32_t)s + 1u, val[s + 2] = (uint32_t)s + 2u;
    if (!act) {
        key[s] = key[s + 1] = key[s + 2] = kTopSkipped;
        return;
    }
    const uint32_t i0 = tris[s], i1 = tris[s + 1], i2 = tris[s + 2];  // in range and distinct: the triangle is valid
    key[s] = top_edge_key(i0, i1), key[s + 1] = top_edge_key(i1, i2), key[s + 2] = top_edge_key(i2, i0);
    used[i0] = 1u, used[i1] = 1u, used[i2] = 1u;  // (every writer stores the same word)
    comp_unite(parent, i0, i1);
    comp_unite(parent, i0, i2);
}

// k_comp_flatten calls every vertex that is its own parent a root; a root counts only when the vertex takes part: a | b non-zero (b
// may be NULL).
__global__ __launch_bounds__(256) void k_top_mask(uint32_t* __restrict__ flag, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                  const uint64_t n_verts)
{
    const uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (v >= n_verts) return;
    if ((a[v] | (b ? b[v] : 0u)) == 0u) flag[v] = 0u;
}

// label[v] = the number of v's component (base = the exclusive scan of the root flags), kTopNone for a vertex that takes no part.
__global__ __launch_bounds__(256) void k_top_vlabel(const uint32_t* __restrict__ root, const uint32_t* __restrict__ base, const uint32_t* __restrict__ a,
                                                    const uint32_t* __restrict__ b, const uint64_t n_verts, uint32_t* __restrict__ label)
{
    const uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (v >= n_verts) return;
    label[v] = (a[v] | (b ? b[v] : 0u)) != 0u ? base[root[v]] : kTopNone;
}

// One lane per sorted half-edge of a used triangle (n_he of them; the skipped slots sort behind).  The first of a run walks it,
// however long it is: use[i] = the edge's saturated counts, listed[i] = 1 for an edge that is not INTERIOR (listed has n_he + 1
// entries, the last one 0 for the scan).  A boundary edge's ends get their degrees and their union.
__global__ __launch_bounds__(256) void k_top_classify(const uint64_t* __restrict__ key, const uint64_t n_he, uint32_t* __restrict__ use,
                                                      uint32_t* __restrict__ listed, uint32_t* __restrict__ parent, uint32_t* __restrict__ deg_out,
                                                      uint32_t* __restrict__ deg_in, TopCounters* __restrict__ ctr)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool live = i < n_he;  // no lane leaves before the ballots
    bool start = false;
    uint32_t kind = 0u;
    if (live) {
        const uint64_t e = key[i];
        start = e != kTopSkipped && (i == 0 || !top_same_edge(key[i - 1], e));
        if (start) {
            uint32_t n_fwd = 0u, n_bwd = 0u;
            for (uint64_t j = i; j < n_he; j++) {
                const uint64_t f = key[j];
                if (!top_same_edge(f, e)) break;
                if (f & kTopForward) n_fwd++;
                else n_bwd++;
            }
            kind = top_edge_kind(n_fwd, n_bwd);
            use[i] = top_edge_uses(n_fwd, n_bwd);
            if (kind == kTopBoundary) {
                const uint32_t p0 = n_fwd ? top_key_va(e) : top_key_vb(e), p1 = n_fwd ? top_key_vb(e) : top_key_va(e);
                atomicAdd(&deg_out[p0], 1u);
                atomicAdd(&deg_in[p1], 1u);
                comp_unite(parent, p0, p1);
            }
        } else {
            use[i] = 0u;
        }
        listed[i] = start && kind != 0u ? 1u : 0u;
    } else if (i == n_he) {
        listed[i] = 0u;
    }
    const unsigned long long me = __ballot(start), mb = __ballot(start && kind == kTopBoundary), mn = __ballot(start && kind == kTopNonManifold),
                             mm = __ballot(start && kind == kTopMiswound);
    if ((threadIdx.x & 63u) != 0u || me == 0ull) return;
    atomicAdd(&ctr->n_edges, (unsigned long long)__popcll(me));
    if (me & ~(mb | mn | mm)) atomicAdd(&ctr->n_interior, (unsigned long long)__popcll(me & ~(mb | mn | mm)));
    if (mb) atomicAdd(&ctr->n_boundary, (unsigned long long)__popcll(mb));
    if (mn) atomicAdd(&ctr->n_nonmanifold, (unsigned long long)__popcll(mn));
    if (mm) atomicAdd(&ctr->n_miswound, (unsigned long long)__popcll(mm));
}

// One lane per vertex: its share of its shell's and of its loop's record (both zeroed before).  A representative writes the words
// nobody adds to.
__global__ __launch_bounds__(256) void k_top_vertices(const uint64_t n_verts, const uint32_t* __restrict__ used, const uint32_t* __restrict__ vshell,
                                                      const uint32_t* __restrict__ vloop, const uint32_t* __restrict__ root_s,
                                                      const uint32_t* __restrict__ root_l, const uint32_t* __restrict__ deg_out,
                                                      const uint32_t* __restrict__ deg_in, TopShell* __restrict__ shells, const uint32_t n_shells,
                                                      TopLoop* __restrict__ loops, const uint32_t n_loops, TopCounters* __restrict__ ctr)
{
    const uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u;
    const bool live = v < n_verts;  // no lane leaves before the last shuffle
    const bool in_shell = live && used[v] != 0u;
    const uint32_t n_out = live ? deg_out[v] : 0u, n_in = live ? deg_in[v] : 0u;
    const bool on_rim = n_out + n_in != 0u;
    uint32_t s = in_shell ? vshell[v] : kTopNone, l = on_rim ? vloop[v] : kTopNone;
    if (s >= n_shells) s = kTopNone;
    if (l >= n_loops) l = kTopNone;
    if (s != kTopNone && root_s[v] == (uint32_t)v) shells[s].first_vertex = (uint32_t)v;
    if (l != kTopNone && root_l[v] == (uint32_t)v) loops[l].first_vertex = (uint32_t)v, loops[l].shell = s;
    const unsigned long long mu = __ballot(in_shell);
    if (lane == 0u && mu) atomicAdd(&ctr->n_verts_used, (unsigned long long)__popcll(mu));
    const TopRun rs = top_run(s, lane);
    const uint32_t nv = top_run_sum(s != kTopNone ? 1u : 0u, rs, lane);
    if (rs.head && s != kTopNone) atomicAdd(&shells[s].n_verts, nv);
    // a wave holds at most 64 of each: vertices | ends << 8 | not (1 in, 1 out) << 16 | branched << 24 in one word
    const uint32_t mine = l == kTopNone ? 0u : 1u | (n_in + n_out == 1u ? 1u << 8 : 0u) | (n_in == 1u && n_out == 1u ? 0u : 1u << 16) |
                                               (n_in > 1u || n_out > 1u ? 1u << 24 : 0u);
    const TopRun rl = top_run(l, lane);
    const uint32_t w = top_run_sum(mine, rl, lane);
    if (!rl.head || l == kTopNone) return;
    TopLoop* k = &loops[l];
    atomicAdd(&k->n_verts, w & 0xFFu);
    if ((w >> 8) & 0xFFu) atomicAdd(&k->n_ends, (w >> 8) & 0xFFu);
    const uint32_t flags = ((w >> 16) & 0xFFu ? kTopLoopOpenMark : 0u) | ((w >> 24) ? kTopLoopBranched : 0u);
    if (flags) atomicOr(&k->flags, flags);
}

// One lane per triangle: its shell (tri_shell, when wanted) and its terms of the shell's triangle count, area and volume about the
// representative's point (k_top_vertices has named it).
__global__ __launch_bounds__(256) void k_top_tris(const TopParams p, const uint32_t* __restrict__ tris, const double* __restrict__ V,
                                                  const uint32_t* __restrict__ vshell, TopShell* __restrict__ shells, const uint32_t n_shells,
                                                  uint32_t* __restrict__ tri_shell)
{
    const uint64_t k64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u;
    const bool live = k64 < p.n_tris;  // no lane leaves before the last shuffle
    const uint32_t k = live ? (uint32_t)k64 : 0u;
    DevTri tr;
    double NN = 0.0;
    bool act = false;
    if (live) {
        double ab[3], ac[3], L2;
        act = dev_tri_valid(p.n_verts, tris, V, k, tr, ab, ac, NN, L2) && sec_in_range(tr, p.c);
    }
    uint32_t s = act ? vshell[tris[3ull * k]] : kTopNone;
    if (s >= n_shells) s = kTopNone;
    if (live && tri_shell) tri_shell[k] = s;
    long long area = 0ll, volume = 0ll;
    if (s != kTopNone) {
        const double* Pr = V + 3ull * shells[s].first_vertex;
        double a[3], b[3], c[3];
#pragma unroll
        for (int x = 0; x < 3; x++) a[x] = tr.A[x] - Pr[x], b[x] = tr.B[x] - Pr[x], c[x] = tr.C[x] - Pr[x];
        const double X[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
        area = (long long)rint((0.5 * sqrt(NN)) * 4294967296.0);
        volume = (long long)rint((dev_dot(a, X) / 6.0) * 1099511627776.0);
    }
    const TopRun r = top_run(s, lane);
    const uint32_t n = top_run_sum(s != kTopNone ? 1u : 0u, r, lane);
    area = top_run_sum(area, r, lane);
    volume = top_run_sum(volume, r, lane);
    if (!r.head || s == kTopNone) return;
    TopShell* h = &shells[s];
    atomicAdd(&h->n_tris, n);
    atomicAdd((unsigned long long*)&h->area_q32, (unsigned long long)area);
    atomicAdd((unsigned long long*)&h->volume_q40, (unsigned long long)volume);
}

// One lane per sorted half-edge: the first of a run adds the edge to its shell's counts and writes the record of a listed edge at its
// place (base = the exclusive scan of the listed flags).  The other lanes of a run carry the shell's label and add nothing, so that
// the runs of a wave stay as long as the shell is.
__global__ __launch_bounds__(256) void k_top_edges(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val, const uint64_t n_he,
                                                   const uint32_t* __restrict__ use, const uint32_t* __restrict__ base, const uint32_t* __restrict__ vshell,
                                                   const uint32_t* __restrict__ vloop, const uint64_t n_verts, TopShell* __restrict__ shells,
                                                   const uint32_t n_shells, TopEdge* __restrict__ edges, const uint32_t n_listed)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u;
    const uint64_t e = i < n_he ? key[i] : kTopSkipped;  // no lane leaves before the last shuffle
    const uint32_t va = top_key_va(e), vb = top_key_vb(e);
    const bool real = e != kTopSkipped && vb < n_verts;  // (va < vb in every key the emit pass writes)
    const bool start = real && (i == 0 || !top_same_edge(key[i - 1], e));
    uint32_t s = real ? vshell[va] : kTopNone;
    if (s >= n_shells) s = kTopNone;
    uint32_t mine = 0u;  // a wave holds at most 64 of each: edges | boundary << 8 | non-manifold << 16 | miswound << 24 in one word
    if (start) {
        const uint32_t uses = use[i], kind = top_edge_kind(uses & 0xFFFFu, uses >> 16);
        mine = 1u | (kind == kTopBoundary ? 1u << 8 : 0u) | (kind == kTopNonManifold ? 1u << 16 : 0u) | (kind == kTopMiswound ? 1u << 24 : 0u);
        const uint32_t o = base[i];
        if (kind != 0u && o < n_listed) {
            const bool back = kind == kTopBoundary && !(e & kTopForward);
            edges[o] = TopEdge{back ? vb : va, back ? va : vb, val[i] / 3u, kind, uses, kind == kTopBoundary ? vloop[va] : kTopNone, s, 0u};
        }
    }
    const TopRun r = top_run(s, lane);
    const uint32_t w = top_run_sum(mine, r, lane);
    if (!r.head || s == kTopNone || w == 0u) return;
    TopShell* h = &shells[s];
    atomicAdd(&h->n_edges, w & 0xFFu);
    if ((w >> 8) & 0xFFu) atomicAdd(&h->n_boundary, (w >> 8) & 0xFFu);
    if ((w >> 16) & 0xFFu) atomicAdd(&h->n_nonmanifold, (w >> 16) & 0xFFu);
    if (w >> 24) atomicAdd(&h->n_miswound, w >> 24);
}

// One lane per listed edge: a boundary edge's terms of its loop's edge count, length and vector area about the representative's point.
__global__ __launch_bounds__(256) void k_top_loops(const TopEdge* __restrict__ edges, const uint32_t n_listed, const double* __restrict__ V,
                                                   const uint64_t n_verts, TopLoop* __restrict__ loops, const uint32_t n_loops)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u;
    uint32_t l = kTopNone, p0 = 0u, p1 = 0u;  // no lane leaves before the last shuffle
    if (i < n_listed) {
        const TopEdge e = edges[i];
        if (e.kind == kTopBoundary && e.loop < n_loops && e.p0 < n_verts && e.p1 < n_verts) l = e.loop, p0 = e.p0, p1 = e.p1;
    }
    long long len = 0ll, area[3] = {0ll, 0ll, 0ll};
    if (l != kTopNone) {
        const double* P0 = V + 3ull * p0;
        const double* P1 = V + 3ull * p1;
        const double* Pr = V + 3ull * loops[l].first_vertex;
        double d[3], a[3], b[3];
#pragma unroll
        for (int x = 0; x < 3; x++) d[x] = P1[x] - P0[x], a[x] = P0[x] - Pr[x], b[x] = P1[x] - Pr[x];
        const double X[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        len = (long long)rint(sqrt(dev_dot(d, d)) * 4294967296.0);
#pragma unroll
        for (int x = 0; x < 3; x++) area[x] = (long long)rint((0.5 * X[x]) * 268435456.0);
    }
    const TopRun r = top_run(l, lane);
    const uint32_t n = top_run_sum(l != kTopNone ? 1u : 0u, r, lane);
    len = top_run_sum(len, r, lane);
#pragma unroll
    for (int x = 0; x < 3; x++) area[x] = top_run_sum(area[x], r, lane);
    if (!r.head || l == kTopNone) return;
    TopLoop* k = &loops[l];
    atomicAdd(&k->n_edges, n);
    atomicAdd((unsigned long long*)&k->length_q32, (unsigned long long)len);
#pragma unroll
    for (int x = 0; x < 3; x++) atomicAdd((unsigned long long*)&k->area_q28[x], (unsigned long long)area[x]);
}

// One lane per loop and per shell: the final flags, a loop's share of its shell's record and the summary's two counts.
__global__ __launch_bounds__(256) void k_top_finish(const uint32_t n_loops, TopLoop* __restrict__ loops, const uint32_t n_shells, TopShell* __restrict__ shells,
                                                    TopCounters* __restrict__ ctr)
{
    const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    bool closed = false, tight = false;
    if (c < n_loops) {
        const uint32_t f = loops[c].flags, s = loops[c].shell;
        closed = (f & kTopLoopOpenMark) == 0u;
        loops[c].flags = (closed ? kTopLoopClosed : 0u) | ((f & kTopLoopBranched) ? kTopLoopBranched : 0u);
        if (s < n_shells) atomicAdd(&shells[s].n_loops, 1u);
    }
    if (c < n_shells) {
        const TopShell* h = &shells[c];
        const uint32_t f = (h->n_boundary ? kTopShellOpen : 0u) | (h->n_nonmanifold ? kTopShellNonManifold : 0u) | (h->n_miswound ? kTopShellMiswound : 0u);
        tight = f == 0u;
        shells[c].flags = tight ? kTopShellWatertight : f;
    }
    const unsigned long long mc = __ballot(closed), mt = __ballot(tight);
    if ((threadIdx.x & 63u) != 0u) return;
    if (mc) atomicAdd(&ctr->n_closed_loops, (unsigned long long)__popcll(mc));
    if (mt) atomicAdd(&ctr->n_watertight, (unsigned long long)__popcll(mt));
}

}  // namespace hfpf
