// csrc/snapshot.hpp -- snapshot / restore (hfpf_snapshot, hfpf_restore, hfpf_save, hfpf_load; include/hfpf.h):
// its kernels, its host code and its entries.  It builds on hfpf_handle and the helpers of hfpf.hip, which includes it once, at its end.
// The kernels: the used prefix of every pool <-> ONE contiguous staging buffer, so that a session
// crosses the link as a few large copies.  A span is a run of 16-byte units that lies 16-byte aligned in its pool and in the
// staging buffer; `head` leading bytes and everything behind `bytes` are not state (the unused record 0 of the record arrays,
// the up to three entries in front of an append region of the colour log, the tail of a list whose length is no multiple of
// four): packed as zeros, left alone in the pool when unpacked.  One launch takes up to kSnapSpans spans; a workgroup moves one
// 16 KB tile (4 units per lane, loads first), so the lanes of a wave read and write 1 KB runs on both sides.
#pragma once

#include "kernels.hpp"

namespace hfpf {

constexpr uint32_t kSnapSpans = 48;
constexpr uint32_t kSnapTileUnits = 1024;  // 16-byte units per workgroup
struct SnapSpans {
    uint64_t pool[kSnapSpans];    // address of the span's first unit in its pool
    uint64_t stage[kSnapSpans];   // ... and its byte offset in the staging buffer
    uint64_t bytes[kSnapSpans];   // span length, head included (a multiple of 4)
    uint32_t head[kSnapSpans];
    uint32_t tile0[kSnapSpans + 1];  // first tile of every span; tile0[n] = tiles of the launch
    uint32_t n;
};
// One unit that holds a span's head or tail: word by word.
template <bool PACK>
__device__ __forceinline__ void snap_edge_unit(uint8_t* pool, uint8_t* st, uint64_t u, uint64_t head, uint64_t bytes)
{
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    const uint64_t b = u * 16;
    const bool s0 = b >= head && b < bytes, s1 = b + 4 >= head && b + 4 < bytes, s2 = b + 8 >= head && b + 8 < bytes, s3 = b + 12 >= head && b + 12 < bytes;
    if (PACK) {
        if (s0) w0 = *reinterpret_cast<const uint32_t*>(pool + b);
        if (s1) w1 = *reinterpret_cast<const uint32_t*>(pool + b + 4);
        if (s2) w2 = *reinterpret_cast<const uint32_t*>(pool + b + 8);
        if (s3) w3 = *reinterpret_cast<const uint32_t*>(pool + b + 12);
        *reinterpret_cast<uint4*>(st + b) = make_uint4(w0, w1, w2, w3);
    } else {
        const uint4 v = *reinterpret_cast<const uint4*>(st + b);
        if (s0) *reinterpret_cast<uint32_t*>(pool + b) = v.x;
        if (s1) *reinterpret_cast<uint32_t*>(pool + b + 4) = v.y;
        if (s2) *reinterpret_cast<uint32_t*>(pool + b + 8) = v.z;
        if (s3) *reinterpret_cast<uint32_t*>(pool + b + 12) = v.w;
    }
}
template <bool PACK>
__global__ __launch_bounds__(256) void k_snap_copy(const SnapSpans sp, uint8_t* __restrict__ stage)
{
    uint32_t s = 0;
    while (s + 1 < sp.n && blockIdx.x >= sp.tile0[s + 1]) s++;  // workgroup-uniform: scalar compares on the kernel arguments
    const uint64_t bytes = sp.bytes[s], head = sp.head[s];
    const uint64_t n_units = (bytes + 15) >> 4;
    uint8_t* pool = reinterpret_cast<uint8_t*>(sp.pool[s]);
    uint8_t* st = stage + sp.stage[s];
    const uint8_t* src = PACK ? pool : st;
    uint8_t* dst = PACK ? st : pool;
    const uint64_t t0 = (uint64_t)(blockIdx.x - sp.tile0[s]) * kSnapTileUnits;
    const uint64_t u0 = t0 + threadIdx.x, u1 = u0 + 256u, u2 = u0 + 512u, u3 = u0 + 768u;
    // a tile that lies inside the span's whole units (all but a span's first and last tile): four loads in flight, four stores
    if (t0 * 16 >= head && (t0 + kSnapTileUnits) * 16 <= bytes) {  // workgroup-uniform
        const uint4 a = *reinterpret_cast<const uint4*>(src + u0 * 16), b = *reinterpret_cast<const uint4*>(src + u1 * 16);
        const uint4 c = *reinterpret_cast<const uint4*>(src + u2 * 16), d = *reinterpret_cast<const uint4*>(src + u3 * 16);
        *reinterpret_cast<uint4*>(dst + u0 * 16) = a;
        *reinterpret_cast<uint4*>(dst + u1 * 16) = b;
        *reinterpret_cast<uint4*>(dst + u2 * 16) = c;
        *reinterpret_cast<uint4*>(dst + u3 * 16) = d;
        return;
    }
    for (uint64_t u = u0; u < n_units && u < t0 + kSnapTileUnits; u += 256u) {
        if (u * 16 >= head && u * 16 + 16 <= bytes) *reinterpret_cast<uint4*>(dst + u * 16) = *reinterpret_cast<const uint4*>(src + u * 16);
        else snap_edge_unit<PACK>(pool, st, u, head, bytes);
    }
}

// What the restored indices are checked against: the used range of every pool as the snapshot's header states it (the host has
// compared those with the target's capacities before anything was uploaded).
enum SnapErr : uint32_t {
    SE_BRICK = 1,    // brick_lin outside the directory, or two bricks on one directory entry
    SE_RUN = 2,      // a brick's run record outside the used part of its log region
    SE_FRAME = 4,    // frame id >= max_frames
    SE_HEAD = 8,     // a chain head that names no log entry
    SE_SLOT = 16,    // stat_id / pre_dep beyond the records, first_frame beyond the frames
    SE_DEP = 32,     // a dependant list outside dep[], or one of its entries naming no record
    SE_LINK = 64,    // a log link that names no log entry / no slot
    SE_RECORD = 128, // nv_slot outside the slots, nv_key outside the grid
    SE_LIST = 256,   // reg_occ / prereg_list / occ_list / pending-cell entry outside the slots or the records
};
struct SnapLimits {
    uint64_t n_slots;   // (bricks + 1) * 512: slots of the allocated bricks and the null brick
    uint64_t n_normals, n_dep, n_reg, n_prereg, n_occ, n_pend, max_frames, dir_entries, region_cap;
    uint32_t n_bricks;
    uint32_t log_n[kLogRegions];
};
__device__ __forceinline__ bool snap_log_entry_ok(const SnapLimits& lim, uint32_t e)  // a 1-based log index that names a used entry
{
    if (e == 0) return false;
    const uint64_t r = (uint64_t)(e - 1) / lim.region_cap;
    return r < (uint64_t)kLogRegions && (uint64_t)(e - 1) - r * lim.region_cap < lim.log_n[r];
}

// Per-brick records: (brick_lin, run_start, run_len, run_cnt) of bricks first + 1 .. first + n as one 16-byte record each (the
// run record of a brick that never buffered is not state: zeros).  Unpacking also rebuilds the directory from brick_lin -- the
// compare-and-swap finds two bricks on one entry -- and checks the run record the streaming replay would follow.
template <bool PACK>
__global__ __launch_bounds__(256) void k_snap_bricks(const Tables t, const SnapLimits lim, uint4* __restrict__ rec, const uint32_t first, const uint32_t n, uint32_t* __restrict__ err)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t b = first + i + 1;
    if (PACK) {
        const uint32_t cnt = t.run_cnt[b];
        rec[i] = make_uint4(t.brick_lin[b], cnt ? t.run_start[b] : 0u, cnt ? t.run_len[b] : 0u, cnt);
        return;
    }
    const uint4 v = rec[i];
    t.brick_lin[b] = v.x;
    t.run_start[b] = v.y;
    t.run_len[b] = v.z;
    t.run_cnt[b] = v.w;
    uint32_t e = 0;
    if (v.x >= lim.dir_entries) e |= SE_BRICK;
    else if (atomicCAS(&t.dir[v.x], 0u, b) != 0u) e |= SE_BRICK;
    if (v.w == 1u) {  // one run: [run_start, run_start + run_len) is streamed
        const uint64_t r = v.y ? (uint64_t)(v.y - 1) / lim.region_cap : (uint64_t)kLogRegions;
        if (r >= (uint64_t)kLogRegions || (uint64_t)(v.y - 1) - r * lim.region_cap + v.z > lim.log_n[r]) e |= SE_RUN;
    }
    if (e) atomicOr(err, e);
}

// Frames: (id, viewpoint) of frame_list entries first .. first + n - 1 as one 16-byte record each: frame_vp is indexed by frame
// id, and ids need not be dense.
template <bool PACK>
__global__ __launch_bounds__(256) void k_snap_frames(const Tables t, uint4* __restrict__ rec, const uint32_t first, const uint32_t n, uint32_t* __restrict__ err)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (PACK) {
        const uint32_t id = t.frame_list[first + i];
        uint4 v = make_uint4(id, 0u, 0u, 0u);
        if (id < t.max_frames) {
            v.y = __float_as_uint(t.frame_vp[3 * (uint64_t)id]);
            v.z = __float_as_uint(t.frame_vp[3 * (uint64_t)id + 1]);
            v.w = __float_as_uint(t.frame_vp[3 * (uint64_t)id + 2]);
        }
        rec[i] = v;
        return;
    }
    const uint4 v = rec[i];
    t.frame_list[first + i] = v.x;
    if (v.x >= t.max_frames) {
        atomicOr(err, (uint32_t)SE_FRAME);
        return;
    }
    t.frame_vp[3 * (uint64_t)v.x] = __uint_as_float(v.y);
    t.frame_vp[3 * (uint64_t)v.x + 1] = __uint_as_float(v.z);
    t.frame_vp[3 * (uint64_t)v.x + 2] = __uint_as_float(v.w);
}

// Range check of a restored session, before any other kernel follows an index of it.  One thread per slot of the allocated bricks.
__global__ __launch_bounds__(256) void k_snap_check_slots(const Tables t, const SnapLimits lim, uint32_t* __restrict__ err)
{
    const uint64_t slot = (uint64_t)kBrickCells + (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (slot >= lim.n_slots) return;
    uint32_t e = 0;
    const uint4 hd = *reinterpret_cast<const uint4*>(&t.buf_head[slot * kChains]);
    static_assert(kChains == 4, "one 16-byte load reads a cell's chain heads");
    if ((hd.x && !snap_log_entry_ok(lim, hd.x)) || (hd.y && !snap_log_entry_ok(lim, hd.y)) || (hd.z && !snap_log_entry_ok(lim, hd.z)) ||
        (hd.w && !snap_log_entry_ok(lim, hd.w)))
        e |= SE_HEAD;
    const uint32_t ff = t.first_frame[slot];
    if (t.stat_id[slot] > lim.n_normals || t.pre_dep[slot] > lim.n_normals || (ff != kNoFrame && ff >= lim.max_frames)) e |= SE_SLOT;
    const uint64_t info = t.info[slot];
    const uint64_t cnt = (info >> kDepCntShift) & kDepCntMask, off = info >> kDepOffShift;
    if (cnt) {
        if (off + cnt > lim.n_dep) {
            e |= SE_DEP;
        } else {
            for (uint64_t k = 0; k < cnt; k++)
                if (t.dep[off + k].sid > lim.n_normals) e |= SE_DEP;
        }
    }
    if (e) atomicOr(err, e);
}

// ... one thread per used log entry (grid.y = append region): an unchained entry names its slot, a chained one the next entry or 0.
__global__ __launch_bounds__(256) void k_snap_check_log(const Tables t, const SnapLimits lim, uint32_t* __restrict__ err)
{
    const uint32_t r = blockIdx.y;
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= lim.log_n[r]) return;
    const uint32_t w = __float_as_uint(t.log_pt[(uint64_t)r * lim.region_cap + i + 1].w);
    const bool ok = (w & kLogUnlinked) ? (uint64_t)(w & ~kLogUnlinked) < lim.n_slots : (w == 0u || snap_log_entry_ok(lim, w));
    if (!ok) atomicOr(err, (uint32_t)SE_LINK);
}

// ... one thread per index of the longest list: records, registrations, filed pre-dependants, occupied cells, pending cells.
__global__ __launch_bounds__(256) void k_snap_check_lists(const GridParams g, const Tables t, const SnapLimits lim, const uint32_t* __restrict__ pend, uint32_t* __restrict__ err)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t e = 0;
    if (i >= 1 && i <= lim.n_normals) {
        int32_t x, y, z;
        const uint64_t key = t.nv_key[i];
        key_coords(g, key, x, y, z);
        if (t.nv_slot[i] >= lim.n_slots || (key >> g.key_bits) != 0 || x > g.dim[0] || y > g.dim[1] || z > g.dim[2]) e |= SE_RECORD;
    }
    if (i < lim.n_reg) {
        const uint2 ro = t.reg_occ[i];
        if (ro.x >= lim.n_slots || ro.y > lim.n_normals) e |= SE_LIST;
    }
    if (i < lim.n_prereg && t.prereg_list[i] >= lim.n_slots) e |= SE_LIST;
    if (i < lim.n_occ && t.occ_list[i] >= lim.n_slots) e |= SE_LIST;
    if (i < lim.n_pend && pend[i] >= lim.n_slots) e |= SE_LIST;
    if (e) atomicOr(err, e);
}

}  // namespace hfpf

// A blob = a 4096-byte header + the payload: sections, each 256-byte aligned, listed in the header as (id, offset, bytes).  The
// payload is what the staging buffer on the device holds: the pack kernels (k_snap_* above) gather the used prefix of every
// pool into it and it crosses the link through download_pageable / upload_pageable, whole or in windows.

namespace {

constexpr uint32_t kSnapVersion = 1;
constexpr uint32_t kSnapLayoutRev = 2;  // bump when a table's meaning changes without its shape changing (2: the colour log's section is sized by the total)
constexpr uint64_t kSnapLayoutTag = ((uint64_t)kSnapLayoutRev << 48) | ((uint64_t)kChains << 40) | ((uint64_t)kLogRegions << 32) | ((uint64_t)kStatWords << 24) |
                                    ((uint64_t)sizeof(DepEntry) << 16) | ((uint64_t)C_COUNT << 8) | (uint64_t)kBrickShift;
constexpr char kSnapMagic[8] = {'H', 'F', 'P', 'F', 'S', 'N', 'A', 'P'};
constexpr uint32_t kSnapMaxSections = 32;
constexpr uint32_t kSnapSemanticFlags = HFPF_FLAG_FUSE_COLOR | HFPF_FLAG_PCL_SHIFTED_COV;

enum SnapSectionId : uint32_t {
    SS_CTR = 1, SS_LOG_CTR, SS_INFO, SS_FIRST_FRAME, SS_BUF_HEAD, SS_STAT_ID, SS_PRE_DEP, SS_OCC_MASK, SS_ND_MASK, SS_BRICKS, SS_LOG_PT, SS_LOG_RGB,
    SS_NV_KEY, SS_NV_SLOT, SS_NV_C, SS_NV_N, SS_NV_LINE, SS_STATS, SS_REG_OCC, SS_DEP, SS_OCC_LIST, SS_PREREG, SS_FRAMES, SS_PEND,
    SS_HIDDEN  // the HIDDEN bits of hfpf_hide_*, 64 bytes per brick; the last section, present only when something is hidden
};
struct SnapSection {
    uint32_t id, reserved;
    uint64_t offset, bytes;  // offset into the payload (a multiple of 256); bytes without the padding behind them
};
struct SnapHeader {  // at the front of the 4096 header bytes; the rest of them is zero.  Every field is naturally aligned: no padding.
    char magic[8];
    uint32_t version, header_bytes;
    uint64_t layout_tag, total_bytes, payload_bytes, payload_checksum, header_checksum;  // header_checksum: over the 4096 bytes with this field 0
    float resolution;
    uint32_t flags;
    double bbox[6];
    int32_t k, K, gate, reserved0;
    double cylinder_radius, ball_radius, z_clip_min, z_clip_max;
    uint64_t need_bricks, log_points, need_normals, need_frames;
    uint64_t frames_integrated, clean_passes, next_frame_id, voxels_occupied, voxels_with_normal;
    uint32_t dirty, pend_valid, normals_possible, n_sections;
    uint64_t gate_done, direct_linked;
    uint64_t n_bricks, n_normals, n_occ, n_reg, n_prereg, n_dep, n_frames, n_pend;
    uint64_t n_linked[kLogRegions], log_n[kLogRegions];
    SnapSection sec[kSnapMaxSections];
};
static_assert(sizeof(SnapHeader) <= HFPF_SNAPSHOT_HEADER_BYTES, "the snapshot header has a fixed size");
static_assert(sizeof(struct hfpf_snapshot_info) == 248, "hfpf_snapshot_info layout");

// 64-bit checksum of n bytes (n a multiple of 32: sections are 256-byte aligned): four interleaved multiply-xorshift lanes over the
// 8-byte words, folded at the end.  Not cryptographic: it catches truncation, bit rot and mixed-up files.
uint64_t snap_checksum(const void* data, uint64_t n)
{
    const uint64_t kMul = 0x9E3779B97F4A7C15ull;
    uint64_t a = 0x243F6A8885A308D3ull, b = 0x13198A2E03707344ull, c = 0xA4093822299F31D0ull, d = 0x082EFA98EC4E6C89ull;
    const uint8_t* p = (const uint8_t*)data;
    for (uint64_t i = 0; i + 32 <= n; i += 32) {
        uint64_t w[4];
        memcpy(w, p + i, 32);
        a = (a ^ w[0]) * kMul, a ^= a >> 29;
        b = (b ^ w[1]) * kMul, b ^= b >> 29;
        c = (c ^ w[2]) * kMul, c ^= c >> 29;
        d = (d ^ w[3]) * kMul, d ^= d >> 29;
    }
    uint64_t r = n;
    for (uint64_t v : {a, b, c, d}) r = (r ^ v) * kMul, r ^= r >> 32;
    return r;
}

uint64_t snap_header_checksum(const uint8_t* hdr)
{
    uint8_t tmp[HFPF_SNAPSHOT_HEADER_BYTES];
    memcpy(tmp, hdr, sizeof tmp);
    memset(tmp + offsetof(SnapHeader, header_checksum), 0, 8);
    return snap_checksum(tmp, sizeof tmp);
}

// The header of a blob, validated as far as the header alone allows: 0, or why not (a static text).
const char* snap_parse_header(const void* blob, uint64_t bytes, SnapHeader* hd)
{
    if (!blob || bytes < HFPF_SNAPSHOT_HEADER_BYTES) return "shorter than a snapshot header";
    memcpy(hd, blob, sizeof *hd);
    if (memcmp(hd->magic, kSnapMagic, 8) != 0) return "not a snapshot (magic)";
    if (hd->version != kSnapVersion || hd->header_bytes != HFPF_SNAPSHOT_HEADER_BYTES) return "unknown snapshot format version";
    if (hd->header_checksum != snap_header_checksum((const uint8_t*)blob)) return "header checksum mismatch";
    if (hd->n_sections > kSnapMaxSections || hd->total_bytes != hd->payload_bytes + HFPF_SNAPSHOT_HEADER_BYTES || (hd->payload_bytes & 255u)) return "inconsistent header";
    return nullptr;
}

// How much of every pool a session used (from the counters at snapshot, from the header at restore).
struct SnapUsed {
    uint64_t n_bricks, n_normals, n_occ, n_reg, n_prereg, n_dep, n_frames, n_pend;
    uint64_t log_n[kLogRegions];
    bool hidden;  // the session hides rows: the blob carries SS_HIDDEN (snapshot: Session::n_hidden; restore: the header lists the section)
};

inline uint64_t up16(uint64_t v) { return (v + 15) & ~15ull; }
inline uint64_t up256(uint64_t v) { return (v + 255) & ~255ull; }
// bytes in front of append region r of the colour log that make its first entry's unit 16-byte aligned (entries are 1-based)
inline uint32_t snap_rgb_head(uint64_t region_cap, int r) { return (uint32_t)((((uint64_t)r * region_cap + 1) & 3u) * 4u); }

// The sections of a session, in file order; the same function lays a blob out at snapshot and reads it back at restore.
uint32_t snap_layout(const SnapUsed& u, bool color, uint64_t region_cap, SnapSection* sec, uint64_t* payload_bytes)
{
    const uint64_t cells = u.n_bricks * (uint64_t)kBrickCells, rec = u.n_normals ? u.n_normals + 1 : 0;
    uint64_t log_pt = 0, log_rgb = 0;
    for (int r = 0; r < kLogRegions; r++) log_pt += u.log_n[r] * sizeof(float4);
    // The colour log's regions are packed one behind the other, each with its head and padded to 16 bytes (snap_spans): how many bytes
    // that takes depends on how the buffered points spread over the append regions, which is scheduling.  The section is sized by the
    // total alone -- a head and a padding of less than 16 bytes each per region -- so that a blob's size follows the counts only.
    if (log_pt) log_rgb = up16(log_pt / sizeof(float4) * 4) + 32ull * kLogRegions;
    (void)region_cap;
    const struct {
        uint32_t id;
        uint64_t bytes;
    } all[] = {{SS_CTR, C_COUNT * 8}, {SS_LOG_CTR, kLogRegions * 16 * 8}, {SS_INFO, cells * 8}, {SS_FIRST_FRAME, cells * 4}, {SS_BUF_HEAD, cells * 4 * kChains},
               {SS_STAT_ID, cells * 4}, {SS_PRE_DEP, cells * 4}, {SS_OCC_MASK, u.n_bricks * 64}, {SS_ND_MASK, u.n_bricks * 128}, {SS_BRICKS, u.n_bricks * 16},
               {SS_LOG_PT, log_pt}, {SS_LOG_RGB, color ? log_rgb : 0}, {SS_NV_KEY, rec * 8}, {SS_NV_SLOT, rec * 4}, {SS_NV_C, rec * 12}, {SS_NV_N, rec * 12},
               {SS_NV_LINE, rec * 32}, {SS_STATS, rec * kStatWords * 8}, {SS_REG_OCC, u.n_reg * 8}, {SS_DEP, u.n_dep * sizeof(DepEntry)}, {SS_OCC_LIST, u.n_occ * 4},
               {SS_PREREG, u.n_prereg * 4}, {SS_FRAMES, u.n_frames * 16}, {SS_PEND, u.n_pend * 4}};
    uint32_t n = 0;
    uint64_t off = 0;
    for (const auto& a : all) {
        sec[n++] = SnapSection{a.id, 0u, off, a.bytes};
        off += up256(a.bytes);
    }
    if (u.hidden) {
        sec[n++] = SnapSection{SS_HIDDEN, 0u, off, u.n_bricks * 64};
        off += up256(u.n_bricks * 64);
    }
    *payload_bytes = off;
    return n;
}

struct SnapSpan {  // SnapSpans (above), one entry
    uint64_t pool, stage, bytes;
    uint32_t head;
};

// The copy spans of a session on this handle (everything but the two gathered sections).  pend = the pending-cell list.
void snap_spans(hfpf_handle* h, const SnapUsed& u, const SnapSection* sec, uint32_t n_sec, std::vector<SnapSpan>* out)
{
    const Tables& t = h->t;
    const uint64_t c0 = kBrickCells;  // the first cell of brick 1
    auto at = [&](uint32_t id) -> const SnapSection& {
        for (uint32_t i = 0; i < n_sec; i++)
            if (sec[i].id == id) return sec[i];
        return sec[0];
    };
    auto add = [&](uint32_t id, const void* pool, uint32_t head = 0) {
        const SnapSection& s = at(id);
        if (s.bytes) out->push_back(SnapSpan{(uint64_t)(uintptr_t)pool, s.offset, s.bytes, head});
    };
    add(SS_CTR, t.ctr);
    add(SS_LOG_CTR, t.log_ctr);
    add(SS_INFO, t.info + c0);
    add(SS_FIRST_FRAME, t.first_frame + c0);
    add(SS_BUF_HEAD, t.buf_head + c0 * kChains);
    add(SS_STAT_ID, t.stat_id + c0);
    add(SS_PRE_DEP, t.pre_dep + c0);
    add(SS_OCC_MASK, t.occ_mask + 8);
    add(SS_ND_MASK, t.nd_mask + 16);
    add(SS_NV_KEY, t.nv_key, 8);  // record 0 does not exist: head
    add(SS_NV_SLOT, t.nv_slot, 4);
    add(SS_NV_C, t.nv_c, 12);
    add(SS_NV_N, t.nv_n, 12);
    add(SS_NV_LINE, t.nv_line, 32);
    add(SS_STATS, t.stats);
    add(SS_REG_OCC, t.reg_occ);
    add(SS_DEP, t.dep);
    add(SS_OCC_LIST, t.occ_list);
    add(SS_PREREG, t.prereg_list);
    add(SS_PEND, h->pend_a.p);
    if (u.hidden) add(SS_HIDDEN, h->hidden_words + 8);
    uint64_t off_pt = at(SS_LOG_PT).offset, off_rgb = at(SS_LOG_RGB).offset;
    for (int r = 0; r < kLogRegions; r++) {
        if (!u.log_n[r]) continue;
        const uint64_t first = (uint64_t)r * t.log_region_cap + 1;  // the region's first entry
        out->push_back(SnapSpan{(uint64_t)(uintptr_t)(t.log_pt + first), off_pt, u.log_n[r] * sizeof(float4), 0u});
        off_pt += u.log_n[r] * sizeof(float4);
        if (t.color) {
            const uint32_t head = snap_rgb_head(t.log_region_cap, r);
            out->push_back(SnapSpan{(uint64_t)(uintptr_t)(t.log_rgb + (first & ~3ull)), off_rgb, head + u.log_n[r] * 4, head});
            off_rgb += up16(head + u.log_n[r] * 4);
        }
    }
}

// Pack (device -> staging) or unpack the part of the payload inside the window [w0, w1) (multiples of 16); the staging buffer
// holds that window from its first byte.  err: the range check's error words.
template <bool PACK>
int snap_move_window(hfpf_handle* h, uint8_t* stage, uint32_t* err, const SnapSection* sec, uint32_t n_sec, const std::vector<SnapSpan>& spans, const SnapLimits& lim,
                     uint64_t w0, uint64_t w1)
{
    SnapSpans sp;
    memset(&sp, 0, sizeof sp);
    auto flush = [&]() {
        if (sp.n == 0) return;
        hipLaunchKernelGGL(k_snap_copy<PACK>, dim3(sp.tile0[sp.n]), dim3(256), 0, h->stream, sp, stage);
        memset(&sp, 0, sizeof sp);
    };
    for (const SnapSpan& full : spans) {
        const uint64_t lo = std::max(full.stage, w0), hi = std::min(full.stage + up16(full.bytes), w1);
        if (lo >= hi) continue;
        const uint64_t skip = lo - full.stage;  // (a multiple of 16)
        const uint64_t bytes = std::min(full.bytes - skip, hi - lo);
        const uint32_t head = (uint32_t)(full.head > skip ? full.head - skip : 0);
        const uint64_t tiles = (up16(bytes) / 16 + kSnapTileUnits - 1) / kSnapTileUnits;
        if (sp.n == kSnapSpans || (uint64_t)sp.tile0[sp.n] + tiles > 0x7FFFFFFFull) flush();
        sp.pool[sp.n] = full.pool + skip;
        sp.stage[sp.n] = lo - w0;
        sp.bytes[sp.n] = bytes;
        sp.head[sp.n] = head;
        sp.tile0[sp.n + 1] = sp.tile0[sp.n] + (uint32_t)tiles;
        sp.n++;
    }
    flush();
    // the gathered sections: 16-byte records
    for (uint32_t i = 0; i < n_sec; i++) {
        if ((sec[i].id != SS_BRICKS && sec[i].id != SS_FRAMES) || !sec[i].bytes) continue;
        const uint64_t lo = std::max(sec[i].offset, w0), hi = std::min(sec[i].offset + sec[i].bytes, w1);
        if (lo >= hi) continue;
        const uint32_t first = (uint32_t)((lo - sec[i].offset) / 16), n = (uint32_t)((hi - lo) / 16);
        uint4* rec = (uint4*)(stage + (lo - w0));
        if (sec[i].id == SS_BRICKS) hipLaunchKernelGGL(k_snap_bricks<PACK>, dim3(blocks_for(n, 256)), dim3(256), 0, h->stream, h->t, lim, rec, first, n, err);
        else hipLaunchKernelGGL(k_snap_frames<PACK>, dim3(blocks_for(n, 256)), dim3(256), 0, h->stream, h->t, rec, first, n, err);
    }
    HIPCHK(h, hipGetLastError());
    return HFPF_OK;
}

// A staging buffer for `payload` bytes, or -- when the device has no room for it -- for the largest window it has room for (halved
// until the allocation succeeds; a window is a multiple of 1 MB).  HFPF_TEST_SNAPSHOT_WINDOW=<bytes> (tests) caps it.
int snap_stage_alloc(hfpf_handle* h, uint64_t payload, uint64_t* window)
{
    uint64_t want = std::max<uint64_t>(up256(payload), 4096);
    if (const char* e = getenv("HFPF_TEST_SNAPSHOT_WINDOW")) want = std::min<uint64_t>(want, std::max<uint64_t>((uint64_t)atoll(e) & ~4095ull, 4096));
    if (h->snap_stage.p && h->snap_stage.bytes >= want) {
        *window = want;
        return HFPF_OK;
    }
    if (h->snap_stage.p) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipFree(h->snap_stage.p));
        h->device_bytes -= h->snap_stage.bytes;
        h->snap_stage.p = nullptr, h->snap_stage.bytes = 0;
    }
    for (;;) {
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) {
            h->snap_stage.p = p;
            h->snap_stage.bytes = want;
            h->device_bytes += want;
            *window = want;
            return HFPF_OK;
        }
        (void)hipGetLastError();
        if (e != hipErrorOutOfMemory || want <= (1u << 20)) return fail(h, HFPF_ERR_HIP, "snapshot staging: hipMalloc(%llu) failed: %s", (unsigned long long)want, hipGetErrorString(e));
        want = std::max<uint64_t>((want / 2 + (1u << 20) - 1) & ~(uint64_t)((1u << 20) - 1), 1u << 20);
    }
}

int snap_refuse_distributed(hfpf_handle* h, const char* what)
{
    if (h->dist_on) return fail(h, HFPF_ERR_STATE, "%s: not available on a handle with an RCCL communicator", what);
    if (h->epoch_used) return fail(h, HFPF_ERR_STATE, "%s: this handle has exchanged epoch records or statistic words; a distributed snapshot is not provided", what);
    return HFPF_OK;
}

SnapLimits snap_limits(const hfpf_handle* h, const SnapUsed& u)
{
    SnapLimits lim;
    memset(&lim, 0, sizeof lim);
    lim.n_slots = (u.n_bricks + 1) * (uint64_t)kBrickCells;
    lim.n_normals = u.n_normals, lim.n_dep = u.n_dep, lim.n_reg = u.n_reg, lim.n_prereg = u.n_prereg, lim.n_occ = u.n_occ, lim.n_pend = u.n_pend;
    lim.max_frames = h->t.max_frames;
    lim.dir_entries = h->dir_entries;
    lim.region_cap = h->t.log_region_cap;
    lim.n_bricks = (uint32_t)u.n_bricks;
    for (int r = 0; r < kLogRegions; r++) lim.log_n[r] = (uint32_t)u.log_n[r];
    return lim;
}

// The host state a snapshot carries, into the header and back: ONE field list, the same order in both.  Everything else in Session
// is re-created after a restore or needs not be (see the notes there); frames_integrated and clean_passes travel too because a
// clear leaves them alone.
void session_to_header(const hfpf_handle* h, const SnapUsed& u, SnapHeader* hd)
{
    const Session& ss = h->ss;
    hd->frames_integrated = h->frames_integrated;
    hd->clean_passes = h->clean_passes;
    hd->next_frame_id = ss.next_frame_id;
    hd->dirty = ss.dirty ? 1 : 0;
    hd->pend_valid = ss.pend_valid ? 1 : 0;
    hd->normals_possible = ss.normals_possible ? 1 : 0;
    hd->gate_done = ss.gate_done;
    hd->direct_linked = ss.direct_linked;
    for (int r = 0; r < kLogRegions; r++) hd->n_linked[r] = std::min(ss.n_linked[r], u.log_n[r]);
}
void header_to_session(const SnapHeader& hd, hfpf_handle* h)
{
    Session& ss = h->ss;
    h->frames_integrated = hd.frames_integrated;
    h->clean_passes = hd.clean_passes;
    ss.next_frame_id = (uint32_t)hd.next_frame_id;
    ss.dirty = hd.dirty != 0;
    ss.pend_valid = hd.pend_valid != 0;
    ss.normals_possible = hd.normals_possible != 0;
    ss.gate_done = hd.gate_done;
    ss.direct_linked = hd.direct_linked;
    for (int r = 0; r < kLogRegions; r++) ss.n_linked[r] = hd.n_linked[r];
}

int snapshot_locked(hfpf_handle* h, void** blob_out, uint64_t* bytes_out)
{
    int rc = snap_refuse_distributed(h, "snapshot");
    if (!rc) rc = read_prologue_locked(h);  // (the counter read-back waits for a clean pass still running)
    if (rc) return rc;
    const Tables& t = h->t;
    const hfpf_config& c = h->cfg;
    SnapUsed u{};
    u.n_bricks = std::min<uint64_t>(h->h_ctr[C_BRICKS], t.max_bricks);
    u.n_normals = std::min<uint64_t>(h->h_ctr[C_NORMALS], t.max_normals);
    u.n_occ = std::min<uint64_t>(h->h_ctr[C_OCC], t.max_occ);
    u.n_reg = std::min<uint64_t>(h->h_ctr[C_REG], t.max_reg);
    u.n_prereg = std::min<uint64_t>(h->h_ctr[C_PREREG], t.max_reg);
    u.n_dep = std::min<uint64_t>(h->h_ctr[C_DEP], t.max_dep);
    u.n_frames = std::min<uint64_t>(h->h_ctr[C_FRAMES], t.max_frames);
    u.n_pend = h->ss.pend_valid ? h->h_ctr[C_PEND] : 0;
    if (u.n_pend * 4 > h->pend_a.bytes) return fail(h, HFPF_ERR_STATE, "snapshot: pending-cell list of %llu entries exceeds its buffer (internal)", (unsigned long long)u.n_pend);
    for (int r = 0; r < kLogRegions; r++) u.log_n[r] = std::min<uint64_t>(h->h_log_ctr[r * 16], t.log_region_cap);
    u.hidden = snapshot_carries_hidden(h->ss.n_hidden);

    uint8_t hdr_bytes[HFPF_SNAPSHOT_HEADER_BYTES];
    memset(hdr_bytes, 0, sizeof hdr_bytes);
    SnapHeader hd;
    memset(&hd, 0, sizeof hd);
    memcpy(hd.magic, kSnapMagic, 8);
    hd.version = kSnapVersion;
    hd.header_bytes = HFPF_SNAPSHOT_HEADER_BYTES;
    hd.layout_tag = kSnapLayoutTag;
    hd.n_sections = snap_layout(u, t.color != 0, t.log_region_cap, hd.sec, &hd.payload_bytes);
    hd.total_bytes = hd.payload_bytes + HFPF_SNAPSHOT_HEADER_BYTES;
    hd.resolution = c.resolution;
    hd.flags = c.flags;
    memcpy(hd.bbox, c.bbox, sizeof hd.bbox);
    hd.k = c.k, hd.K = c.K, hd.gate = c.gate;
    hd.cylinder_radius = c.cylinder_radius, hd.ball_radius = c.ball_radius, hd.z_clip_min = c.z_clip_min, hd.z_clip_max = c.z_clip_max;
    {
        const uint64_t per = 2ull * (uint64_t)c.K + 1ull;  // max_occ = 4 n, max_reg = (2K+1) n, max_dep = 2 max_reg (alloc_tables)
        uint64_t nn = std::max<uint64_t>(u.n_normals, 1);
        nn = std::max(nn, (u.n_occ + 3) / 4);
        nn = std::max(nn, (std::max(u.n_reg, u.n_prereg) + per - 1) / per);
        nn = std::max(nn, (u.n_dep + 2 * per - 1) / (2 * per));
        hd.need_normals = nn;
    }
    hd.need_bricks = std::max<uint64_t>(u.n_bricks, 1);
    hd.log_points = c.max_log_points;
    hd.need_frames = 1;  // raised below to the largest frame id + 1
    hd.voxels_occupied = h->h_ctr[C_OCC];
    hd.voxels_with_normal = h->h_ctr[C_NORMALS];
    hd.n_bricks = u.n_bricks, hd.n_normals = u.n_normals, hd.n_occ = u.n_occ, hd.n_reg = u.n_reg, hd.n_prereg = u.n_prereg, hd.n_dep = u.n_dep;
    hd.n_frames = u.n_frames, hd.n_pend = u.n_pend;
    for (int r = 0; r < kLogRegions; r++) hd.log_n[r] = u.log_n[r];
    session_to_header(h, u, &hd);

    uint64_t window = 0;
    if ((rc = snap_stage_alloc(h, hd.payload_bytes, &window))) return rc;
    uint32_t* err; if ((rc = scratch_n(h, h->snap_err, 16, &err))) return rc;
    uint8_t* stage = static_cast<uint8_t*>(h->snap_stage.p);
    uint8_t* blob = (uint8_t*)host_result_alloc(hd.total_bytes);
    if (!blob) return fail(h, HFPF_ERR_CAPACITY, "snapshot: host allocation of %llu bytes failed", (unsigned long long)hd.total_bytes);
    std::vector<SnapSpan> spans;
    snap_spans(h, u, hd.sec, hd.n_sections, &spans);
    const SnapLimits lim = snap_limits(h, u);
    for (uint64_t w0 = 0; w0 < hd.payload_bytes; w0 += window) {
        const uint64_t w1 = std::min(hd.payload_bytes, w0 + window);
        hipError_t e = hipMemsetAsync(stage, 0, w1 - w0, h->stream);  // the gaps between sections are zero
        if (e == hipSuccess) rc = snap_move_window<true>(h, stage, err, hd.sec, hd.n_sections, spans, lim, w0, w1);
        if (e == hipSuccess && !rc) e = download_pageable(h, blob + HFPF_SNAPSHOT_HEADER_BYTES + w0, stage, w1 - w0);
        if (e != hipSuccess) rc = fail(h, HFPF_ERR_HIP, "snapshot download: %s", hipGetErrorString(e));
        if (rc) {
            free(blob);
            return rc;
        }
    }
    for (uint32_t i = 0; i < hd.n_sections; i++)  // the largest frame id this session integrated
        if (hd.sec[i].id == SS_FRAMES)
            for (uint64_t f = 0; f < u.n_frames; f++) {
                uint32_t id;
                memcpy(&id, blob + HFPF_SNAPSHOT_HEADER_BYTES + hd.sec[i].offset + 16 * f, 4);
                hd.need_frames = std::max<uint64_t>(hd.need_frames, (uint64_t)id + 1);
            }
    hd.payload_checksum = snap_checksum(blob + HFPF_SNAPSHOT_HEADER_BYTES, hd.payload_bytes);
    memcpy(hdr_bytes, &hd, sizeof hd);
    hd.header_checksum = snap_header_checksum(hdr_bytes);
    memcpy(hdr_bytes, &hd, sizeof hd);
    memcpy(blob, hdr_bytes, sizeof hdr_bytes);
    *blob_out = blob;
    *bytes_out = hd.total_bytes;
    return HFPF_OK;
}

int restore_locked(hfpf_handle* h, const void* blob, uint64_t bytes)
{
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc = snap_refuse_distributed(h, "restore");
    if (rc) return rc;
    // ---- everything the host can decide, before the handle is touched ----
    SnapHeader hd;
    if (const char* why = snap_parse_header(blob, bytes, &hd)) return fail(h, HFPF_ERR_BAD_ARG, "restore: %s", why);
    if (hd.layout_tag != kSnapLayoutTag)
        return fail(h, HFPF_ERR_BAD_ARG, "restore: the snapshot was written by a build with another table layout (tag %llx, this build %llx)", (unsigned long long)hd.layout_tag,
                    (unsigned long long)kSnapLayoutTag);
    if (bytes < hd.total_bytes) return fail(h, HFPF_ERR_BAD_ARG, "restore: %llu bytes given, the header says %llu", (unsigned long long)bytes, (unsigned long long)hd.total_bytes);
    const uint8_t* payload = (const uint8_t*)blob + HFPF_SNAPSHOT_HEADER_BYTES;
    if (snap_checksum(payload, hd.payload_bytes) != hd.payload_checksum) return fail(h, HFPF_ERR_BAD_ARG, "restore: payload checksum mismatch");
    const hfpf_config& c = h->cfg;
    const Tables& t = h->t;
    uint32_t res_a, res_b;
    memcpy(&res_a, &hd.resolution, 4);
    memcpy(&res_b, &c.resolution, 4);
    if (res_a != res_b || memcmp(hd.bbox, c.bbox, sizeof hd.bbox) != 0 || hd.k != c.k || hd.K != c.K || hd.gate != c.gate ||
        memcmp(&hd.cylinder_radius, &c.cylinder_radius, 8) != 0 || memcmp(&hd.ball_radius, &c.ball_radius, 8) != 0 || memcmp(&hd.z_clip_min, &c.z_clip_min, 8) != 0 ||
        memcmp(&hd.z_clip_max, &c.z_clip_max, 8) != 0 || ((hd.flags ^ c.flags) & kSnapSemanticFlags))
        return fail(h, HFPF_ERR_BAD_CONFIG, "restore: the snapshot was made with another grid configuration (resolution, bbox, k, K, gate, radii, z-clips, colour / covariance flags)");
    if (hd.log_points != c.max_log_points)
        return fail(h, HFPF_ERR_BAD_CONFIG, "restore: max_log_points %llu, the snapshot needs exactly %llu (log indices are not remapped)", (unsigned long long)c.max_log_points,
                    (unsigned long long)hd.log_points);
    SnapUsed u{};
    u.n_bricks = hd.n_bricks, u.n_normals = hd.n_normals, u.n_occ = hd.n_occ, u.n_reg = hd.n_reg, u.n_prereg = hd.n_prereg, u.n_dep = hd.n_dep;
    u.n_frames = hd.n_frames, u.n_pend = hd.n_pend;
    for (uint32_t i = 0; i < hd.n_sections; i++) u.hidden = u.hidden || hd.sec[i].id == SS_HIDDEN;  // (the layout below must then agree)
    for (int r = 0; r < kLogRegions; r++) {
        u.log_n[r] = hd.log_n[r];
        if (hd.log_n[r] > t.log_region_cap || hd.n_linked[r] > hd.log_n[r]) return fail(h, HFPF_ERR_BAD_ARG, "restore: log region %d out of range", r);
    }
    if (u.n_bricks > t.max_bricks || u.n_normals > t.max_normals || u.n_occ > t.max_occ || u.n_reg > t.max_reg || u.n_prereg > t.max_reg || u.n_dep > t.max_dep ||
        hd.need_frames > t.max_frames || u.n_frames > t.max_frames)
        return fail(h, HFPF_ERR_CAPACITY,
                    "restore: the session needs max_bricks >= %llu, max_normals >= %llu, max_frames >= %llu (this handle: %llu, %llu, %llu)", (unsigned long long)hd.need_bricks,
                    (unsigned long long)hd.need_normals, (unsigned long long)hd.need_frames, (unsigned long long)t.max_bricks, (unsigned long long)t.max_normals,
                    (unsigned long long)t.max_frames);
    if (u.n_pend > u.n_occ || hd.gate_done > u.n_occ) return fail(h, HFPF_ERR_BAD_ARG, "restore: inconsistent header (pending cells)");
    {   // the section table must be the one this build lays out for these counts, and the counters in the payload the header's
        SnapSection want[kSnapMaxSections];
        uint64_t pb = 0;
        const uint32_t n = snap_layout(u, t.color != 0, t.log_region_cap, want, &pb);
        if (n != hd.n_sections || pb != hd.payload_bytes || memcmp(want, hd.sec, n * sizeof(SnapSection)) != 0)
            return fail(h, HFPF_ERR_BAD_ARG, "restore: section table does not match the header's counts");
        unsigned long long ctr[C_COUNT];
        memcpy(ctr, payload + hd.sec[0].offset, sizeof ctr);  // (section 0 is SS_CTR)
        if (ctr[C_BRICKS] != u.n_bricks || ctr[C_NORMALS] != u.n_normals || ctr[C_OCC] != u.n_occ || ctr[C_REG] != u.n_reg || ctr[C_PREREG] != u.n_prereg ||
            ctr[C_DEP] != u.n_dep || ctr[C_FRAMES] != u.n_frames || ctr[C_ERR] != 0)
            return fail(h, HFPF_ERR_BAD_ARG, "restore: counters in the payload do not match the header");
        const uint8_t* lc = payload + hd.sec[1].offset;  // SS_LOG_CTR
        for (int r = 0; r < kLogRegions; r++) {
            unsigned long long n_r;
            memcpy(&n_r, lc + (size_t)r * 16 * 8, 8);
            if (n_r != u.log_n[r]) return fail(h, HFPF_ERR_BAD_ARG, "restore: log counters in the payload do not match the header");
        }
    }
    // ---- from here on a failure leaves the handle as after hfpf_clear ----
    if ((rc = clear_locked(h))) return rc;
    auto bail = [&](int code) {
        const std::string msg = h->err;
        (void)hipStreamSynchronize(h->stream);
        (void)reset_state(h);  // in full: what was uploaded is not to be trusted
        h->ss.dirty = true;
        h->err = msg;
        return code;
    };
    uint64_t window = 0;
    if ((rc = snap_stage_alloc(h, hd.payload_bytes, &window))) return bail(rc);
    uint32_t *err, *pend = nullptr;  // pend: read below u.n_pend only
    if ((rc = scratch_n(h, h->snap_err, 16, &err))) return bail(rc);
    if (u.n_pend && (rc = scratch_n(h, h->pend_a, u.n_pend, &pend))) return bail(rc);
    if (u.hidden && (rc = hide_words_locked(h))) return bail(rc);
    uint8_t* stage = static_cast<uint8_t*>(h->snap_stage.p);
    if (hipMemsetAsync(err, 0, 64, h->stream) != hipSuccess) return bail(fail(h, HFPF_ERR_HIP, "restore: hipMemsetAsync failed"));
    std::vector<SnapSpan> spans;
    snap_spans(h, u, hd.sec, hd.n_sections, &spans);
    const SnapLimits lim = snap_limits(h, u);
    for (uint64_t w0 = 0; w0 < hd.payload_bytes; w0 += window) {
        const uint64_t w1 = std::min(hd.payload_bytes, w0 + window);
        const hipError_t e = upload_pageable(h, stage, payload + w0, w1 - w0);
        if (e != hipSuccess) return bail(fail(h, HFPF_ERR_HIP, "restore upload: %s", hipGetErrorString(e)));
        if ((rc = snap_move_window<false>(h, stage, err, hd.sec, hd.n_sections, spans, lim, w0, w1))) return bail(rc);
        if (w1 < hd.payload_bytes && hipStreamSynchronize(h->stream) != hipSuccess) return bail(fail(h, HFPF_ERR_HIP, "restore: unpack failed"));  // the window is reused
    }
    // range check of every index a later kernel would follow, before anything else touches the tables
    if (u.n_bricks) hipLaunchKernelGGL(k_snap_check_slots, dim3(blocks_for(u.n_bricks * (uint64_t)kBrickCells, 256)), dim3(256), 0, h->stream, h->t, lim, err);
    {
        uint64_t max_log = 0;
        for (int r = 0; r < kLogRegions; r++) max_log = std::max(max_log, u.log_n[r]);
        if (max_log) hipLaunchKernelGGL(k_snap_check_log, dim3(blocks_for(max_log, 256), kLogRegions), dim3(256), 0, h->stream, h->t, lim, err);
        const uint64_t n_list = std::max({u.n_normals + 1, u.n_reg, u.n_prereg, u.n_occ, u.n_pend});
        hipLaunchKernelGGL(k_snap_check_lists, dim3(blocks_for(n_list, 256)), dim3(256), 0, h->stream, h->g, h->t, lim, pend, err);
    }
    if (hipGetLastError() != hipSuccess) return bail(fail(h, HFPF_ERR_HIP, "restore: launch of the range check failed"));
    uint32_t err_word = 0;
    if (hipMemcpyAsync(&err_word, err, 4, hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
        return bail(fail(h, HFPF_ERR_HIP, "restore: reading the range check's result failed"));
    if (err_word) return bail(fail(h, HFPF_ERR_IO, "restore: the snapshot's tables hold indices outside their pools (range check bits 0x%x); the handle has been cleared", err_word));
    header_to_session(hd, h);
    if ((rc = read_counters(h))) return bail(rc);  // h_ctr, h_log_ctr, n_bricks_known from the restored device counters
    h->ss.n_bricks_before = h->ss.n_bricks_known;
    if (u.hidden) {  // |H| and Tables::hidden from the restored bits; they must lie inside normal_found
        HideCall c;
        HideCounts k{};
        if ((rc = hide_begin_locked(h, &c)) || (rc = hide_apply_locked(h, c, HFPF_HIDE, nullptr, &k))) return bail(rc);
        if (k.n_bad) return bail(fail(h, HFPF_ERR_IO, "restore: the snapshot hides voxels that hold no row (%llu plane words); the handle has been cleared", k.n_bad));
    }
    if (h->binned) {
        // Entries the source's direct form appended since its last clean are still unchained; the binned form never runs
        // k_link_log at a clean pass (its own appends arrive chained), so they are chained here.
        LinkRanges lr;
        uint64_t max_new = 0;
        for (int r = 0; r < kLogRegions; r++) {
            const uint64_t base = (uint64_t)r * t.log_region_cap;
            lr.first[r] = (uint32_t)(base + h->ss.n_linked[r] + 1);
            lr.last[r] = (uint32_t)(base + u.log_n[r]);
            max_new = std::max(max_new, u.log_n[r] - h->ss.n_linked[r]);
        }
        if (max_new && (hd.flags & HFPF_FLAG_DIRECT_UPDATE)) {
            hipLaunchKernelGGL(k_link_log, dim3(blocks_for(max_new, 256), kLogRegions), dim3(256), 0, h->stream, h->t, lr);
            if (hipGetLastError() != hipSuccess) return bail(fail(h, HFPF_ERR_HIP, "restore: k_link_log launch failed"));
            for (int r = 0; r < kLogRegions; r++) h->ss.n_linked[r] = u.log_n[r];
            h->ss.direct_linked = h->h_ctr[C_BUFFERED];
        }
    }
    return HFPF_OK;
}

}  // namespace

extern "C" {

int hfpf_snapshot(hfpf_handle* h, void** blob, uint64_t* bytes)
{
    if (!h || !blob || !bytes) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    *blob = nullptr;
    *bytes = 0;
    return snapshot_locked(h, blob, bytes);
}

void hfpf_free_snapshot(void* blob) { free(blob); }

int hfpf_restore(hfpf_handle* h, const void* blob, uint64_t bytes)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    if (!blob) return fail(h, HFPF_ERR_BAD_ARG, "restore: null blob");
    return restore_locked(h, blob, bytes);
}

int hfpf_save(hfpf_handle* h, const char* path)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    if (!path) return fail(h, HFPF_ERR_BAD_ARG, "save: null path");
    void* blob = nullptr;
    uint64_t bytes = 0;
    if (int rc = snapshot_locked(h, &blob, &bytes)) return rc;
    FILE* f = fopen(path, "wb");
    if (!f) {
        free(blob);
        return fail(h, HFPF_ERR_IO, "save: cannot open %s for writing", path);
    }
    const bool wrote = fwrite(blob, 1, bytes, f) == bytes;
    const bool closed = fclose(f) == 0;
    free(blob);
    if (!wrote || !closed) {
        remove(path);  // no partial file is left behind
        return fail(h, HFPF_ERR_IO, "save: short write to %s", path);
    }
    return HFPF_OK;
}

int hfpf_load(hfpf_handle* h, const char* path)
{
    if (!h) return HFPF_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(h->mtx);
    if (!path) return fail(h, HFPF_ERR_BAD_ARG, "load: null path");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(h, HFPF_ERR_IO, "load: cannot open %s", path);
    uint8_t hdr[HFPF_SNAPSHOT_HEADER_BYTES];
    SnapHeader hd;
    if (fread(hdr, 1, sizeof hdr, f) != sizeof hdr) {
        fclose(f);
        return fail(h, HFPF_ERR_IO, "load: %s is shorter than a snapshot header", path);
    }
    if (const char* why = snap_parse_header(hdr, sizeof hdr, &hd)) {
        fclose(f);
        return fail(h, HFPF_ERR_BAD_ARG, "load: %s: %s", path, why);
    }
    uint8_t* blob = (uint8_t*)host_result_alloc(hd.total_bytes);
    if (!blob) {
        fclose(f);
        return fail(h, HFPF_ERR_CAPACITY, "load: host allocation of %llu bytes failed", (unsigned long long)hd.total_bytes);
    }
    memcpy(blob, hdr, sizeof hdr);
    const bool whole = fread(blob + sizeof hdr, 1, hd.payload_bytes, f) == hd.payload_bytes;
    fclose(f);
    int rc = whole ? restore_locked(h, blob, hd.total_bytes) : fail(h, HFPF_ERR_IO, "load: %s ends before the %llu bytes its header announces", path, (unsigned long long)hd.total_bytes);
    free(blob);
    return rc;
}

int hfpf_snapshot_info(const void* blob, uint64_t bytes, struct hfpf_snapshot_info* out)
{
    if (!blob || !out || out->struct_size != sizeof(struct hfpf_snapshot_info)) return HFPF_ERR_BAD_ARG;
    SnapHeader hd;
    if (snap_parse_header(blob, std::min<uint64_t>(bytes, HFPF_SNAPSHOT_HEADER_BYTES), &hd)) return HFPF_ERR_BAD_ARG;
    struct hfpf_snapshot_info o;
    memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.format_version = hd.version;
    o.layout_tag = hd.layout_tag;
    o.total_bytes = hd.total_bytes;
    o.payload_bytes = hd.payload_bytes;
    o.payload_checksum = hd.payload_checksum;
    o.resolution = hd.resolution;
    o.flags = hd.flags;
    memcpy(o.bbox, hd.bbox, sizeof o.bbox);
    o.k = hd.k, o.K = hd.K, o.gate = hd.gate;
    o.cylinder_radius = hd.cylinder_radius, o.ball_radius = hd.ball_radius, o.z_clip_min = hd.z_clip_min, o.z_clip_max = hd.z_clip_max;
    o.max_bricks = hd.need_bricks, o.max_log_points = hd.log_points, o.max_normals = hd.need_normals, o.max_frames = hd.need_frames;
    o.frames_integrated = hd.frames_integrated, o.clean_passes = hd.clean_passes, o.next_frame_id = hd.next_frame_id;
    o.voxels_occupied = hd.voxels_occupied, o.voxels_with_normal = hd.voxels_with_normal;
    *out = o;
    return HFPF_OK;
}

int hfpf_config_from_snapshot(const struct hfpf_snapshot_info* info, hfpf_config* cfg)
{
    if (!info || !cfg || info->struct_size != sizeof(struct hfpf_snapshot_info)) return HFPF_ERR_BAD_ARG;
    hfpf_default_config(cfg);
    cfg->resolution = info->resolution;
    memcpy(cfg->bbox, info->bbox, sizeof cfg->bbox);
    cfg->k = info->k, cfg->K = info->K, cfg->gate = info->gate;
    cfg->cylinder_radius = info->cylinder_radius, cfg->ball_radius = info->ball_radius;
    cfg->z_clip_min = info->z_clip_min, cfg->z_clip_max = info->z_clip_max;
    cfg->flags = info->flags & kSnapSemanticFlags;
    cfg->max_bricks = info->max_bricks, cfg->max_log_points = info->max_log_points, cfg->max_normals = info->max_normals, cfg->max_frames = info->max_frames;
    return HFPF_OK;
}

}  // extern "C"
