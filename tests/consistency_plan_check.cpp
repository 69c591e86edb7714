// tests/consistency_plan_check.cpp -- plan_consistency (csrc/host_plan.hpp) as a program of its own: whatever the rows, frames,
// compute units and forced chunk length, walking the launches and chunks the way consistency_span_locked and k_consistency do covers
// every frame exactly once, with chunks of 1..64 frames and launches of at most 32768 chunks.
#include <cstdio>
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

static void walk(uint64_t rows, uint32_t frames, uint32_t cus, uint32_t forced)
{
    const ConsPlan p = plan_consistency(rows, frames, cus, forced);
    CHECK(p.frames_per_chunk >= 1 && p.frames_per_chunk <= kConsChunkFrames);
    CHECK(p.chunks_per_launch >= 1 && p.chunks_per_launch <= kConsLaunchChunks);
    CHECK((uint64_t)p.n_chunks * p.frames_per_chunk >= frames);
    CHECK(frames == 0 ? p.n_chunks == 0 : (uint64_t)(p.n_chunks - 1) * p.frames_per_chunk < frames);  // no empty chunk
    CHECK(p.single == (p.n_chunks <= 1));
    if (forced) CHECK(p.frames_per_chunk == std::min(forced, kConsChunkFrames));
    std::vector<uint8_t> seen(frames, 0);
    uint32_t launches = 0;
    for (uint32_t c0 = 0; c0 < p.n_chunks; c0 += p.chunks_per_launch, launches++) {
        const uint32_t nc = std::min(p.chunks_per_launch, p.n_chunks - c0);  // grid.y of this launch
        CHECK(nc >= 1);
        for (uint32_t y = 0; y < nc; y++) {
            const uint32_t f0 = (c0 + y) * p.frames_per_chunk;  // k_consistency's
            CHECK(f0 < frames);
            if (f0 >= frames) continue;
            const uint32_t nf = std::min(p.frames_per_chunk, frames - f0);
            CHECK(nf >= 1);
            for (uint32_t f = f0; f < f0 + nf; f++) seen[f]++;
        }
    }
    for (uint32_t f = 0; f < frames; f++) CHECK(seen[f] == 1);
    CHECK(launches == (p.n_chunks + p.chunks_per_launch - 1) / p.chunks_per_launch);
}

int main()
{
    const uint64_t rows[] = {0, 1, 255, 256, 257};
    const uint32_t frames[] = {0, 1, 63, 64, 65, 130};
    const uint32_t cus[] = {0, 1, 256};
    const uint32_t forced[] = {0, 1, 2, 64};
    for (uint64_t r : rows)
        for (uint32_t f : frames)
            for (uint32_t c : cus)
                for (uint32_t k : forced) walk(r, f, c, k);
    // many rows: whole chunks of 64; few rows on a large device: shorter chunks, more workgroups
    CHECK(plan_consistency(1u << 20, 130, 256).frames_per_chunk == 64 && plan_consistency(1u << 20, 130, 256).n_chunks == 3);
    CHECK(plan_consistency(1u << 20, 64, 256).single);
    CHECK(plan_consistency(257, 130, 256).frames_per_chunk == 1);   // 2 tiles, 1024 workgroups wanted: 512 chunks wanted, 130 frames
    CHECK(plan_consistency(16128, 120, 256).frames_per_chunk == 8); // 63 tiles: 17 chunks wanted, ceil(120 / 17) = 8
    CHECK(plan_consistency(16128, 120, 256).n_chunks == 15 && !plan_consistency(16128, 120, 256).single);
    CHECK(plan_consistency(100, 130, 256, 64).n_chunks == 3 && plan_consistency(100, 130, 256, 1).n_chunks == 130);
    // the largest call: 2^20 frames one per chunk leave in 32 launches
    walk(1, 1u << 20, 256, 1);
    CHECK(plan_consistency(1, 1u << 20, 256, 1).chunks_per_launch == kConsLaunchChunks);
    walk(0xFFFFFFFEull, 1u << 20, 304, 0);
    if (g_fail) return 1;
    printf("consistency_plan ok\n");
    return 0;
}
