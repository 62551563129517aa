// The plan of k_bpe_merge_lds_pair (csrc/merge_pair_plan_core.hpp, compiled for the host exactly as the kernel compiles it), walked
// for every grid of GRIDS and pairs of fills from 0 to just past two rounds of that grid: EVERY pair for the grids up to 8; for 512
// the fills within 2 of a multiple of 64 (the plan changes nowhere else) at a stride, the borders of one and of two rounds and the fills
// of the flagship workload.  Every item of both queues must belong to exactly one (round, workgroup, lane): a unit's items are a range
// of its queue by construction, so every plan is checked for ranges that tile both queues and for a (round, workgroup) walk that meets
// every unit once, and the plans at the borders and a sample of the others are walked lane by lane as well.  A stand-alone program (tests/test_merge_pair_plan.py
// builds it with -fsanitize=address,undefined and runs it): prints the number of plans it checked and exits 0, or the first plan that
// is wrong and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "merge_pair_plan_core.hpp"

using namespace tkamd;

namespace {

long long g_checked = 0, g_lanes = 0, g_thin = 0, g_fallback = 0, g_two_rounds = 0;

#define PLAN_CHECK(cond)                                                                                                             \
    do {                                                                                                                             \
        if (!(cond)) {                                                                                                               \
            std::printf("FAILED %s: grid %u n16 %u n32 %u -> rounds %u take_l %u take_s %u units_l %u units %u\n", #cond, grid, n16, n32, \
                        p.rounds, p.take_l, p.take_s, p.units_l, p.units);                                                           \
            return false;                                                                                                            \
        }                                                                                                                            \
    } while (0)

bool check(uint32_t grid, uint32_t n16, uint32_t n32, bool lanes, std::vector<uint8_t>& seen_u, std::vector<uint8_t>& seen16, std::vector<uint8_t>& seen32) {
    const PairPlan p = pair_plan(n16, n32, grid);
    ++g_checked;
    const uint32_t need_l = (n32 + 319u) / 320u, need_s = (n16 + 639u) / 640u;
    PLAN_CHECK(p.rounds == (need_l + need_s + grid - 1u) / grid);                       // the fewest rounds that hold both queues at full units
    PLAN_CHECK(p.take_l % 64u == 0u && p.take_l >= 64u && p.take_l <= 320u);
    PLAN_CHECK(p.take_s % 64u == 0u && p.take_s >= 64u && p.take_s <= 640u);
    PLAN_CHECK(p.units_l <= p.units && (uint64_t)p.units <= (uint64_t)p.rounds * grid);  // units per round <= grid
    if (p.rounds > 1u) {                                                                // more than one round: full units
        PLAN_CHECK(p.take_l == 320u && p.take_s == 640u);
        ++g_two_rounds;
    }
    if (p.rounds == 1u && n32) {                                                        // thin long units whenever the free slots allow it
        const uint32_t free_slots = grid - need_s;
        if ((n32 + 255u) / 256u <= free_slots) { PLAN_CHECK(p.take_l <= 256u); ++g_thin; }
        else { PLAN_CHECK(p.take_l == 320u); ++g_fallback; }
        if (p.take_l > 64u) PLAN_CHECK((uint64_t)(p.take_l - 64u) * free_slots < n32);   // the smallest multiple of 64 that fits
    }
    // the units' ranges tile both queues, and the kernel's walk (round, workgroup) -> unit meets every unit exactly once
    PLAN_CHECK((uint64_t)p.units_l * p.take_l >= n32 && (n32 == 0u ? p.units_l == 0u : (uint64_t)(p.units_l - 1u) * p.take_l < n32));
    const uint32_t units_s = p.units - p.units_l;
    PLAN_CHECK((uint64_t)units_s * p.take_s >= n16 && (n16 == 0u ? units_s == 0u : (uint64_t)(units_s - 1u) * p.take_s < n16));
    seen_u.assign((size_t)p.rounds * grid, 0);
    for (uint32_t round = 0; round < p.rounds; ++round)
        for (uint32_t wg = 0; wg < grid; ++wg) {
            const uint32_t u = pair_plan_unit(round, wg, grid);
            PLAN_CHECK(u < p.rounds * grid && !seen_u[u]);
            seen_u[u] = 1;
        }
    if (!lanes) return true;
    ++g_lanes;
    // every item exactly once, lane by lane
    seen16.assign(n16, 0);
    seen32.assign(n32, 0);
    for (uint32_t round = 0; round < p.rounds; ++round) {
        for (uint32_t wg = 0; wg < grid; ++wg) {
            const uint32_t u = pair_plan_unit(round, wg, grid);
            PLAN_CHECK(u >= round * grid && u < (round + 1u) * grid);
            if (u < p.units_l) {
                for (uint32_t lane = 0; lane < p.take_l; ++lane) {
                    const uint64_t item = (uint64_t)u * p.take_l + lane;
                    if (item < n32) { PLAN_CHECK(!seen32[item]); seen32[item] = 1; }
                }
            } else if (u < p.units) {
                for (uint32_t lane = 0; lane < p.take_s; ++lane) {
                    const uint64_t item = (uint64_t)(u - p.units_l) * p.take_s + lane;
                    if (item < n16) { PLAN_CHECK(!seen16[item]); seen16[item] = 1; }
                }
            }
        }
    }
    for (uint32_t i = 0; i < n16; ++i) PLAN_CHECK(seen16[i]);
    for (uint32_t i = 0; i < n32; ++i) PLAN_CHECK(seen32[i]);
    return true;
}

}  // namespace

int main() {
    const uint32_t GRIDS[] = {1u, 2u, 3u, 8u, 512u};
    std::vector<uint8_t> seen_u, seen16, seen32;
    uint32_t k = 0, kb = 0;
    for (const uint32_t grid : GRIDS) {
        // the fills walked: all of them for a small grid; for the large one those around the multiples of 64 and a coarse stride
        const uint32_t max16 = 2u * grid * 640u + 70u, max32 = 2u * grid * 320u + 70u;
        std::vector<uint32_t> f16, f32;
        if (grid <= 8u) {
            for (uint32_t n = 0; n <= max16; ++n) f16.push_back(n);
            for (uint32_t n = 0; n <= max32; ++n) f32.push_back(n);
        } else {
            const uint32_t stride16 = 64u * 97u, stride32 = 64u * 41u;
            for (uint32_t n = 0; n <= max16; n += stride16) for (int d = -2; d <= 2; ++d) if ((int64_t)n + d >= 0) f16.push_back(n + d);
            for (uint32_t n = 0; n <= max32; n += stride32) for (int d = -2; d <= 2; ++d) if ((int64_t)n + d >= 0) f32.push_back(n + d);
            // (what a step of the flagship workload queues, and the borders of one round of the large grid)
            for (const uint32_t n : {263000u, 264960u, grid * 640u - 1u, grid * 640u, grid * 640u + 1u, max16}) f16.push_back(n);
            for (const uint32_t n : {19000u, 25344u, 25345u, grid * 320u - 1u, grid * 320u, grid * 320u + 1u, max32}) f32.push_back(n);
        }
        for (const uint32_t n16 : f16)
            for (const uint32_t n32 : f32) {
                const bool border = (n16 + 2u) % 64u <= 4u && (n32 + 2u) % 64u <= 4u;
                const bool lanes = grid <= 8u ? ((border && ++kb % 16u == 0u) || ++k % 8191u == 0u) : ++k % 997u == 0u;
                if (!check(grid, n16, n32, lanes, seen_u, seen16, seen32)) return 1;
            }
    }
    std::printf("ok: %lld plans, %lld of them lane by lane (%lld with thin long units, %lld at the 320 fallback, %lld of more than one round)\n", g_checked, g_lanes, g_thin, g_fallback, g_two_rounds);
    return (g_thin && g_fallback && g_two_rounds) ? 0 : 1;
}
