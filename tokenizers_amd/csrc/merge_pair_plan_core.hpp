// The plan of k_bpe_merge_lds_pair (kernels/bpe.hip): how a grid of workgroups splits itself between the <= 16-byte queue (units of the
// short role, up to 640 lanes) and the 17..32-byte queue (units of the long role, up to 320 lanes), derived from the two fills alone.
// Every workgroup computes the same plan on the device; one host+device function pair, so that the CPU test runs exactly what the
// kernel runs (tests/harness/merge_pair_plan_harness.cpp walks it exhaustively over small grids).
#pragma once
#include <cstdint>

#include "tables.hpp"

namespace tkamd {

constexpr uint32_t PAIR_TAKE_S_MAX = 640u;      // lanes of a workgroup: a short unit's words
constexpr uint32_t PAIR_TAKE_L_MAX = 320u;      // half of them: a long unit's words (32 keys a word where the short role has 16)
constexpr uint32_t PAIR_TAKE_L_THIN = 256u;     // four wavefronts, one per SIMD: no SIMD runs two chains of 32-symbol merges

struct PairPlan {
    uint32_t rounds;      // rounds of the grid (0: nothing queued)
    uint32_t take_l;      // items of a long unit (a multiple of 64, <= PAIR_TAKE_L_MAX)
    uint32_t take_s;      // items of a short unit (a multiple of 64, <= PAIR_TAKE_S_MAX)
    uint32_t units_l;     // units 0 .. units_l - 1 are long ones: unit u takes items [u * take_l, ..) of the long queue
    uint32_t units;       // units units_l .. units - 1 are short ones: unit u takes items [(u - units_l) * take_s, ..) of the short queue
};

TK_HD uint32_t pair_plan_up64(uint32_t x) { return (x + 63u) & ~63u; }

// n16 / n32: the fills of the short and of the long queue; grid >= 1.
//   More than one round of full units: full units, numbered long role first, so that only the workgroups the overflow is dealt to run
//   a second unit at all (profiles/pair_ab_c2.txt).
//   One round: the short role keeps the slots its full units need, the long role gets every other one and spreads its queue over them
//   in the thinnest whole wavefronts that fit -- at most PAIR_TAKE_L_THIN lanes, PAIR_TAKE_L_MAX only when the slots do not suffice --;
//   the short queue is then spread evenly over what the long units left.
TK_HD PairPlan pair_plan(uint32_t n16, uint32_t n32, uint32_t grid) {
    PairPlan p;
    const uint32_t need_l = (n32 + PAIR_TAKE_L_MAX - 1u) / PAIR_TAKE_L_MAX, need_s = (n16 + PAIR_TAKE_S_MAX - 1u) / PAIR_TAKE_S_MAX;   // full units
    const uint32_t need = need_l + need_s;
    p.rounds = (need + grid - 1u) / grid;
    p.take_l = PAIR_TAKE_L_MAX;
    p.take_s = PAIR_TAKE_S_MAX;
    if (p.rounds == 1u) {
        if (n32) {
            const uint32_t slots_l = grid - need_s;                                   // (>= need_l >= 1)
            const uint32_t thin = pair_plan_up64((n32 + slots_l - 1u) / slots_l);
            p.take_l = thin <= PAIR_TAKE_L_THIN ? thin : PAIR_TAKE_L_MAX;
        }
        const uint32_t units_l = (n32 + p.take_l - 1u) / p.take_l;                    // (<= slots_l)
        if (n16) {
            const uint32_t slots_s = grid - units_l;                                  // (>= need_s >= 1)
            const uint32_t even = pair_plan_up64((n16 + slots_s - 1u) / slots_s);
            p.take_s = even < PAIR_TAKE_S_MAX ? even : PAIR_TAKE_S_MAX;
        }
    }
    p.units_l = (n32 + p.take_l - 1u) / p.take_l;
    p.units = p.units_l + (n16 + p.take_s - 1u) / p.take_s;
    return p;
}

// The unit workgroup wg runs in a round (>= units: none).  The rounds alternate their direction: a second round goes first to the
// workgroups whose first unit was a short one.
TK_HD uint32_t pair_plan_unit(uint32_t round, uint32_t wg, uint32_t grid) {
    return round * grid + ((round & 1u) ? (grid - 1u - wg) : wg);
}

}  // namespace tkamd
