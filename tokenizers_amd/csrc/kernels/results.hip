// Part of kernels.hip (ONE translation unit: this file is #included there, inside namespace tkamd, after the shared
// helpers; it is not compiled on its own).  How the model kernels hand their tokens to the compaction.

// =================================================================================================
// Result layout between Model::tokenize and into_encoding (replaces the Vec<Token> every Split carries,
// tokenizer/pre_tokenizer.rs:22-47):
//   tok0[p]   one word per pre-token:  TOK_ONE | id            exactly one token (settled by the lookup kernel)
//                                      TOK_ROW | row            the tokens are in rows[row]        (30 bits of row)
//                                      TOK_SLOT | slot          the tokens are in the row of a claimed / cached slot (both flag bits; kernels/lookup.hip)
//   rows[r]   16 bytes per QUEUED pre-token, named by the queue position the lookup kernel gave it (so the model kernels
//             never touch the P-sized arrays):   { id0 | count << 28, id1, id2, id3 }                 count <= 4
//                                                { id0 | 15 << 28, s, count, 0 }                      any count: ids 1.. in
//             tmp_ids[s + j] -- s is the pre-token's first byte; a pre-token of L bytes has at most L tokens, so the slots
//             s+1 .. s+L-1 of a 4-byte-per-text-byte array belong to it alone.
//   tmp_end[s + j]  (only when offsets are requested) end of token j, in bytes from the pre-token start.
// Token ids are < 2^24 (checked at load), so the flag / count bits never collide with an id.
// =================================================================================================
constexpr uint32_t TOK_ROW = 0x80000000u;
constexpr uint32_t TOK_ONE = 0x40000000u;
constexpr uint32_t TOK_ID_MASK = 0x00FFFFFFu;
constexpr uint32_t TOK_SLOT = TOK_ROW | TOK_ONE, TOK_REF_MASK = 0x3FFFFFFFu;
constexpr uint32_t ROW_CNT_SHIFT = 28, ROW_CNT_MORE = 15u, ROW_ID_MASK = 0x0FFFFFFFu;
constexpr uint32_t ROW_WHOLE_WORD = 0xFFFFFFFFu;      // word 1 of a ONE-token row (unused otherwise): a whole-word vocabulary hit of k_long_vocab, not a merge result (k_token_meta)

// one queued pre-token: first byte and length (the model kernels need nothing else).  Bit 31 of the length: this entry HOLDS the in-batch
// claim of its word (kernels/lookup.hip) -- the model kernel that finishes it also copies its row to the claimed slot's row, where
// the compaction finds it for the word's other occurrences.  Every reader takes the length through qitem_len().
struct __attribute__((aligned(8))) QItem { uint32_t s, len; };
constexpr uint32_t QLEN_CLAIM = 0x80000000u;
__device__ __forceinline__ uint32_t qitem_len(uint32_t len_word) { return len_word & ~QLEN_CLAIM; }

// A work queue is NSQ sub-queues of sq_cap entries each.  Atomics on ONE address serialise at ~10 ns each on MI355X (device-scope
// atomics are resolved at the memory side), and a shared fill counter would take one per workgroup, tile and queue -- tens of
// thousands per batch.  Instead lookup workgroup b owns sub-queue b outright and writes its fill once, at the end; the
// consumers see the sub-queues laid end to end (qview_*).  Position p = sub-queue * sq_cap + index names the queue entry and,
// with row_base, the result row.
// (struct QView / NSQ / QCNT_STRIDE: kernels.hpp)
// all threads of the workgroup: loads the fill counts, leaves their prefix sums in s_pre[NSQ + 1], returns the total
__device__ __forceinline__ uint32_t qview_prefix(const QView& v, uint32_t* s_pre) {
    constexpr int PER = NSQ / 64;                           // one wavefront scans the counts, PER consecutive ones per lane
    static_assert(NSQ % 64 == 0, "sub-queues per lane");
    __syncthreads();
    if (threadIdx.x < 64) {
        uint32_t c[PER], sum = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) { c[k] = min(v.counts[(threadIdx.x * PER + k) * QCNT_STRIDE], v.sq_cap); sum += c[k]; }
        uint32_t run = wave_incl_scan(sum) - sum;
#pragma unroll
        for (int k = 0; k < PER; ++k) { run += c[k]; s_pre[threadIdx.x * PER + k + 1] = run; }
        if (threadIdx.x == 0) s_pre[0] = 0u;
    }
    __syncthreads();
    return s_pre[NSQ];
}
// the queue position of the item-th entry of the concatenated sub-queues (item < total)
__device__ __forceinline__ uint32_t qview_pos(const uint32_t* s_pre, uint32_t sq_cap, uint32_t item) {
    uint32_t lo = 0, hi = NSQ;                              // invariant: s_pre[lo] <= item < s_pre[hi]
#pragma unroll
    for (int it = 0; it < 10; ++it) {
        static_assert(NSQ <= 1024, "binary search depth");
        const uint32_t mid = (lo + hi) >> 1;
        if (hi - lo > 1) { if (s_pre[mid] <= item) lo = mid; else hi = mid; }
    }
    return lo * sq_cap + (item - s_pre[lo]);
}

__device__ __forceinline__ uint32_t row_count(const uint4& row) {
    const uint32_t cf = row.x >> ROW_CNT_SHIFT;
    return cf < ROW_CNT_MORE ? cf : row.z;
}
// up to four tokens held in registers; beyond four the caller has written ids 1.. to tmp_ids[s + j] itself
// (round 6) Token ENDS in the row.  With offsets requested, a row of two to four tokens of a pre-token of <= 32 bytes carries the boundary
// in front of token j (1..3) in the top byte of its word j (ids are < 2^24): position in the pre-token (1..31, five bits) and -- byte-level
// tokens may cut a multi-byte char, whose whole range both neighbours then report (byte_level.rs:135-143) -- how far the token that
// starts there snaps back and the one that ends there snaps forward (three bits: 0 = a char boundary; 1..6 = (back, fwd) of a cut at
// byte k of a char of L bytes: (1,1) (1,2) (2,1) (1,3) (2,2) (3,1)).  The compaction hands the byte on, one per token, next to the ids
// (tok_b8: a dense array), and k_token_meta reads its neighbours' instead of a sparse array indexed by byte position, a claimant's
// place behind tok0 -> claim_pos and the text at every cut (kernels/output.hip).  0 = not carried: token_meta takes the old way.
// The byte of token 0 is B8_FIRST, put there by the compaction: the set of them is token_meta's map from tokens to pre-tokens.
constexpr uint32_t ROW_B8_SHIFT = 24;
constexpr uint32_t B8_FIRST = 0xE0u;                  // the byte of a pre-token's FIRST token in tok_b8 (no boundary looks like it: position 0, code 7) -- the compaction's marker
__device__ __forceinline__ uint32_t row_boundary(const uint8_t* __restrict__ text, uint32_t s, uint32_t pos, bool snap) {
    uint32_t code = 0u;
    if (snap && (text[s + pos] & 0xC0u) == 0x80u) {       // (the pre-token starts and ends on char boundaries: the walks stay inside it)
        uint32_t back = 1u, fwd = 1u;
        while (back < 3u && (text[s + pos - back] & 0xC0u) == 0x80u) ++back;
        while (fwd < 3u && (text[s + pos + fwd] & 0xC0u) == 0x80u) ++fwd;
        code = back == 1u ? (fwd == 1u ? 1u : fwd == 2u ? 2u : 4u) : back == 2u ? (fwd == 1u ? 3u : 5u) : 6u;
    }
    return (pos | (code << 5)) << ROW_B8_SHIFT;
}
// (two bits a code, looked up in a constant: code 0 -> 0; (back, fwd) of codes 1..6 as listed above)
__device__ __forceinline__ uint32_t b8_back(uint32_t v) { return (0x3994u >> ((v >> 5) * 2u)) & 3u; }
__device__ __forceinline__ uint32_t b8_fwd(uint32_t v) { return (0x1B64u >> ((v >> 5) * 2u)) & 3u; }

__device__ __forceinline__ uint4 make_row(uint32_t count, uint32_t s, uint32_t id0, uint32_t id1, uint32_t id2, uint32_t id3) {
    return count <= 4u ? make_uint4(id0 | (count << ROW_CNT_SHIFT), id1, id2, id3) : make_uint4(id0 | (ROW_CNT_MORE << ROW_CNT_SHIFT), s, count, 0u);
}

// =================================================================================================
// Single-pass prefix sums from published TOTALS: chunk c publishes its own total as soon as it knows it; whoever needs the sum of a
// range of chunks adds up their published totals.  Nothing else is ever published -- no inclusive prefix that only exists once its
// chunk has itself resolved, so no chain of device-scope round trips down the chunks (rounds 3 to 6 walked back to the nearest such
// prefix: HISTORY.md).  A workgroup that takes the chunks c, c + G, c + 2G, ... in order carries its own inclusive prefix forward:
//   base(c + G) = incl(c) + sum of total(j), c < j < c + G,
// every term of which a front() published long before it is asked for.
// Two kinds of word, all accesses device-scope atomics (the L2 of one XCD is not coherent with the others'):
//   state[c]     LB_AGG | total of chunk c; 0 = not yet published.  State and value in ONE word: a reader never sees one without the other.
//   group word g (lb_group_word) count << 56 | sum of the totals of the chunks [64 g, 64 g + 64) whose OWNERS have published.  A reader
//                takes it only when the count is 64 (the whole group in one load: G - 1 totals are G / 64 of these and two partial
//                windows of state[] -- three loads a lane at any grid up to 4,096); otherwise it reads the group's 64 state words.
// A wait never depends on another workgroup being scheduled: a chunk's total is a pure function of data that is final before the
// kernel starts, so a wavefront that has polled an unpublished total `patience` times computes it itself (`help`) and publishes it on
// the owner's behalf -- into state[] ALONE, by compare-and-swap from "nothing", so an owner that got there first wins, and either way
// the word holds the same value.  Only owners add to a group word: it is never counted twice.
// The group words are LB_GROUP_STRIDE words apart (kernels.hpp): device-scope atomics execute at the memory side, those on one 64-byte
// block one after the other (~11 ns each, MI355X), and the ~20 groups in flight at once take 18 k adds a C2 batch between them.
// (Measured: the words packed eight to a block, k_compact 0.315 ms at C2 against 0.0915 -- profiles/compact_carry_ab_c2.txt.)
// =================================================================================================
constexpr unsigned long long LB_AGG = 1ull << 62, LB_VALUE = LB_AGG - 1ull;
constexpr int LB_GCOUNT_SHIFT = 56;                 // a group's sum stays below 2^40: 64 totals of less than 2^32
constexpr unsigned long long LB_GSUM = (1ull << LB_GCOUNT_SHIFT) - 1ull;
static_assert(LB_GROUP_CHUNKS == 64, "one wavefront-wide load reads a group's states");

__device__ __forceinline__ void lb_store(unsigned long long* p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long lb_load(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the group words of a batch of n_chunks chunks: behind its state words, in the same allocation (the host sizes and zeroes both: lb_state_words)
__device__ __forceinline__ unsigned long long* lb_groups(unsigned long long* state, int64_t n_chunks) { return state + lb_group_base((size_t)n_chunks); }
__device__ __forceinline__ unsigned long long* lb_group_word(unsigned long long* groups, int64_t g) { return groups + g * LB_GROUP_STRIDE; }
// Two halves, so that a workgroup can publish a chunk's total early and come back for its place after other work:
//   lb_publish(state, groups, ch, total)   one lane, the chunk's OWNER: total of chunk ch is known
//   lb_resolve(state, groups, prev, ch, patience, help, pre)
//                                  ONE whole wavefront: returns, in every lane, the sum of the totals of the chunks prev < j < ch (prev = -1:
//                                  of all chunks before ch).  help(c): called by the whole wavefront, returns chunk c's total in every lane.
__device__ __forceinline__ void lb_publish(unsigned long long* __restrict__ state, unsigned long long* __restrict__ groups, int64_t ch, unsigned long long total) {
    lb_store(&state[ch], LB_AGG | total);
    atomicAdd(lb_group_word(groups, ch / LB_GROUP_CHUNKS), (1ull << LB_GCOUNT_SHIFT) | total);      // (result unused: a no-return add, nobody waits for it)
}
constexpr uint32_t LB_PATIENCE = 1024;              // polls of an unpublished total before it is computed here (about half a millisecond; TKAMD_LB_PATIENCE)

// The range (prev, ch) cut at the multiples of 64: a partial group at the front [lo, fe), whole groups [gl, gh), a partial group at the
// back [64 gh, hi).  (No multiple of 64 inside the range: everything is "front".)
struct LbCut { int64_t lo, fe, gl, gh, hi; };
__device__ __forceinline__ LbCut lb_cut(int64_t prev, int64_t ch) {
    LbCut c;
    c.lo = prev + 1;
    c.hi = ch;
    c.gl = (c.lo + LB_GROUP_CHUNKS - 1) / LB_GROUP_CHUNKS;
    c.gh = max(ch / LB_GROUP_CHUNKS, c.gl);
    c.fe = min(c.gl * LB_GROUP_CHUNKS, ch);
    return c;
}
// The first read of all three parts, taken EARLY: one load per part and lane, all in flight together, no wait -- the front window upwards
// from lo, the first 64 group words, the back window downwards from hi - 1.  A state word goes from nothing to a total and never changes
// after that, and a group word is used only when its count is 64 -- complete, it never changes again either --, so a value read early is
// still true when it is used; what the early read does not settle, lb_resolve reads again fresh.
// (How wide an early read may be: sessions S / T, profiles/r5s_*, r5t_*, on the look-back of rounds 4 to 6: two, three and four loads a
// lane level, eight slower than none -- eight device-scope loads a chunk are traffic of their own.)
struct LbPre { unsigned long long a, g, b; };
__device__ __forceinline__ void lb_prefetch(unsigned long long* __restrict__ state, unsigned long long* __restrict__ groups, int64_t prev, int64_t ch, LbPre& p) {
    const int lane = lane_id();
    const LbCut c = lb_cut(prev, ch);
    p.a = c.lo + lane < c.fe ? lb_load(&state[c.lo + lane]) : 0ull;
    p.g = c.gl + lane < c.gh ? lb_load(lb_group_word(groups, c.gl + lane)) : 0ull;
    p.b = c.hi - 1 - lane >= c.gh * LB_GROUP_CHUNKS ? lb_load(&state[c.hi - 1 - lane]) : 0ull;
}
// One window of up to 64 state words -- lane l: chunk first + step * l, l < n; `st`: that word as last read (0: not published then).
// Returns the lane's total once every chunk of the window has one: polls the missing ones, and out of patience computes one of them here.
struct LbWait { uint32_t patience, polls; };
template <class Help>
__device__ __forceinline__ unsigned long long lb_window(unsigned long long* __restrict__ state, int64_t first, int step, int n, unsigned long long st, LbWait& w, Help&& help) {
    const int lane = lane_id();
    const bool want = lane < n;
    const int64_t idx = first + (int64_t)step * lane;
    uint64_t empty;
    while ((empty = __ballot(want && st == 0ull)) != 0ull) {
        if (++w.polls > w.patience) {                               // (wavefront-uniform) out of patience: one of the missing totals is computed here
            // (different workgroups pick different ones; having helped once, this look-back goes on helping without the long pause)
            int k = (int)((blockIdx.x + w.polls) % (uint32_t)__popcll((unsigned long long)empty));
            uint64_t e = empty;
            for (; k > 0; --k) e &= e - 1ull;
            const int64_t hc = first + (int64_t)step * (__ffsll((unsigned long long)e) - 1);
            const unsigned long long t = help(hc);
            if (lane == 0) atomicCAS(&state[hc], 0ull, LB_AGG | t);
            w.patience = 8u;
            w.polls = 0u;
        }
        if (want && st == 0ull) st = lb_load(&state[idx]);
    }
    return want ? (st & LB_VALUE) : 0ull;
}
template <class Help>
__device__ __forceinline__ unsigned long long lb_resolve(unsigned long long* __restrict__ state, unsigned long long* __restrict__ groups, int64_t prev, int64_t ch,
                                                         uint32_t patience, Help&& help, const LbPre& p) {
    const int lane = lane_id();
    const LbCut c = lb_cut(prev, ch);
    LbWait w{patience, 0u};
    // every part's share of this lane first, ONE sum over the lanes behind them (the branches are wavefront-uniform)
    unsigned long long acc = lb_window(state, c.lo, 1, (int)(c.fe - c.lo), p.a, w, help);
    acc += lb_window(state, c.hi - 1, -1, (int)(c.hi - c.gh * LB_GROUP_CHUNKS), p.b, w, help);
    for (int64_t g0 = c.gl; g0 < c.gh; g0 += 64) {                  // (one round up to a grid of 4,096; the early read is the first round's)
        const bool want = g0 + lane < c.gh;
        unsigned long long gw = g0 == c.gl ? p.g : 0ull;
        if (want && (gw >> LB_GCOUNT_SHIFT) != (unsigned long long)LB_GROUP_CHUNKS) gw = lb_load(lb_group_word(groups, g0 + lane));      // not complete when read early: once more, fresh
        const bool whole = (gw >> LB_GCOUNT_SHIFT) == (unsigned long long)LB_GROUP_CHUNKS;
        acc += want && whole ? (gw & LB_GSUM) : 0ull;
        // still short of an owner (or it never will be complete in time: its owners are not resident): the group's 64 state words, helpers' included
        for (uint64_t m = __ballot(want && !whole); m; m &= m - 1ull) {
            const int64_t gx = g0 + (__ffsll((unsigned long long)m) - 1);
            const unsigned long long st = lb_load(&state[gx * LB_GROUP_CHUNKS + lane]);
            acc += lb_window(state, gx * LB_GROUP_CHUNKS, 1, LB_GROUP_CHUNKS, st, w, help);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    return acc;
}

// (Round 4 also tried the look-back by the whole 256-lane workgroup, four windows of 64 predecessors a round: two barriers a round
// cost more than the shorter walk saved -- k_compact 0.152 ms against 0.143 ms on C2, profiles/r4g_ab_c2.txt.)
