// String::from_utf8_lossy (what the ByteLevel decoder ends with, pre_tokenizers/byte_level.rs:170) as a decision per byte: every
// maximal invalid subpart of a byte string becomes one U+FFFD (EF BF BD), everything else is copied.  A byte therefore contributes
// 1 byte (it is part of a well-formed character), 3 bytes (it starts an invalid subpart) or nothing (it is a later byte of one).
// The decision is local: a byte that is no continuation byte (anything but 80..BF) always starts a unit, and a continuation byte
// belongs to the unit of the nearest such byte at most 3 positions back iff that byte is a lead (C2..F4) whose sequence is still
// well-formed through this position -- else it is a unit of its own.  Neither direction looks past [lo, hi), the byte range of one
// decoded sequence.  One host+device function, so that the CPU tests (tkamd_probe_utf8_lossy, tests/test_utf8_lossy.py) run exactly
// what k_lossy_count / k_lossy_len run.
#pragma once
#include <cstdint>

#include "tables.hpp"

namespace tkamd {

// continuation bytes the lead byte b asks for; 0: b is no lead (ASCII, a continuation byte, C0, C1, F5..FF)
TK_HD uint32_t utf8_lossy_need(uint32_t b) {
    if (b >= 0xC2u && b <= 0xDFu) return 1u;
    if (b >= 0xE0u && b <= 0xEFu) return 2u;
    if (b >= 0xF0u && b <= 0xF4u) return 3u;
    return 0u;
}

// is c well-formed as the k-th byte (k >= 1) behind `lead`?  The first one is restricted behind E0 (no overlong forms), ED (no
// surrogates), F0 (no overlong forms) and F4 (nothing above U+10FFFF) -- the automaton of utf8_step (kernels/decode.hip).
TK_HD bool utf8_lossy_cont_ok(uint32_t lead, uint32_t k, uint32_t c) {
    uint32_t lo = 0x80u, hi = 0xBFu;
    if (k == 1u) {
        if (lead == 0xE0u) lo = 0xA0u;
        else if (lead == 0xEDu) hi = 0x9Fu;
        else if (lead == 0xF0u) lo = 0x90u;
        else if (lead == 0xF4u) hi = 0x8Fu;
    }
    return c >= lo && c <= hi;
}

// bytes that s[i] contributes to the repaired text of the sequence s[lo .. hi): 1, 3 (U+FFFD is written in its place) or 0
TK_HD uint32_t utf8_lossy_len(const uint8_t* s, int64_t i, int64_t lo, int64_t hi) {
    const uint32_t b = s[i];
    if (b < 0x80u) return 1u;
    int64_t start = i;                                         // first byte of the unit s[i] belongs to
    if (b <= 0xBFu) {
        for (int64_t j = i - 1; j >= lo && j >= i - 3; --j) {
            const uint32_t c = s[j];
            if (c >= 0x80u && c <= 0xBFu) continue;
            const uint32_t need = utf8_lossy_need(c);          // the nearest byte that is no continuation byte
            bool ok = (uint32_t)(i - j) <= need;
            for (int64_t q = j + 1; ok && q <= i; ++q) ok = utf8_lossy_cont_ok(c, (uint32_t)(q - j), s[q]);
            if (ok) start = j;
            break;
        }
        if (start == i) return 3u;                             // a continuation byte no lead reaches
    }
    const uint32_t lead = s[start], need = utf8_lossy_need(lead);
    if (need == 0u) return 3u;                                 // C0, C1, F5..FF
    uint32_t have = 0u;                                        // well-formed continuation bytes behind the lead
    while (have < need && start + 1 + have < hi && utf8_lossy_cont_ok(lead, have + 1u, s[start + 1 + have])) ++have;
    if (have == need) return 1u;
    return start == i ? 3u : 0u;
}

}  // namespace tkamd
