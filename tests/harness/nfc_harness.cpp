// CPU harness for tokenizers_amd/csrc/nfc_core.hpp: normalizes a batch of strings (each one piece) with the core the kernels run --
// HostModel::nfc_normalize over the tables of nfc_tables.inc -- and runs the quick check of kernels/nfc.hip k_nfc_check lane by lane
// over each of them.  Built as a shared library by tests/test_nfc.py, which holds both against the reference wheel.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "host_model.hpp"
#include "nfc_core.hpp"

using namespace tkamd;

namespace {
HostModel& model() {
    static HostModel hm = [] { HostModel m; m.build_nfc(); return m; }();
    return hm;
}
}  // namespace

extern "C" {

// documents [off[d], off[d + 1]) of text; out / out_off: the normalized documents as a CSR (out holds out_cap bytes); norig: per output
// byte the first byte of the source char it is aligned to, relative to its document; status[d]: 1 = refused (a segment beyond 48), 2 =
// the quick check says "not known to be NFC" (the document laid out behind d % 16 ASCII bytes, so that its lanes fall differently).
// Returns the bytes written, or -1 if out_cap is too small.
int64_t nfch_normalize_batch(const uint8_t* text, const int64_t* off, int64_t count, uint8_t* out, int64_t out_cap, int64_t* out_off, uint32_t* norig,
                             uint8_t* status) {
    const HostModel& hm = model();
    const NfcTables t{hm.nfc_stage1.data(), hm.nfc_stage2.data(), hm.nfc_map.data(), hm.nfc_mask, hm.nfc_seed};
    int64_t w = 0;
    std::vector<uint32_t> al;
    std::vector<uint8_t> buf;
    for (int64_t d = 0; d < count; ++d) {
        const std::string s((const char*)text + off[d], (size_t)(off[d + 1] - off[d]));
        bool refused = false;
        const std::string o = hm.nfc_normalize(s, &al, &refused);
        out_off[d] = w;
        if (w + (int64_t)o.size() > out_cap) return -1;
        memcpy(out + w, o.data(), o.size());
        if (norig) memcpy(norig + w, al.data(), al.size() * 4);
        w += (int64_t)o.size();
        uint8_t st = refused ? 1 : 0;
        const int64_t shift = d % 16, n = shift + (int64_t)s.size();
        buf.assign((size_t)n + 64, 'x');
        memcpy(buf.data() + shift, s.data(), s.size());
        for (int64_t i0 = 0; i0 < n; i0 += NFC_LANE)
            if (nfc_check_lane(t, buf.data(), n, i0)) st |= 2;
        status[d] = st;
    }
    out_off[count] = w;
    return w;
}

}  // extern "C"
