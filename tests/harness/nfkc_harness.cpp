// Stand-alone CPU harness for the K mode of tokenizers_amd/csrc/nfc_core.hpp (NFKC): over every document of a file it runs what the two
// passes of kernels/nfkc.hip run -- the COUNT pass byte by byte, each byte finding its segment backwards (nfc_seg_start) and taking its
// charge of the segment's output (nfc_charge_g<NFK_GROWTH>), as every lane does for itself; the WRITE pass head by head, each head
// emitting its whole segment -- and checks that the two agree: the charges of a segment's bytes sum to its output, no byte is charged
// more than NFK_GROWTH, the sum over a document is what the write pass emits, and that is HostModel::nfkc_normalize's length.
// Built by tests/test_nfkc.py with g++ (it has its own main; a sanitizer build needs nothing else).
// Input file: for every document a line "<n>\n" and then its n bytes.  Output: one line of totals; exit status 1 on any disagreement.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_model.hpp"
#include "nfc_core.hpp"

using namespace tkamd;

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: nfkc_harness <documents>\n"); return 2; }
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    HostModel hm;
    hm.build_nfkc();
    NfcTables t{hm.nfc_stage1.data(), hm.nfc_stage2.data(), hm.nfc_map.data(), hm.nfc_mask, hm.nfc_seed};
    t.lmap = hm.nfk_map.data(); t.lmap_mask = hm.nfk_mask; t.lmap_seed = hm.nfk_seed; t.kflat = hm.nfk_flat.data();
    long long n_docs = 0, n_refused = 0, n_bad = 0, src_bytes = 0, out_bytes = 0, n_segments = 0;
    long long len;
    NfcSeg g;
    while (fscanf(fh, "%lld", &len) == 1) {
        fgetc(fh);
        std::string s((size_t)len, '\0');
        if (len && fread(&s[0], 1, (size_t)len, fh) != (size_t)len) { fprintf(stderr, "short document\n"); return 2; }
        ++n_docs;
        const int64_t n = len;
        std::vector<uint8_t> buf((size_t)n + 64, 0);
        memcpy(buf.data(), s.data(), (size_t)n);
        const uint8_t* text = buf.data();
        std::vector<nfc_mask_t> bound((size_t)(n >> 6) + 2, 0ull);
        bound[0] = 1ull;
        // the write pass: every head its whole segment
        long long written = 0;
        bool refused = false;
        std::vector<long long> seg_out((size_t)n + 1, -1), seg_end((size_t)n + 1, -1);
        for (int64_t p = 0; p < n;) {
            uint32_t l;
            const uint32_t f = nfc_flags(t, nfc_decode(text, n, p, &l));
            if (nfc_trivial<true>(t, text, n, bound.data(), p, f, l)) { seg_out[p] = l; seg_end[p] = p + l; written += l; p += l; ++n_segments; continue; }
            if (!nfc_segment<true>(t, text, n, bound.data(), p, g)) { refused = true; break; }
            seg_out[p] = g.obytes; seg_end[p] = g.e; written += g.obytes; p = g.e; ++n_segments;
        }
        if (refused) { ++n_refused; continue; }
        // the count pass: every byte for itself
        long long counted = 0;
        bool bad = false;
        for (int64_t i = 0; i < n && !bad; ++i) {
            const int64_t h = nfc_seg_start<true>(t, text, n, bound.data(), nfc_unit_start(text, n, i));
            if (h < 0 || seg_out[h] < 0 || i >= seg_end[h]) { bad = true; break; }
            const uint32_t c = nfc_charge_g<NFK_GROWTH>((uint32_t)(i - h), (uint32_t)seg_out[h], (uint32_t)(seg_end[h] - h));
            if (c > NFK_GROWTH) bad = true;
            counted += c;
        }
        bool r2 = false;
        const std::string o = hm.nfkc_normalize(s, nullptr, &r2);
        if (bad || r2 || counted != written || written != (long long)o.size() || written > (long long)NFK_GROWTH * n) {
            ++n_bad;
            fprintf(stderr, "document %lld (%lld bytes): counted %lld, written %lld, normalized %zu\n", n_docs - 1, len, counted, written, o.size());
        }
        src_bytes += n;
        out_bytes += written;
    }
    fclose(fh);
    printf("documents %lld refused %lld bad %lld segments %lld source_bytes %lld output_bytes %lld\n", n_docs, n_refused, n_bad, n_segments, src_bytes, out_bytes);
    return n_bad ? 1 : 0;
}
