// Stand-alone host program for csrc/kfsp_dia_diag.h (tests/test_dia_diag_fold_host.py compiles it under AddressSanitizer /
// UBSan and drives it through stdin): the plan, the exact division, the tables, and the encode / decode round trip of DIAG
// folded into the spare bits of the coded banded records - the very functions the build and the product kernel call.
//   plan nd n w rec lds  d_0 .. d_{nd-1}
//       -> "plan 1 nk size.. stride.. toff.. ntab" or "plan 0"
//   div d q0 q1          -> "div ok" when dia_diag_div gives q / d for every q in [q0, q1) (and a few values below 2^31)
//   fold nd n ld w rec lds  d_0 .. d_{nd-1}  then ld 64-bit patterns (hexadecimal): DIAG of the ld rows the product computes
//       -> "fold 0 <first failing row>" or "fold 1", "tables <patterns>", "resid <ld integers>", "decode <patterns>"
//          (decode: what the kernel's steps give for every row from records whose low 48 bits are filled with noise)
#include "kfsp_dia_diag.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace kfsp;

static bool read_plan(int &nd, long long &n, int &w, int &rec, long long &lds, std::vector<int32_t> &delta, long long *ld)
{
    if (ld) {
        if (std::scanf("%d %lld %lld %d %d %lld", &nd, &n, ld, &w, &rec, &lds) != 6) return false;
    } else if (std::scanf("%d %lld %d %d %lld", &nd, &n, &w, &rec, &lds) != 5) {
        return false;
    }
    if (nd < 0 || nd > 64) return false;
    delta.assign((size_t)nd, 0);
    for (int d = 0; d < nd; ++d)
        if (std::scanf("%" SCNd32, &delta[(size_t)d]) != 1) return false;
    return true;
}

int main()
{
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        const std::string c = cmd;
        if (c == "plan") {
            int nd, w, rec;
            long long n, lds;
            std::vector<int32_t> delta;
            if (!read_plan(nd, n, w, rec, lds, delta, nullptr)) return 2;
            DiaDiagDev G;
            if (!dia_diag_plan(nd, delta.data(), n, w, rec, lds, &G)) {
                std::printf("plan 0\n");
                if (G.nk != 0 || G.ntab != 0) return 3;
                continue;
            }
            std::printf("plan 1 %d", G.nk);
            for (int k = 0; k < G.nk; ++k) std::printf(" %d", G.size[k]);
            for (int k = 0; k < G.nk; ++k) std::printf(" %d", G.stride[k]);
            for (int k = 0; k < G.nk; ++k) std::printf(" %d", G.toff[k]);
            std::printf(" %d\n", G.ntab);
        } else if (c == "div") {
            unsigned d, q0, q1;
            if (std::scanf("%u %u %u", &d, &q0, &q1) != 3 || d < 2) return 2;
            uint32_t magic;
            int32_t shift;
            dia_diag_magic(d, &magic, &shift);
            bool ok = shift >= 0;
            for (uint32_t q = q0; q < q1 && ok; ++q) ok = dia_diag_div(q, magic, shift) == q / d;
            for (uint32_t q = 0x7FFFFFFFu; q > 0x7FFFFFFFu - 100000u && ok; --q) ok = dia_diag_div(q, magic, shift) == q / d;
            for (uint64_t m = d; m < 0x80000000ull && ok; m += (uint64_t)d * 9973u) {      // around multiples of d
                const uint32_t q = (uint32_t)m;
                ok = dia_diag_div(q, magic, shift) == q / d && dia_diag_div(q - 1, magic, shift) == (q - 1) / d;
            }
            std::printf(ok ? "div ok\n" : "div wrong\n");
        } else if (c == "fold") {
            int nd, w, rec;
            long long n, lds, ld;
            std::vector<int32_t> delta;
            if (!read_plan(nd, n, w, rec, lds, delta, &ld) || ld < n || ld > (1 << 26)) return 2;
            std::vector<double> diag((size_t)ld);
            for (long long r = 0; r < ld; ++r) {
                uint64_t b;
                if (std::scanf("%" SCNx64, &b) != 1) return 2;
                diag[(size_t)r] = dia_diag_from_bits(b);
            }
            DiaDiagDev G;
            if (!dia_diag_plan(nd, delta.data(), n, w, rec, lds, &G)) {
                std::printf("fold 0 -1\n");
                continue;
            }
            // the tables, as k_dia_diag_tables makes them
            std::vector<double> tab((size_t)G.ntab);
            for (int k = 0; k < G.nk; ++k)
                for (int j = 0; j < G.size[k]; ++j) {
                    const int64_t r = (int64_t)j * G.stride[k];
                    tab[(size_t)(G.toff[k] + j)] = dia_diag_entry(k == G.nk - 1, r < n ? diag[(size_t)r] : 0.0, diag[0]);
                }
            // every row, as k_dia_diag_fold<false> checks it
            std::vector<uint64_t> field((size_t)ld);
            long long bad = -1;
            for (long long r = 0; r < ld && bad < 0; ++r)
                if (!dia_diag_encode(G, tab.data(), r, n, diag[(size_t)r], &field[(size_t)r])) bad = r;
            if (bad >= 0) {
                std::printf("fold 0 %lld\n", bad);
                continue;
            }
            std::printf("fold 1\ntables");
            for (double t : tab) std::printf(" %" PRIx64, dia_diag_bits(t));
            std::printf("\nresid");
            for (long long r = 0; r < ld; ++r) std::printf(" %lld", (long long)((int64_t)field[(size_t)r] >> kDiagFoldBit));
            // the records, as k_dia_diag_fold<true> writes them over codes (noise here), and the kernel's decode: row pairs,
            // the digits of the even row by division, of the odd row by increment
            std::vector<uint64_t> recs((size_t)ld);
            uint64_t s = 0x9E3779B97F4A7C15ull;
            for (long long r = 0; r < ld; ++r) {
                s = s * 6364136223846793005ull + 1442695040888963407ull;
                const uint64_t codes = s >> 16;
                recs[(size_t)r] = (codes & ((1ull << kDiagFoldBit) - 1ull)) | field[(size_t)r];
                if ((recs[(size_t)r] & ((1ull << kDiagFoldBit) - 1ull)) != codes) return 4;
            }
            std::printf("\ndecode");
            for (long long g = 0; g + 1 < ld + 1; g += 2) {
                int a0, a1, a2;
                dia_diag_digits(G, (uint32_t)g, a0, a1, a2);
                int b0 = a0, b1 = a1, b2 = a2;
                dia_diag_next(G, b0, b1, b2);
                const double x = dia_diag_value(dia_diag_predict(G, tab.data(), a0, a1, a2), recs[(size_t)g], g < n);
                std::printf(" %" PRIx64, dia_diag_bits(x));
                if (g + 1 < ld) {
                    const double y = dia_diag_value(dia_diag_predict(G, tab.data(), b0, b1, b2), recs[(size_t)g + 1], g + 1 < n);
                    std::printf(" %" PRIx64, dia_diag_bits(y));
                }
            }
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
