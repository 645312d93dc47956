// Stand-alone CPU program around csrc/amt_flac_lpc_core.h, the analysis the FLAC frame kernel compiles: built by
// tests/test_flac_lpc_cpu.py with -ffp-contract=off and the address and undefined-behaviour sanitizers, and compared value
// for value with the numpy restatement (tests/flac_lpc_reference.py).
//
//   flac_lpc_host_main FILE
//
// FILE: "FLP1", int32 records, then per record (all int32, little-endian)
//   kind 0 (analysis):  0, bps, max_order, bs, bs samples
//       -> "R l0 l1 ... l12" and per order m = 1 .. max_order "m shift c_0 .. c_(m-1)" or "m -"
//   kind 1 (residual):  1, bs, bs samples, m, shift, m coefficients
//       -> "resid min max ok": the smallest and largest residual over i = m .. bs - 1, ok = 1 if none is disqualified
#include <cstdint>
#include <cstdio>
#include <vector>

#include "amt_flac_lpc_core.h"

static bool get(FILE *f, int32_t *v, size_t n) { return fread(v, sizeof(int32_t), n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    char magic[4];
    int32_t records = 0;
    if (fread(magic, 1, 4, f) != 4 || magic[0] != 'F' || magic[1] != 'L' || magic[2] != 'P' || magic[3] != '1' ||
        !get(f, &records, 1))
        return 3;
    for (int32_t rec = 0; rec < records; ++rec) {
        int32_t kind;
        if (!get(f, &kind, 1)) return 3;
        if (kind == 0) {
            int32_t h[3];
            if (!get(f, h, 3)) return 3;
            const int bps = h[0], max_order = h[1], bs = h[2];
            if ((bps != 16 && bps != 24) || max_order < 0 || max_order > FLL_MAX_ORDER || bs < 1 || bs > 65536) return 4;
            std::vector<int32_t> q(bs), x(bs);
            if (!get(f, q.data(), bs)) return 3;
            for (int i = 0; i < bs; ++i) x[i] = fll_windowed(q[i], i, bs);
            fll_i64 R[FLL_LAGS];
            for (int l = 0; l < FLL_LAGS; ++l) {
                R[l] = 0;
                for (int i = l; i < bs; ++i) R[l] += (fll_i64)x[i] * x[i - l];
            }
            printf("R");
            for (int l = 0; l < FLL_LAGS; ++l) printf(" %lld", R[l]);
            printf("\n");
            double work[FLL_WORK];
            int coef[FLL_MAX_ORDER * FLL_MAX_ORDER], shift[FLL_MAX_ORDER];
            const int orders = max_order < bs - 1 ? max_order : bs - 1;
            fll_analyse(R, orders, fll_precision(bps), work, coef, shift);
            for (int m = 1; m <= orders; ++m) {
                printf("%d", m);
                if (shift[m - 1] < 0) {
                    printf(" -");
                } else {
                    printf(" %d", shift[m - 1]);
                    for (int j = 0; j < m; ++j) printf(" %d", coef[(m - 1) * FLL_MAX_ORDER + j]);
                }
                printf("\n");
            }
        } else if (kind == 1) {
            int32_t bs;
            if (!get(f, &bs, 1) || bs < 2 || bs > 65536) return 4;
            std::vector<int32_t> q(bs);
            int32_t ms[2];
            if (!get(f, q.data(), bs) || !get(f, ms, 2)) return 3;
            const int m = ms[0], shift = ms[1];
            if (m < 1 || m > FLL_MAX_ORDER || m >= bs || shift < 0 || shift > 15) return 4;
            int32_t c[FLL_MAX_ORDER];
            if (!get(f, c, m)) return 3;
            fll_i64 lo = 0, hi = 0;
            int ok = 1;
            for (int i = m; i < bs; ++i) {
                const fll_i64 r = fll_resid(q.data(), i, c, m, shift);
                if (i == m || r < lo) lo = r;
                if (i == m || r > hi) hi = r;
                ok &= fll_resid_ok(r) ? 1 : 0;
            }
            printf("resid %lld %lld %d\n", lo, hi, ok);
        } else {
            return 4;
        }
    }
    fclose(f);
    return 0;
}
