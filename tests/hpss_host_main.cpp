// amt_hpss_core.h on the host, alone: built by tests/test_hpss_cpu.py with the address and undefined-behaviour
// sanitizers and run directly.  Reads packed cases, splits each the way the kernel does -- per cell the two windows
// through the reflection map into the size class's array, the sorting network, the masks -- from arrays of exactly the
// stated sizes, and writes per case Ht and Pf, then Sh and Sp of every parameter set, to stdout, [T][ldf] float32 each, pad
// columns zero.
//
// File: "HPSS", int32 n; per case: int32 T, F, ldf, kt, kf, sets; float32 (power, margin_h, margin_p) x sets; float32
// S[T][ldf].
#include <stdio.h>
#include <string.h>
#include <vector>
#include "amt_hpss_core.h"

static bool read_exact(FILE *f, void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

static bool bisect = false;                      // argv[2] == "bisect": the core's other median, the same values

template <class Fetch> static uint32_t median_of(int k, Fetch fetch) {
    if (bisect) return hpss_median_bisect(k, fetch);
    switch (hpss_class(k)) {
    case 8: return hpss_median<8>(k, fetch);
    case 32: return hpss_median<32>(k, fetch);
    default: return hpss_median<64>(k, fetch);
    }
}

int main(int argc, char **argv) {
    if (argc != 2 && argc != 3) { fprintf(stderr, "usage: hpss_host_main cases.bin [bisect] > planes\n"); return 2; }
    bisect = argc == 3 && strcmp(argv[2], "bisect") == 0;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char magic[4];
    int32_t n = 0;
    if (!read_exact(f, magic, 4) || memcmp(magic, "HPSS", 4) != 0 || !read_exact(f, &n, 4) || n < 0) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    for (int c = 0; c < n; ++c) {
        int32_t dims[6];
        if (!read_exact(f, dims, sizeof dims)) { fprintf(stderr, "case %d: short file\n", c); return 2; }
        const int T = dims[0], F = dims[1], ldf = dims[2], kt = dims[3], kf = dims[4], sets = dims[5];
        if (sets < 1 || sets > 64) { fprintf(stderr, "case %d: bad number of parameter sets\n", c); return 2; }
        std::vector<float> par(3u * sets);
        if (!read_exact(f, par.data(), 12u * sets)) { fprintf(stderr, "case %d: short file\n", c); return 2; }
        bool ok = T >= 1 && F >= 1 && F <= ldf && !(ldf & 3);
        for (int s = 0; s < sets; ++s) ok = ok && hpss_params_ok(kt, kf, par[3 * s], par[3 * s + 1], par[3 * s + 2]);
        if (!ok) {
            fprintf(stderr, "case %d: parameters outside the limits\n", c);
            return 3;
        }
        // the live bins alone, in an array of exactly T * F values: a read of a pad column or past an end is a report
        std::vector<float> row((size_t)ldf), S((size_t)T * F);
        for (int t = 0; t < T; ++t) {
            if (!read_exact(f, row.data(), 4u * ldf)) { fprintf(stderr, "case %d: short file\n", c); return 2; }
            memcpy(S.data() + (size_t)t * F, row.data(), 4u * F);
        }
        // the medians once, then the masks of every parameter set
        std::vector<float> med[2], out[2];
        for (auto &plane : med) plane.assign((size_t)T * ldf, 0.0f);
        const int ht = (kt - 1) / 2, hf = (kf - 1) / 2;
        for (int t = 0; t < T; ++t)
            for (int b = 0; b < F; ++b) {
                med[0][(size_t)t * ldf + b] = hpss_float(median_of(kt, [&](int j) {
                    return hpss_bits(S[(size_t)hpss_reflect((long long)t - ht + j, T) * F + b]); }));
                med[1][(size_t)t * ldf + b] = hpss_float(median_of(kf, [&](int j) {
                    return hpss_bits(S[(size_t)t * F + hpss_reflect((long long)b - hf + j, F)]); }));
            }
        for (auto &plane : med)
            if (fwrite(plane.data(), 4, plane.size(), stdout) != plane.size()) { fprintf(stderr, "case %d: short write\n", c); return 2; }
        for (int s = 0; s < sets; ++s) {
            for (auto &plane : out) plane.assign((size_t)T * ldf, 0.0f);
            for (int t = 0; t < T; ++t)
                for (int b = 0; b < F; ++b) {
                    const size_t at = (size_t)t * ldf + b;
                    float mask_h, mask_p;
                    hpss_masks(med[0][at], med[1][at], par[3 * s], par[3 * s + 1], par[3 * s + 2], &mask_h, &mask_p);
                    out[0][at] = S[(size_t)t * F + b] * mask_h;
                    out[1][at] = S[(size_t)t * F + b] * mask_p;
                }
            for (auto &plane : out)
                if (fwrite(plane.data(), 4, plane.size(), stdout) != plane.size()) { fprintf(stderr, "case %d: short write\n", c); return 2; }
        }
    }
    fclose(f);
    return 0;
}
