// Stand-alone CPU program over csrc/amt_pcm_core.h: the WAV sample rule and the table clamps exactly as the kernels of
// amt_pcm.hip compile them, run thread by thread on the host.  Built by tests/test_wav_cpu.py with the address and
// undefined-behaviour sanitizers; a report aborts the program (a nonzero exit).
//
// Input file (little-endian), written by the test:
//   "PCMC" | int32 cases
//   unpack case: int32 0 | int64 data_bytes | data | int32 rows | int64 [rows][8] | int64 out_values | int32 with_pcm |
//                uint32 expect_out[out_values] | int32 expect_pcm[out_values]      (untouched values: the sentinels)
//   pack case:   int32 1 | int64 len | uint32 wave bits[len] | int32 fmt | int32 has_peak | uint32 peak bits |
//                int64 out_base | int64 out_bytes | uint8 expect[out_bytes]         (untouched bytes: 0xAB)
// Every case is run with the byte buffer at each of the four alignments modulo 4, each time ending exactly where its
// allocation ends, so a read or write one byte past it is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "amt_pcm_core.h"

#define SENT_OUT 0xDEADBEEFu
#define SENT_PCM 0x5EADBEEF
#define SENT_BYTE 0xAB
#define THREADS 256
#define TILE (THREADS * PCM_RUN)
#define GRID_X 3                      /* narrower than the files: the walk by the grid's width is exercised */

template <class T>
static bool rd(FILE *f, T *v, size_t n = 1) { return fread(v, sizeof(T), n, f) == n; }

template <int C>
static void unpack_thread(const unsigned char *data, pcm_i64 data_bytes, pcm_i64 off, pcm_i64 values, pcm_i64 v0, int kind,
                          int bits, uint32_t *out, int32_t *pcm) {
    const int nv = (int)(values - v0 < PCM_RUN ? values - v0 : PCM_RUN);
    uint32_t y[PCM_RUN];
    int32_t q[PCM_RUN];
    pcm_unpack_values<C>(data, data_bytes, off + v0 * C, nv, kind, bits, y, q);
    for (int j = 0; j < nv; ++j) {
        out[v0 + j] = y[j];
        if (pcm && kind == PCM_KIND_INT) pcm[v0 + j] = q[j];
    }
}

static int run_unpack(FILE *f, int index) {
    pcm_i64 data_bytes, out_values;
    int rows, with_pcm;
    if (!rd(f, &data_bytes)) return 1;
    std::vector<unsigned char> bytes((size_t)data_bytes);
    if (data_bytes && !rd(f, bytes.data(), (size_t)data_bytes)) return 1;
    if (!rd(f, &rows)) return 1;
    std::vector<pcm_i64> meta((size_t)rows * PCM_META);
    if (!rd(f, meta.data(), meta.size()) || !rd(f, &out_values) || !rd(f, &with_pcm)) return 1;
    std::vector<uint32_t> want((size_t)out_values);
    std::vector<int32_t> want_pcm((size_t)out_values);
    if (out_values && (!rd(f, want.data(), want.size()) || !rd(f, want_pcm.data(), want_pcm.size()))) return 1;
    for (int k = 0; k < 4; ++k) {
        unsigned char *buf = (unsigned char *)malloc((size_t)data_bytes + k);       // data ends where the block ends
        unsigned char *data = buf + k;
        if (data_bytes) memcpy(data, bytes.data(), (size_t)data_bytes);
        uint32_t *out = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)out_values);
        int32_t *pcm = with_pcm ? (int32_t *)malloc(sizeof(int32_t) * (size_t)out_values) : nullptr;
        for (pcm_i64 i = 0; i < out_values; ++i) {
            out[i] = SENT_OUT;
            if (pcm) pcm[i] = SENT_PCM;
        }
        for (int b = 0; b < rows; ++b) {
            const pcm_i64 *row = meta.data() + (size_t)b * PCM_META;
            const pcm_i64 values = pcm_row_values(row, data_bytes, out_values);
            const int kind = (int)row[3], c = (int)row[4], bits = (int)row[5];
            for (int bx = 0; bx < GRID_X; ++bx)
                for (pcm_i64 t0 = (pcm_i64)bx * TILE; t0 < values; t0 += (pcm_i64)GRID_X * TILE)
                    for (int t = 0; t < THREADS; ++t) {
                        const pcm_i64 v0 = t0 + (pcm_i64)t * PCM_RUN;
                        if (v0 >= values) continue;
                        uint32_t *o = out + row[6];
                        int32_t *p = pcm ? pcm + row[6] : nullptr;
                        switch (c) {
                        case 1: unpack_thread<1>(data, data_bytes, row[0], values, v0, kind, bits, o, p); break;
                        case 2: unpack_thread<2>(data, data_bytes, row[0], values, v0, kind, bits, o, p); break;
                        case 3: unpack_thread<3>(data, data_bytes, row[0], values, v0, kind, bits, o, p); break;
                        case 4: unpack_thread<4>(data, data_bytes, row[0], values, v0, kind, bits, o, p); break;
                        case 8: unpack_thread<8>(data, data_bytes, row[0], values, v0, kind, bits, o, p); break;
                        default: break;
                        }
                    }
        }
        pcm_i64 bad = 0;
        for (pcm_i64 i = 0; i < out_values; ++i) {
            if (out[i] != want[(size_t)i] || (pcm && pcm[i] != want_pcm[(size_t)i])) {
                if (!bad++)
                    printf("case %d align %d: value %lld is %08x / %d, expected %08x / %d\n", index, k, (long long)i,
                           out[i], pcm ? pcm[i] : 0, want[(size_t)i], want_pcm[(size_t)i]);
            }
        }
        free(buf);
        free(out);
        free(pcm);
        if (bad) {
            printf("case %d align %d -> %lld values differ\n", index, k, (long long)bad);
            return 2;
        }
    }
    printf("case %d unpack rows %d values %lld -> ok\n", index, rows, (long long)out_values);
    return 0;
}

template <int C>
static void pack_thread(const float *x, pcm_i64 n_s, pcm_i64 s0, int fmt, float divisor, unsigned char *dst) {
    const int nv = (int)(n_s - s0 < PCM_RUN ? n_s - s0 : PCM_RUN);
    uint32_t w[C];
    pcm_pack_words<C>(x + s0, nv, fmt, divisor, w);
    for (int i = 0; i < nv * C; ++i) dst[s0 * C + i] = (unsigned char)(w[i >> 2] >> (8 * (i & 3)));
}

static int run_pack(FILE *f, int index) {
    pcm_i64 len, out_base, out_bytes;
    int fmt, has_peak;
    uint32_t peak_bits;
    if (!rd(f, &len)) return 1;
    std::vector<uint32_t> wave_bits((size_t)len);
    if (len && !rd(f, wave_bits.data(), wave_bits.size())) return 1;
    if (!rd(f, &fmt) || !rd(f, &has_peak) || !rd(f, &peak_bits) || !rd(f, &out_base) || !rd(f, &out_bytes)) return 1;
    std::vector<unsigned char> want((size_t)out_bytes);
    if (out_bytes && !rd(f, want.data(), want.size())) return 1;
    float *x = (float *)malloc(sizeof(float) * (size_t)len);                        // exact size: reads past it are reported
    if (len) memcpy(x, wave_bits.data(), sizeof(float) * (size_t)len);
    unsigned char *out = (unsigned char *)malloc((size_t)out_bytes);
    memset(out, SENT_BYTE, (size_t)out_bytes);
    if (pcm_pack_bytes(len, out_base, fmt, out_bytes) != 0) {
        const float divisor = has_peak ? pcm_norm_divisor(pcm_bits_float(peak_bits)) : 0.f;
        for (int bx = 0; bx < GRID_X; ++bx)
            for (pcm_i64 t0 = (pcm_i64)bx * TILE; t0 < len; t0 += (pcm_i64)GRID_X * TILE)
                for (int t = 0; t < THREADS; ++t) {
                    const pcm_i64 s0 = t0 + (pcm_i64)t * PCM_RUN;
                    if (s0 >= len) continue;
                    if (fmt == PCM_FMT_PCM16) pack_thread<2>(x, len, s0, fmt, divisor, out + out_base);
                    else if (fmt == PCM_FMT_PCM24) pack_thread<3>(x, len, s0, fmt, divisor, out + out_base);
                    else pack_thread<4>(x, len, s0, fmt, divisor, out + out_base);
                }
    }
    pcm_i64 bad = 0;
    for (pcm_i64 i = 0; i < out_bytes; ++i)
        if (out[i] != want[(size_t)i] && !bad++)
            printf("case %d: byte %lld is %02x, expected %02x\n", index, (long long)i, out[i], want[(size_t)i]);
    free(x);
    free(out);
    if (bad) {
        printf("case %d -> %lld bytes differ\n", index, (long long)bad);
        return 2;
    }
    printf("case %d pack fmt %d len %lld -> ok\n", index, fmt, (long long)len);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) return 64;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 65;
    char magic[4];
    int cases = 0;
    if (!rd(f, magic, 4) || memcmp(magic, "PCMC", 4) != 0 || !rd(f, &cases)) return 66;
    for (int i = 0; i < cases; ++i) {
        int type;
        if (!rd(f, &type)) return 67;
        const int e = type == 0 ? run_unpack(f, i) : run_pack(f, i);
        if (e) {
            printf("case %d -> failed (%d)\n", i, e);
            return 1;
        }
    }
    fclose(f);
    return 0;
}
