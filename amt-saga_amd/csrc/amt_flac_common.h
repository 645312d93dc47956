// CRC and MD5 pieces shared by the FLAC encoder (amt_flac.hip) and decoder (amt_flacdec.hip).
#ifndef AMT_FLAC_COMMON_H
#define AMT_FLAC_COMMON_H
#include <math.h>

__device__ __forceinline__ unsigned fl_crc8_step(unsigned crc, unsigned byte) {
    crc ^= byte;
    for (int i = 0; i < 8; ++i) crc = (crc & 0x80u) ? ((crc << 1) ^ 0x07u) & 0xffu : (crc << 1) & 0xffu;
    return crc;
}

// a(x) b(x) modulo x^16 + x^15 + x^2 + 1
__device__ __forceinline__ unsigned fl_mulmod16(unsigned a, unsigned b) {
    unsigned r = 0;
    for (int i = 15; i >= 0; --i) {
        r = (r & 0x8000u) ? ((r << 1) ^ 0x8005u) & 0xffffu : (r << 1);
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

// entry i of the byte table of CRC-16 (0x8005, MSB first, zero initial value)
__device__ __forceinline__ unsigned short fl_crc16_entry(unsigned i) {
    unsigned c = i << 8;
    for (int j = 0; j < 8; ++j) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xffffu : (c << 1);
    return (unsigned short)c;
}

struct fl_md5_consts { unsigned k[64]; };

__device__ __forceinline__ unsigned fl_rotl(unsigned v, int s) { return (v << s) | (v >> (32 - s)); }

// one MD5 block of 16 words at m (LDS; every lane reads the same address)
__device__ __forceinline__ void fl_md5_block(unsigned *st, const unsigned *m, const fl_md5_consts &kc) {
    unsigned a = st[0], b = st[1], c = st[2], d = st[3];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        unsigned fv;
        int g, s;
        if (i < 16) {
            fv = (b & c) | (~b & d); g = i;
            s = (i & 3) == 0 ? 7 : (i & 3) == 1 ? 12 : (i & 3) == 2 ? 17 : 22;
        } else if (i < 32) {
            fv = (d & b) | (~d & c); g = (5 * i + 1) & 15;
            s = (i & 3) == 0 ? 5 : (i & 3) == 1 ? 9 : (i & 3) == 2 ? 14 : 20;
        } else if (i < 48) {
            fv = b ^ c ^ d; g = (3 * i + 5) & 15;
            s = (i & 3) == 0 ? 4 : (i & 3) == 1 ? 11 : (i & 3) == 2 ? 16 : 23;
        } else {
            fv = c ^ (b | ~d); g = (7 * i) & 15;
            s = (i & 3) == 0 ? 6 : (i & 3) == 1 ? 10 : (i & 3) == 2 ? 15 : 21;
        }
        fv = fv + a + kc.k[i] + m[g];
        a = d; d = c; c = b;
        b = b + fl_rotl(fv, s);
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d;
}

static inline void fl_md5_fill(fl_md5_consts &kc) {
    for (int i = 0; i < 64; ++i) kc.k[i] = (unsigned)(long long)floor(fabs(sin((double)(i + 1))) * 4294967296.0);
}

#endif
