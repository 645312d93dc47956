// WAV sample rule and table clamps: plain C++ behind one macro, so the same functions compile into the kernels of
// amt_pcm.hip and into a stand-alone CPU program (tests/pcm_host_main.cpp, built with the address and
// undefined-behaviour sanitizers).  The rule is amt_saga/wav.py's, which stands where the reference calls librosa.load
// (audio_from_file, util_audio.py:962-964) and librosa.output.write_wav (audio_complete.save, util_audio.py:526-527).
//
//   integer, container c bytes (little-endian, signed; c = 1: unsigned, u - 128), valid bits b:
//       q = container >> (8 c - b)  (arithmetic),  wave = float32(q) 2^-(b-1),  pcm = q
//   float32: the 32 bits as they are.   float64: rounded to float32, nearest even.
//   writing: q = clip(rint(y 2^(b-1)), -2^(b-1), 2^(b-1) - 1) on the float32 product, NaN -> 0 (the FLAC encoder's rule).
//
// Safety: pcm_row_values and pcm_pack_bytes decide from the table row and the buffer sizes alone how much of a row may
// be touched -- all of it or nothing -- with divisions, never a product that could overflow.  pcm_load_run is the only
// load from the byte buffer; it proves pos + bytes <= data_bytes for the bytes it returns, and its aligned 4-byte loads
// lie inside [data, data + data_bytes).
#ifndef AMT_PCM_CORE_H
#define AMT_PCM_CORE_H
#include <stdint.h>

#ifdef __HIP__
#define AMT_PCM_HD __host__ __device__ inline
#else
#define AMT_PCM_HD inline
#endif

#define PCM_KIND_INT 0
#define PCM_KIND_FLOAT 1
#define PCM_MAX_CHANNELS 8
#define PCM_META 8            /* int64 per table row */
#define PCM_RUN 4             /* values one thread takes: 4 c bytes, a whole number of 32-bit words */
#define PCM_FMT_PCM16 0
#define PCM_FMT_PCM24 1
#define PCM_FMT_FLOAT32 2

typedef long long pcm_i64;

// row: byte offset of the first sample, frames, channels, kind, container bytes, valid bits, out base, reserved.
// Returns frames * channels if the row's geometry is one the rule knows and both of its regions lie inside their
// buffers, else 0: a row that points outside costs its output, never an access.
AMT_PCM_HD pcm_i64 pcm_row_values(const pcm_i64 *row, pcm_i64 data_bytes, pcm_i64 out_values) {
    const pcm_i64 off = row[0], frames = row[1], ch = row[2], kind = row[3], c = row[4], bits = row[5], ob = row[6];
    if (data_bytes <= 0 || out_values <= 0 || frames <= 0 || ch < 1 || ch > PCM_MAX_CHANNELS) return 0;
    if (kind == PCM_KIND_INT) {
        if (c < 1 || c > 4 || bits < 1 || bits > 8 * c) return 0;
    } else if (kind == PCM_KIND_FLOAT) {
        if (c != 4 && c != 8) return 0;
    } else {
        return 0;
    }
    if (frames > out_values / ch) return 0;                       // values = frames ch <= out_values: no overflow below
    const pcm_i64 values = frames * ch;
    if (values > data_bytes / c) return 0;                        // values c <= data_bytes
    if (off < 0 || off > data_bytes - values * c) return 0;
    if (ob < 0 || ob > out_values - values) return 0;
    return values;
}

AMT_PCM_HD int pcm_fmt_bytes(int fmt) { return fmt == PCM_FMT_PCM16 ? 2 : fmt == PCM_FMT_PCM24 ? 3 : fmt == PCM_FMT_FLOAT32 ? 4 : 0; }

// bytes signal (len samples, to out_base) may write in a buffer of out_bytes, all or nothing
AMT_PCM_HD pcm_i64 pcm_pack_bytes(pcm_i64 len, pcm_i64 out_base, int fmt, pcm_i64 out_bytes) {
    const pcm_i64 c = pcm_fmt_bytes(fmt);
    if (c == 0 || len <= 0 || out_bytes <= 0 || len > out_bytes / c) return 0;
    if (out_base < 0 || out_base > out_bytes - len * c) return 0;
    return len * c;
}

// The 4 C bytes at data[pos ..) as C little-endian words; `valid` of them (0 .. 4 C) are wanted, the rest read as 0.
// Inside a file one aligned run of C + 1 words is loaded and shifted; at the edges of the buffer, byte by byte.
template <int C>
AMT_PCM_HD void pcm_load_run(const unsigned char *data, pcm_i64 data_bytes, pcm_i64 pos, int valid, uint32_t *w) {
    for (int i = 0; i < C; ++i) w[i] = 0;
    if (pos < 0 || valid <= 0 || pos > data_bytes - valid) return;
    const uintptr_t a = (uintptr_t)(data + pos), a0 = a & ~(uintptr_t)3;
    if (valid == 4 * C && a0 >= (uintptr_t)data && pos + 4 * C + 4 <= data_bytes) {
        // a0 + 4 (C + 1) <= a + 4 C + 4 <= data + data_bytes
        const uint32_t *p = (const uint32_t *)a0;
        const unsigned sh = (unsigned)(a - a0) * 8u;
        uint32_t lo = p[0];
#pragma unroll
        for (int i = 0; i < C; ++i) {
            const uint32_t hi = p[i + 1];
            w[i] = sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
            lo = hi;
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 4 * C; ++i)                                       // (constant indices: w stays in registers)
        if (i < valid) w[i >> 2] |= (uint32_t)data[pos + i] << (8 * (i & 3));
}

// container j (c bytes) of a run of words
AMT_PCM_HD uint64_t pcm_container(const uint32_t *w, int j, int c) {
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < c; ++k) {
        const int byte = j * c + k;
        v |= (uint64_t)((w[byte >> 2] >> (8 * (byte & 3))) & 0xffu) << (8 * k);
    }
    return v;
}

AMT_PCM_HD float pcm_bits_float(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
AMT_PCM_HD uint32_t pcm_float_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }

// integer container -> q (the caller has checked c in 1 .. 4 and bits in 1 .. 8 c)
AMT_PCM_HD int32_t pcm_int_q(uint64_t raw, int c, int bits) {
    int32_t x;
    if (c == 1) x = (int32_t)(raw & 0xffu) - 128;
    else x = (int32_t)((uint32_t)raw << (32 - 8 * c)) >> (32 - 8 * c);
    return x >> (8 * c - bits);
}

// q -> the float the reader returns: float32(q), nearest even, times 2^-(bits-1) (exact)
AMT_PCM_HD float pcm_q_wave(int32_t q, int bits) {
    return (float)q * pcm_bits_float((uint32_t)(127 - (bits - 1)) << 23);
}

// float container -> the bits of the float32 the reader returns
AMT_PCM_HD uint32_t pcm_float_wave_bits(uint64_t raw, int c) {
    if (c == 4) return (uint32_t)raw;
    double d;
    __builtin_memcpy(&d, &raw, 8);
    return pcm_float_bits((float)d);
}

// One thread's run of the reader: values [0, nv) of the PCM_RUN containers at data[pos ..) -> the bit patterns of the
// waveform in y and, for integer rows, q.  The caller has validated the row (pcm_row_values).
template <int C>
AMT_PCM_HD void pcm_unpack_values(const unsigned char *data, pcm_i64 data_bytes, pcm_i64 pos, int nv, int kind, int bits,
                                  uint32_t *y, int32_t *q) {
    uint32_t w[C];
    pcm_load_run<C>(data, data_bytes, pos, nv * C, w);
#pragma unroll
    for (int j = 0; j < PCM_RUN; ++j) {
        const uint64_t raw = pcm_container(w, j, C);
        if (kind == PCM_KIND_INT && C <= 4) {
            q[j] = pcm_int_q(raw, C, bits);
            y[j] = pcm_float_bits(pcm_q_wave(q[j], bits));
        } else {
            q[j] = 0;
            y[j] = pcm_float_wave_bits(raw, C);
        }
    }
}

// the writer's quantiser, bps = 16 or 24
AMT_PCM_HD int32_t pcm_quant(float y, int bps) {
    const int32_t lim = (int32_t)1 << (bps - 1);
    const float r = __builtin_rintf(y * (float)lim);
    if (!(r == r)) return 0;
    if (r >= (float)lim) return lim - 1;
    if (r < -(float)lim) return -lim;
    return (int32_t)r;
}

// the divisor of a normalised write: the signal's peak, or 0 (no division: the signal as it is) where the peak is 0 or
// not finite
AMT_PCM_HD float pcm_norm_divisor(float peak) {
    const uint32_t u = pcm_float_bits(peak) & 0x7fffffffu;
    return (u == 0 || u >= 0x7f800000u) ? 0.f : pcm_bits_float(u);
}

// sample y of a signal -> the c = pcm_fmt_bytes(fmt) little-endian bytes of its container, in the low bits
AMT_PCM_HD uint32_t pcm_pack_value(float y, int fmt, float divisor) {
    if (divisor != 0.f) y = y / divisor;
    if (fmt == PCM_FMT_FLOAT32) return pcm_float_bits(y);
    const int bps = fmt == PCM_FMT_PCM16 ? 16 : 24;
    return (uint32_t)pcm_quant(y, bps) & (bps == 16 ? 0xffffu : 0xffffffu);
}

// One thread's run of the writer: samples x[0 .. nv) (the rest count as 0) -> the 4 C bytes of their containers as C
// little-endian words
template <int C>
AMT_PCM_HD void pcm_pack_words(const float *x, int nv, int fmt, float divisor, uint32_t *w) {
#pragma unroll
    for (int i = 0; i < C; ++i) w[i] = 0;
#pragma unroll
    for (int j = 0; j < PCM_RUN; ++j) {
        const uint32_t v = pcm_pack_value(j < nv ? x[j] : 0.f, fmt, divisor);
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const int byte = j * C + k;
            w[byte >> 2] |= ((v >> (8 * k)) & 0xffu) << (8 * (byte & 3));
        }
    }
}

#endif
