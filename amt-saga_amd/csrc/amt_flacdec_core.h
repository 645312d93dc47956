// FLAC decoder core: bounded bit reader, subframe and frame decoder, chain walk.  Plain C++ behind one macro, so the same
// functions compile into the kernels of amt_flacdec.hip and into a stand-alone CPU program (tests/flacdec_host_main.cpp,
// built with the address and undefined-behaviour sanitizers).  The rule decoded is amt_saga/flac.py's reader, which
// stands where the reference calls librosa.load (audio_from_file, util_audio.py:962-964).
//
// Safety: the only loads from the stream are in fd_read and fd_unary, and both prove pos < end <= 8 * bytes first.
// Whatever the stream says, a read past the end yields zeros and sets FD_E_END; nothing else indexes by stream values
// without a range check (block size, predictor order, partition sizes, sample ranges).
#ifndef AMT_FLACDEC_CORE_H
#define AMT_FLACDEC_CORE_H
#include <stdint.h>
#include "amt_scratch.h"

#ifdef __HIP__
#define AMT_FD_HD __host__ __device__ inline
#else
#define AMT_FD_HD inline
#endif

// frame errors
#define FD_OK 0
#define FD_E_END 1           /* the stream ends inside the frame */
#define FD_E_FORMAT 2        /* reserved code, negative LPC shift, partition order that does not fit the block, ... */
#define FD_E_RANGE 3         /* a restored sample does not fit its subframe's bits */
#define FD_E_UNSUPPORTED 4   /* frame bps above 24 */
#define FD_E_TABLE 5         /* the candidate or stream table itself is out of range */
// stream status codes of the walk
#define FD_S_OK 0
#define FD_S_LOST_SYNC 1     /* no candidate starts where the chain arrived */
#define FD_S_FRAME 2         /* the candidate there does not decode */
#define FD_S_TABLE 5

#define FD_MAX_BLOCK 65536
#define FD_MAX_CHANNELS 8
#define FD_HIST 32
#define FD_MAX_FRAME_BYTES (1ull << 24)   /* STREAMINFO's maximum-frame-size field has 24 bits: no longer frame can be declared */

struct fd_bits {
    const unsigned char *data;
    uint64_t pos, end;        // bits; pos <= end <= 8 * bytes always
    int err;
};

// n = 0 .. 32 bits, MSB first
AMT_FD_HD uint32_t fd_read(fd_bits &b, int n) {
    if (n <= 0) return 0;
    if (b.end - b.pos < (uint64_t)n) {
        b.err = FD_E_END;
        b.pos = b.end;
        return 0;
    }
    const uint64_t p = b.pos, b0 = p >> 3, b1 = (p + (uint64_t)n - 1) >> 3;      // b1 < bytes: p + n <= end
    uint64_t v = 0;
    for (uint64_t i = b0; i <= b1; ++i) v = (v << 8) | b.data[i];                // at most 5 bytes
    v >>= (b1 + 1) * 8 - (p + (uint64_t)n);
    b.pos = p + (uint64_t)n;
    return (uint32_t)(n == 32 ? v : (v & ((1ull << n) - 1)));
}

AMT_FD_HD int32_t fd_read_signed(fd_bits &b, int n) {
    if (n <= 0) return 0;
    const uint32_t v = fd_read(b, n);
    const uint32_t sign = 1u << (n - 1);
    return (int32_t)((v ^ sign) - sign);                                          // two's complement of n bits
}

// zeros before the next one bit.  The run is capped by the end of the buffer (then FD_E_END) and by `limit`: a run
// longer than the caller can use is given up at once, with a value above `limit` and no error flag, so a lane does
// not read on through zeros whose outcome is already decided.  Whole zero words are taken eight bytes at a time.
AMT_FD_HD uint64_t fd_unary(fd_bits &b, uint64_t limit) {
    uint64_t q = 0;
    while (b.pos < b.end) {
        if (q > limit) return q;
        const unsigned off = (unsigned)(b.pos & 7);
        const uint64_t left = b.end - b.pos;
        if (off == 0 && q >= 16 && left >= 64) {                                  // only once a run is long: codes are short
            uint64_t w;
            __builtin_memcpy(&w, b.data + (b.pos >> 3), 8);                       // inside the buffer: 64 bits are left
            if (w == 0) {
                q += 64;
                b.pos += 64;
                continue;
            }
        }
        const unsigned avail = left < 8 - off ? (unsigned)left : 8 - off;
        const unsigned rem = ((unsigned)b.data[b.pos >> 3] << off) & 0xffu;
        if (rem) {
            const unsigned z = (unsigned)__builtin_clz(rem) - 24u;
            if (z < avail) {
                b.pos += z + 1;
                return q + z;
            }
        }
        q += avail;
        b.pos += avail;
    }
    b.err = FD_E_END;
    return q;
}

AMT_FD_HD int32_t fd_shl(int32_t v, int s) { return (int32_t)((uint32_t)v << s); }

// One subframe of `bs` samples at `bps` bits into out[0 .. bs).  hist and coef: FD_HIST entries each, `hs` apart (the
// kernels lay them out [tap][lane] in LDS); the predictor reads its history there, never from `out`.
AMT_FD_HD int fd_subframe(fd_bits &br, int bs, int bps, int32_t *out, int32_t *hist, int32_t *coef, int hs) {
    if (fd_read(br, 1)) return br.err ? br.err : FD_E_FORMAT;                      // padding bit
    const int typ = (int)fd_read(br, 6);
    int wasted = 0;
    if (fd_read(br, 1)) {
        const uint64_t w = fd_unary(br, (uint64_t)bps) + 1;
        if (br.err) return br.err;
        if (w >= (uint64_t)bps) return FD_E_FORMAT;
        wasted = (int)w;
        bps -= wasted;
    }
    if (br.err) return br.err;
    if (typ == 0) {
        const int32_t v = fd_shl(fd_read_signed(br, bps), wasted);
        if (br.err) return br.err;
        for (int i = 0; i < bs; ++i) out[i] = v;
        return FD_OK;
    }
    if (typ == 1) {
        for (int i = 0; i < bs; ++i) {
            out[i] = fd_shl(fd_read_signed(br, bps), wasted);
            if (br.err) return br.err;
        }
        return FD_OK;
    }
    int order, shift = 0;
    const bool lpc = typ >= 32;
    if (lpc) order = (typ & 31) + 1;
    else if (typ >= 8 && typ <= 12) order = typ - 8;
    else return FD_E_FORMAT;
    if (order > bs) return FD_E_FORMAT;
    for (int i = 0; i < order; ++i) {
        const int32_t v = fd_read_signed(br, bps);
        hist[(i & (FD_HIST - 1)) * hs] = v;
        out[i] = fd_shl(v, wasted);
    }
    if (lpc) {
        const int prec = (int)fd_read(br, 4) + 1;
        if (prec == 16) return br.err ? br.err : FD_E_FORMAT;
        shift = fd_read_signed(br, 5);
        if (shift < 0) return br.err ? br.err : FD_E_FORMAT;
        for (int j = 0; j < order; ++j) coef[j * hs] = fd_read_signed(br, prec);
    } else {
        const int c4[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
        for (int j = 0; j < order; ++j) coef[j * hs] = c4[order][j];
    }
    const int method = (int)fd_read(br, 2);
    if (br.err) return br.err;
    if (method > 1) return FD_E_FORMAT;
    const int pbits = method ? 5 : 4, esc = (1 << pbits) - 1;
    const int porder = (int)fd_read(br, 4);
    const int nparts = 1 << porder;
    if (bs & (nparts - 1)) return br.err ? br.err : FD_E_FORMAT;                  // 2^p must divide the block size
    const int psize = bs >> porder;
    if (psize < order) return br.err ? br.err : FD_E_FORMAT;                       // the first count would go negative
    const int64_t lo = -((int64_t)1 << (bps - 1)), hi = ((int64_t)1 << (bps - 1)) - 1;
    int i = order;
    for (int p = 0; p < nparts; ++p) {
        const int n = psize - (p == 0 ? order : 0);                               // may be 0
        const int k = (int)fd_read(br, pbits);
        const int raw = k == esc ? (int)fd_read(br, 5) : -1;
        if (br.err) return br.err;
        for (int t = 0; t < n; ++t, ++i) {
            int64_t s = 0;
            for (int j = 0; j < order; ++j)
                s += (int64_t)coef[j * hs] * (int64_t)hist[((i - 1 - j) & (FD_HIST - 1)) * hs];
            const int64_t pred = s >> shift;                                      // |pred| < 2^46
            int64_t r;
            if (raw >= 0) {
                r = fd_read_signed(br, raw);
            } else {
                // the residuals that leave the sample in range are lo - pred .. hi - pred: a longer run is refused
                // where it passes that, not where it ends
                const int64_t m = (pred < 0 ? -pred : pred) + hi + 1;
                uint64_t qmax = (2 * (uint64_t)m + 1) >> k;
                if (qmax >> (33 - k)) qmax = ((uint64_t)1 << (33 - k)) - 1;       // and the residual stays inside 33 bits
                const uint64_t q = fd_unary(br, qmax);
                if (br.err) return br.err;
                if (q > qmax) return FD_E_RANGE;
                const uint64_t low = fd_read(br, k);
                const uint64_t v = (q << k) | low;
                r = (int64_t)(v >> 1) ^ -(int64_t)(v & 1);
            }
            if (br.err) return br.err;
            const int64_t v = r + pred;
            if (v < lo || v > hi) return FD_E_RANGE;
            hist[(i & (FD_HIST - 1)) * hs] = (int32_t)v;
            out[i] = fd_shl((int32_t)v, wasted);
        }
    }
    return FD_OK;
}

AMT_FD_HD int fd_side_bit(int ca, int c) { return (ca == 8 && c == 1) || (ca == 9 && c == 0) || (ca == 10 && c == 1); }

// One frame whose header (hdr_len bytes at pos, CRC-8 included) the host has parsed: every subframe into slot
// [channels][bs], then the byte after the CRC-16 in *end_byte.  `bytes` bounds every read, and so does
// FD_MAX_FRAME_BYTES from the frame's start: a lane's work is bounded by that, not by the size of the file.
AMT_FD_HD int fd_frame(const unsigned char *data, uint64_t bytes, uint64_t pos, int hdr_len, int bs, int ca, int fbps,
                       int channels, int32_t *slot, int32_t *hist, int32_t *coef, int hs, uint64_t *end_byte) {
    *end_byte = pos;
    if (bs < 1 || bs > FD_MAX_BLOCK || ca < 0 || ca > 10 || hdr_len < 5 || hdr_len > 16 || fbps < 4) return FD_E_TABLE;
    if (fbps > 24) return FD_E_UNSUPPORTED;
    if (channels < 1 || channels > FD_MAX_CHANNELS) return FD_E_TABLE;
    const int nch = ca < 8 ? ca + 1 : 2;
    if (nch != channels) return FD_E_FORMAT;
    if (pos > bytes || bytes - pos < (uint64_t)hdr_len) return FD_E_END;
    if (bytes - pos > FD_MAX_FRAME_BYTES) bytes = pos + FD_MAX_FRAME_BYTES;
    fd_bits br = {data, (pos + (uint64_t)hdr_len) * 8, bytes * 8, 0};
    for (int c = 0; c < nch; ++c) {
        const int e = fd_subframe(br, bs, fbps + fd_side_bit(ca, c), slot + (int64_t)c * bs, hist, coef, hs);
        if (e) return e;
    }
    const uint64_t body_end = (br.pos + 7) >> 3;
    if (bytes - body_end < 2 || body_end > bytes) return FD_E_END;
    *end_byte = body_end + 2;
    return FD_OK;
}

// channel c of sample i from the two decorrelated subframe values (a = first subframe, b = second)
AMT_FD_HD int32_t fd_stereo(int ca, int c, int32_t a, int32_t b) {
    if (ca == 8) return c == 0 ? a : a - b;
    if (ca == 9) return c == 0 ? a + b : b;
    const int32_t mid = fd_shl(a, 1) | (b & 1);
    return c == 0 ? (mid + b) >> 1 : (mid - b) >> 1;
}

typedef long long fd_i64;

// first index in [lo, hi) of the sorted positions cand[i * stride] that equals key, or -1
AMT_FD_HD fd_i64 fd_find(const fd_i64 *cand, fd_i64 stride, fd_i64 lo, fd_i64 hi, fd_i64 key) {
    fd_i64 a = lo, b = hi;
    while (a < b) {
        const fd_i64 m = a + (b - a) / 2;
        if (cand[m * stride] < key) a = m + 1; else b = m;
    }
    return (a < hi && cand[a * stride] == key) ? a : -1;
}

// The sequential reader's walk: from the candidate at first_byte, got += bs until got >= total; frame numbers ignored.
// next[c]: the candidate that starts at c's end byte or -1; cand_out [.][3] = end, error, on-chain (set here);
// first[c] = the first sample of an on-chain frame.  Returns the status code, *at the byte it speaks of.
AMT_FD_HD int fd_walk(const fd_i64 *cand_pos, fd_i64 stride, const fd_i64 *cand_bs, fd_i64 lo, fd_i64 hi,
                      fd_i64 first_byte, fd_i64 total, const fd_i64 *next, fd_i64 *cand_out, fd_i64 *first,
                      fd_i64 *at) {
    fd_i64 got = 0, byte = first_byte;
    fd_i64 c = total > 0 ? fd_find(cand_pos, stride, lo, hi, first_byte) : -1;
    while (got < total) {
        *at = byte;
        if (c < lo || c >= hi) return FD_S_LOST_SYNC;
        if (cand_out[3 * c + 1] != FD_OK) return cand_out[3 * c + 1] == FD_E_TABLE ? FD_S_TABLE : FD_S_FRAME;
        cand_out[3 * c + 2] = 1;
        first[c] = got;
        got += cand_bs[c * stride];
        byte = cand_out[3 * c];
        c = next[c];
    }
    *at = byte;
    return FD_S_OK;
}

// CRC-16 (0x8005, zero initial value), byte by byte: the stand-alone program's; the place kernel does it in parallel
AMT_FD_HD unsigned fd_crc16(const unsigned char *p, uint64_t n) {
    unsigned crc = 0;
    for (uint64_t i = 0; i < n; ++i) {
        crc ^= (unsigned)p[i] << 8;
        for (int j = 0; j < 8; ++j) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x8005u) & 0xffffu : (crc << 1) & 0xffffu;
    }
    return crc;
}

// The scratch of amt_flac_decode_ragged: the candidates' slots, then, on an 8-byte boundary, two int64 per candidate.
struct fd_layout {
    int *slots;                  // [slot_ints]
    fd_i64 *next, *first;        // [n_cand]
};
inline fd_i64 fd_make_layout(void *scratch, fd_i64 n_cand, fd_i64 slot_ints, fd_layout *L) {
    if (n_cand > (1LL << 40) || slot_ints > (1LL << 56)) return -1;
    amt_carver c(scratch);
    L->slots = c.take<int>(slot_ints);
    L->next = c.take<fd_i64>(n_cand, 8);
    L->first = c.take<fd_i64>(n_cand, 8);
    return c.failed ? -1 : c.at;
}

#endif
