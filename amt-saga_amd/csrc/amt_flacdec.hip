// FLAC decoder for gfx950: file bytes on the device -> float32 (and int32) waveforms, n streams in one call.
//
// Replaces the librosa.load of audio_from_file (util_audio.py:962-964 of the reference) at the front of the song queue.
// The host finds the plausible frame headers (amt_saga/flac.py:frame_candidates, O(frames) work); everything per bit
// and per sample happens here.  The decoding rule is amt_flacdec_core.h, shared with a sanitised CPU program.
//
//  * frame kernel: one lane per candidate.  Speculative: the lane decodes the whole frame into its slot of the scratch,
//    int32 [channels][bs], and records end byte and error.  A false candidate costs its slot and nothing else.
//    The 32-sample predictor history and the coefficients live in LDS, [tap][lane].
//  * walk kernel: one wave per stream.  Lanes binary-search, for every candidate, the candidate that starts at its end
//    byte; lane 0 then follows the chain from the first frame byte as the sequential reader does (got += bs until
//    total) and hands every on-chain frame its first sample.
//  * place kernel: one workgroup per candidate, off-chain ones leave at once.  CRC-16 of the frame's bytes in parallel
//    (256 chunks combined pairwise, as the encoder does), then stereo decorrelation, the cut at `total`, and stores
//    interleaved [samples][channels]: float32 pcm 2^-(bps-1) and optionally the int32 PCM.
//  * md5 kernel: one wave per stream over the interleaved little-endian bytes, in the structure of flac_md5_kernel.
//  * the stream is the only ordering; no workgroup waits for another; the only atomic is an integer min on a status word.
#include "amt_common.h"
#include "amt_flac_common.h"
#include "amt_flacdec_core.h"

#define AMT_FD_LANES 64
#define AMT_FD_THREADS 256
#define AMT_FD_SM 9            /* int64 per stream: byte offset, size, first frame byte, channels, bps, total, out base, cand lo, hi */
#define AMT_FD_CM 7            /* int64 per candidate: stream, position, header bytes, block size, assignment, bps, slot offset */
#define AMT_FD_NOPOS 0x7fffffffffffffffLL

struct fd_stream {
    long long off, size, first, channels, bps, total, out_base, lo, hi;
    bool ok;
};

__device__ __forceinline__ fd_stream fd_load_stream(const long long *sm, long long s, long long data_bytes,
                                                    long long n_cand, long long out_values) {
    const long long *m = sm + s * AMT_FD_SM;
    fd_stream t = {m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], false};
    t.ok = t.off >= 0 && t.size >= 0 && t.off <= data_bytes && t.size <= data_bytes - t.off && t.first >= 0 &&
           t.first <= t.size && t.channels >= 1 && t.channels <= FD_MAX_CHANNELS && t.bps >= 4 && t.bps <= 24 &&
           t.total >= 0 && t.total < (1LL << 36) && t.out_base >= 0 && t.out_base <= out_values &&
           t.total * t.channels <= out_values - t.out_base && t.lo >= 0 && t.lo <= t.hi && t.hi <= n_cand;
    return t;
}

__global__ __launch_bounds__(AMT_FD_LANES) void flacdec_frame_kernel(
    const unsigned char *__restrict__ data, long long data_bytes, const long long *__restrict__ sm, int n,
    const long long *__restrict__ cm, long long n_cand, int *__restrict__ slots, long long slot_ints,
    long long out_values, long long *__restrict__ cand_out) {
    __shared__ int hist[FD_HIST * AMT_FD_LANES];
    __shared__ int coef[FD_HIST * AMT_FD_LANES];
    const int lane = threadIdx.x;
    const long long c = (long long)blockIdx.x * AMT_FD_LANES + lane;
    if (c >= n_cand) return;
    const long long *m = cm + c * AMT_FD_CM;
    const long long s = m[0], pos = m[1], hdr = m[2], bs = m[3], ca = m[4], fbps = m[5], slot = m[6];
    int err = FD_E_TABLE;
    uint64_t end = 0;
    if (s >= 0 && s < n) {
        const fd_stream t = fd_load_stream(sm, s, data_bytes, n_cand, out_values);
        if (t.ok && pos >= 0 && pos < t.size && bs >= 1 && bs <= FD_MAX_BLOCK && hdr >= 0 && hdr <= 16 && ca >= 0 &&
            ca <= 10 && fbps >= 0 && fbps <= 64 && slot >= 0 && slot <= slot_ints &&
            t.channels * bs <= slot_ints - slot) {
            err = fd_frame(data + t.off, (uint64_t)t.size, (uint64_t)pos, (int)hdr, (int)bs, (int)ca, (int)fbps,
                           (int)t.channels, slots + slot, hist + lane, coef + lane, AMT_FD_LANES, &end);
        }
    }
    cand_out[3 * c] = (long long)end;
    cand_out[3 * c + 1] = err;
    cand_out[3 * c + 2] = 0;
}

// status [n][4]: code, byte it speaks of, first byte of the lowest frame whose CRC-16 fails (AMT_FD_NOPOS: none), MD5 differs
__global__ __launch_bounds__(AMT_FD_LANES) void flacdec_walk_kernel(
    const long long *__restrict__ sm, int n, const long long *__restrict__ cm, long long n_cand, long long data_bytes,
    long long out_values, long long *__restrict__ cand_out, long long *__restrict__ next, long long *__restrict__ first,
    long long *__restrict__ status) {
    const int lane = threadIdx.x;
    const long long s = blockIdx.x;
    const fd_stream t = fd_load_stream(sm, s, data_bytes, n_cand, out_values);
    if (!t.ok) {
        if (lane == 0) {
            status[4 * s] = FD_S_TABLE; status[4 * s + 1] = 0; status[4 * s + 2] = AMT_FD_NOPOS; status[4 * s + 3] = 0;
        }
        return;
    }
    for (long long c = t.lo + lane; c < t.hi; c += AMT_FD_LANES) {
        long long nx = -1;
        if (cm[c * AMT_FD_CM] != s) cand_out[3 * c + 1] = FD_E_TABLE;               // a candidate of another stream
        else if (cand_out[3 * c + 1] == FD_OK) nx = fd_find(cm + 1, AMT_FD_CM, t.lo, t.hi, cand_out[3 * c]);
        next[c] = nx;
    }
    __syncthreads();
    if (lane == 0) {
        long long at = t.first;
        const int code = fd_walk(cm + 1, AMT_FD_CM, cm + 3, t.lo, t.hi, t.first, t.total, next, cand_out, first, &at);
        status[4 * s] = code; status[4 * s + 1] = at; status[4 * s + 2] = AMT_FD_NOPOS; status[4 * s + 3] = 0;
    }
}

__global__ __launch_bounds__(AMT_FD_THREADS) void flacdec_place_kernel(
    const unsigned char *__restrict__ data, long long data_bytes, const long long *__restrict__ sm, int n,
    const long long *__restrict__ cm, long long n_cand, const int *__restrict__ slots, long long out_values,
    const long long *__restrict__ cand_out, const long long *__restrict__ first, int verify, float *__restrict__ out_f,
    int *__restrict__ out_i, long long *__restrict__ status) {
    __shared__ unsigned crc_s[AMT_FD_THREADS];
    __shared__ unsigned short crctab[256];
    const int tid = threadIdx.x;
    const long long c = blockIdx.x;
    if (cand_out[3 * c + 2] != 1 || cand_out[3 * c + 1] != FD_OK) return;          // off chain (block-uniform)
    const long long *m = cm + c * AMT_FD_CM;
    const long long s = m[0], pos = m[1], bs = m[3], ca = m[4], slot = m[6];
    if (s < 0 || s >= n) return;
    const fd_stream t = fd_load_stream(sm, s, data_bytes, n_cand, out_values);
    if (!t.ok) return;                                                             // (the frame kernel refused it already)
    const long long end = cand_out[3 * c];
    if (verify && end - 2 >= pos && end <= t.size) {
        const unsigned char *p = data + t.off + pos;
        const long long ncrc = end - 2 - pos;                                      // < FD_MAX_FRAME_BYTES (fd_frame)
        crctab[tid] = fl_crc16_entry((unsigned)tid);
        __syncthreads();
        const long long lc = (ncrc + AMT_FD_THREADS - 1) / AMT_FD_THREADS;
        const long long pad = AMT_FD_THREADS * lc - ncrc;                          // zero bytes in front change nothing
        unsigned crc = 0, mul = 1;
        for (long long j = 0; j < lc; ++j) {
            const long long idx = tid * lc + j - pad;
            if (idx >= 0) crc = ((crc << 8) & 0xffffu) ^ crctab[((crc >> 8) ^ p[idx]) & 0xffu];
            mul = ((mul << 8) & 0xffffu) ^ crctab[(mul >> 8) & 0xffu];             // x^(8 lc)
        }
        crc_s[tid] = crc;
        for (int st = 1; st < AMT_FD_THREADS; st <<= 1) {
            __syncthreads();
            if ((tid & (2 * st - 1)) == 2 * st - 1) crc_s[tid] = fl_mulmod16(crc_s[tid - st], mul) ^ crc_s[tid];
            mul = fl_mulmod16(mul, mul);
        }
        __syncthreads();
        if (tid == 0) {
            const unsigned want = ((unsigned)p[ncrc] << 8) | p[ncrc + 1];
            if (crc_s[AMT_FD_THREADS - 1] != want)
                atomicMin((unsigned long long *)&status[4 * s + 2], (unsigned long long)pos);
        }
    }
    const int ch = (int)t.channels;
    const long long f0 = first[c];
    long long keep = t.total - f0;                                                 // the cut at `total`
    if (keep > bs) keep = bs;
    if (f0 < 0 || keep <= 0) return;
    const int *sl = slots + slot;
    const float scale = 1.0f / (float)(1 << (t.bps - 1));                          // a power of two: the product is exact
    const long long base = t.out_base + f0 * ch;
    for (long long j = tid; j < keep * ch; j += AMT_FD_THREADS) {
        const long long i = j / ch;
        const int k = (int)(j - i * ch);
        const int v = ca < 8 ? sl[k * bs + i] : fd_stereo((int)ca, k, sl[i], sl[bs + i]);
        out_f[base + j] = (float)v * scale;
        if (out_i) out_i[base + j] = v;
    }
}

// MD5 of the interleaved little-endian PCM of every stream: one wave per stream.  Per 64 values the lanes put the
// integers back from the floats (exact: |pcm| < 2^24) into LDS, lane w < 16 nb builds message word w from their bytes
// (nb = bytes per sample), and every lane runs the same rounds on the same words.  The next 64 values are in flight
// during the rounds.  The last piece (fewer than 64 values, the 0x80 byte, zeros, the bit length) is one word per lane.
__global__ __launch_bounds__(AMT_FD_LANES) void flacdec_md5_kernel(
    const float *__restrict__ out_f, const long long *__restrict__ sm, long long data_bytes, long long n_cand,
    long long out_values, const unsigned char *__restrict__ expect, unsigned char *__restrict__ md5,
    long long *__restrict__ status, fl_md5_consts kc) {
    __shared__ int val[64];
    __shared__ unsigned m[64];
    const int lane = threadIdx.x;
    const long long s = blockIdx.x;
    const fd_stream t = fd_load_stream(sm, s, data_bytes, n_cand, out_values);
    if (!t.ok || status[4 * s] != FD_S_OK) {
        if (lane < 16) md5[16 * s + lane] = 0;
        return;
    }
    const float *x = out_f + t.out_base;
    const long long nv = t.total * t.channels;
    const int nb = (int)(t.bps + 7) >> 3;
    const float up = (float)(1 << (t.bps - 1));
    unsigned st[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    auto word = [&](int w) {                                                       // bytes 4 w .. 4 w + 3 of the piece
        unsigned r = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = 4 * w + j, vi = b / nb;
            const unsigned byte = vi < 64 ? ((unsigned)val[vi] >> (8 * (b - vi * nb))) & 0xffu : 0u;
            r |= byte << (8 * j);
        }
        return r;
    };
    long long s0 = 0;
    float y = nv >= 64 ? x[lane] : 0.f;
    for (; s0 + 64 <= nv; s0 += 64) {
        val[lane] = (int)(y * up);
        __syncthreads();
        if (s0 + 128 <= nv) y = x[s0 + 64 + lane];
        if (lane < 16 * nb) m[lane] = word(lane);
        __syncthreads();
        for (int k = 0; k < nb; ++k) fl_md5_block(st, m + 16 * k, kc);
        __syncthreads();
    }
    {
        const int r = (int)(nv - s0);                                              // 0 .. 63 values left
        const int nbytes = r * nb;
        const int tail = (nbytes + 9 + 63) / 64 * 64;                              // <= 256
        const int words = tail >> 2;
        const unsigned long long total_bits = (unsigned long long)nv * nb * 8;
        val[lane] = lane < r ? (int)(x[s0 + lane] * up) : 0;
        __syncthreads();
        unsigned wv = 4 * lane < nbytes ? word(lane) : 0u;
        if (4 * lane + 4 > nbytes && 4 * lane < nbytes) wv &= (1u << (8 * (nbytes - 4 * lane))) - 1u;
        if (4 * lane <= nbytes && nbytes < 4 * lane + 4) wv |= 0x80u << (8 * (nbytes - 4 * lane));
        if (lane == words - 2) wv = (unsigned)total_bits;
        if (lane == words - 1) wv = (unsigned)(total_bits >> 32);
        if (lane < words) m[lane] = wv;
        __syncthreads();
        for (int k = 0; k < (tail >> 6); ++k) fl_md5_block(st, m + 16 * k, kc);
    }
    if (lane < 16) {
        const unsigned char d = (unsigned char)(st[lane >> 2] >> (8 * (lane & 3)));
        md5[16 * s + lane] = d;
        bool any = false, diff = false;
        for (int j = 0; j < 16; ++j) any |= expect[16 * s + j] != 0;               // an all-zero digest: none recorded
        diff = d != expect[16 * s + lane];
        if (any && diff) status[4 * s + 3] = 1;                                    // (every writer stores the same 1)
    }
}

extern "C" {

long long amt_flac_decode_scratch_bytes(long long n_cand, long long slot_ints) {
    fd_layout L;
    const fd_i64 need = fd_make_layout(nullptr, n_cand, slot_ints, &L);
    return need < 0 ? AMT_E_INVALID : need;
}

int amt_flac_decode_ragged(const unsigned char *data, long long data_bytes, const long long *stream_meta, int n,
                           const long long *cand_meta, long long n_cand, const unsigned char *expect_md5, int verify,
                           unsigned char *scratch, long long scratch_bytes, long long slot_ints, float *out,
                           int *out_pcm, long long out_values, long long *status, long long *cand_out,
                           unsigned char *md5, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!data || !stream_meta || !cand_meta || !expect_md5 || !scratch || !out || !status || !cand_out || !md5)
        return AMT_E_INVALID;
    if (n < 1 || n_cand < 0 || data_bytes < 0 || slot_ints < 0 || out_values < 0 || verify < 0 || verify > 2)
        return AMT_E_INVALID;
    if (n > 65535 * 32 || n_cand > (1LL << 31) - 64) return AMT_E_UNSUPPORTED;
    fd_layout L;
    const fd_i64 need = fd_make_layout(scratch, n_cand, slot_ints, &L);
    if (need < 0) return AMT_E_INVALID;
    if (scratch_bytes < need) return AMT_E_SHAPE;
    if (n_cand > 0) {
        const unsigned blocks = (unsigned)((n_cand + AMT_FD_LANES - 1) / AMT_FD_LANES);
        flacdec_frame_kernel<<<blocks, AMT_FD_LANES, 0, stream>>>(data, data_bytes, stream_meta, n, cand_meta, n_cand,
                                                                  L.slots, slot_ints, out_values, cand_out);
        AMT_LAUNCH_CHECK();
    }
    flacdec_walk_kernel<<<n, AMT_FD_LANES, 0, stream>>>(stream_meta, n, cand_meta, n_cand, data_bytes, out_values,
                                                        cand_out, L.next, L.first, status);
    AMT_LAUNCH_CHECK();
    if (n_cand > 0) {
        flacdec_place_kernel<<<(unsigned)n_cand, AMT_FD_THREADS, 0, stream>>>(
            data, data_bytes, stream_meta, n, cand_meta, n_cand, L.slots, out_values, cand_out, L.first, verify, out,
            out_pcm, status);
        AMT_LAUNCH_CHECK();
    }
    if (verify == 2) {
        fl_md5_consts kc;
        fl_md5_fill(kc);
        flacdec_md5_kernel<<<n, AMT_FD_LANES, 0, stream>>>(out, stream_meta, data_bytes, n_cand, out_values, expect_md5,
                                                           md5, status, kc);
        AMT_LAUNCH_CHECK();
    }
    return AMT_OK;
}

}  // extern "C"
