// WAV sample data on the device for gfx950: a ragged batch of files' PCM bytes -> float waveforms in one launch, and a
// ragged batch of float signals -> the data bytes of PCM-16 / PCM-24 / float32 WAV files in one launch.
//
// Replaces, for WAV files, the librosa.load of audio_from_file (util_audio.py:962-964 of the reference) and the
// librosa.output.write_wav of audio_complete.save(flac=False) (util_audio.py:526-527).  The host parses the RIFF chunks
// (amt_saga/wav.py: read_header) and writes the 44 / 58 header bytes; everything per sample is here.  The sample rule is
// amt_pcm_core.h's.
//
// Design:
//  * a 256-thread workgroup takes tiles of AMT_PCM_TILE = 1024 consecutive VALUES (frames x channels, interleaved as in
//    the file) of one row; the grid is (tiles of the longest file, rows) and a workgroup walks on by the grid's width,
//    so files with channels take several tiles per workgroup.
//  * a thread takes PCM_RUN = 4 consecutive values: 4 c bytes, a whole number of 32-bit words for every container
//    width c.  A first-sample offset is any byte value, so the run is fetched as c + 1 ALIGNED words and shifted
//    (pcm_load_run); only the runs at the edges of the byte buffer go byte by byte.  The lanes of a wave then read one
//    contiguous 256 c byte span.
//  * the four results leave as one 16-byte store where the output address allows it (audio.wav_decode lays every file's
//    output on a 16-byte boundary), else as four dword stores.  Packing mirrors this: c aligned words per thread.
//  * the container width is a template argument chosen per workgroup (uniform: one row per blockIdx.y).
//  * no LDS, no atomics in unpack and pack.  The peak is a maximum of non-negative floats, whose bit patterns order as
//    unsigned integers: one atomicMax per workgroup on a zeroed word, exact in any order.
//  * every row is checked against both buffer sizes first (pcm_row_values / pcm_pack_bytes): all of it or nothing.
#include "amt_common.h"
#include "amt_pcm_core.h"
#include "amt_wg.h"

#define AMT_PCM_THREADS 256
#define AMT_PCM_TILE (AMT_PCM_THREADS * PCM_RUN)
#define AMT_PCM_PEAK_RUN 8                             /* samples a thread of the peak kernel loads at a time */
#define AMT_PCM_PEAK_SPAN (AMT_PCM_THREADS * AMT_PCM_PEAK_RUN)
#define AMT_PCM_PEAK_GROUPS 1024                       /* workgroups of a peak launch, over all signals */
#define AMT_PCM_MAX_GRID 65536                        /* workgroups along x: the rest is walked */

template <int C>
__device__ __forceinline__ void pcm_unpack_run(const unsigned char *__restrict__ data, pcm_i64 data_bytes, pcm_i64 off,
                                               pcm_i64 values, pcm_i64 v0, int kind, int bits, float *__restrict__ out,
                                               int *__restrict__ out_pcm) {
    const int nv = (int)(values - v0 < PCM_RUN ? values - v0 : PCM_RUN);
    uint32_t y[PCM_RUN];
    int32_t q[PCM_RUN];
    pcm_unpack_values<C>(data, data_bytes, off + v0 * C, nv, kind, bits, y, q);
    uint32_t *o = (uint32_t *)out + v0;                 // (bit patterns: a float32 file's NaN payloads pass untouched)
    if (nv == PCM_RUN && ((uintptr_t)o & 15) == 0) {
        *(uint4 *)o = make_uint4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
        for (int j = 0; j < PCM_RUN; ++j)
            if (j < nv) o[j] = y[j];
    }
    if (out_pcm && kind == PCM_KIND_INT) {
        int *p = out_pcm + v0;
        if (nv == PCM_RUN && ((uintptr_t)p & 15) == 0) {
            *(int4 *)p = make_int4(q[0], q[1], q[2], q[3]);
        } else {
#pragma unroll
            for (int j = 0; j < PCM_RUN; ++j)
                if (j < nv) p[j] = q[j];
        }
    }
}

__global__ __launch_bounds__(AMT_PCM_THREADS) void pcm_unpack_kernel(
    const unsigned char *__restrict__ data, pcm_i64 data_bytes, const pcm_i64 *__restrict__ meta,
    float *__restrict__ out, int *__restrict__ out_pcm, pcm_i64 out_values) {
    pcm_i64 row[PCM_META];
#pragma unroll
    for (int k = 0; k < PCM_META; ++k) row[k] = meta[(pcm_i64)blockIdx.y * PCM_META + k];
    const pcm_i64 values = pcm_row_values(row, data_bytes, out_values);        // 0: the row points outside
    const pcm_i64 off = row[0];
    const int kind = (int)row[3], c = (int)row[4], bits = (int)row[5];
    float *o = out + row[6];
    int *p = out_pcm ? out_pcm + row[6] : nullptr;
    for (pcm_i64 t0 = (pcm_i64)blockIdx.x * AMT_PCM_TILE; t0 < values; t0 += (pcm_i64)gridDim.x * AMT_PCM_TILE) {
        const pcm_i64 v0 = t0 + (pcm_i64)threadIdx.x * PCM_RUN;
        if (v0 >= values) continue;
        switch (c) {                                                            // (uniform over the workgroup)
        case 1: pcm_unpack_run<1>(data, data_bytes, off, values, v0, kind, bits, o, p); break;
        case 2: pcm_unpack_run<2>(data, data_bytes, off, values, v0, kind, bits, o, p); break;
        case 3: pcm_unpack_run<3>(data, data_bytes, off, values, v0, kind, bits, o, p); break;
        case 4: pcm_unpack_run<4>(data, data_bytes, off, values, v0, kind, bits, o, p); break;
        case 8: pcm_unpack_run<8>(data, data_bytes, off, values, v0, kind, bits, o, p); break;
        default: break;
        }
    }
}

__global__ __launch_bounds__(AMT_PCM_THREADS) void pcm_peak_kernel(
    const float *__restrict__ wave, const pcm_i64 *__restrict__ base, const pcm_i64 *__restrict__ len, pcm_i64 max_len,
    float *__restrict__ peak_out) {
    __shared__ float red[16];
    const int b = blockIdx.y;
    const pcm_i64 n_s = amt_clamp_len(len[b], max_len);
    if ((pcm_i64)blockIdx.x * AMT_PCM_PEAK_SPAN >= n_s) return;                // (whole workgroup)
    const float *x = wave + base[b];
    float m = 0.f;
    for (pcm_i64 c0 = (pcm_i64)blockIdx.x * AMT_PCM_PEAK_SPAN; c0 < n_s; c0 += (pcm_i64)gridDim.x * AMT_PCM_PEAK_SPAN) {
        float v[AMT_PCM_PEAK_RUN];                                              // eight independent loads in flight
#pragma unroll
        for (int k = 0; k < AMT_PCM_PEAK_RUN; ++k) {
            const pcm_i64 i = c0 + k * AMT_PCM_THREADS + threadIdx.x;
            v[k] = i < n_s ? fabsf(x[i]) : 0.f;
        }
#pragma unroll
        for (int k = 0; k < AMT_PCM_PEAK_RUN; ++k) m = fmaxf(m, v[k]);          // fmaxf keeps m where |x| is NaN
    }
    m = block_max(m, red);
    if (threadIdx.x == 0) atomicMax((unsigned int *)peak_out + b, __float_as_uint(m));   // m >= 0: bits order as uint
}

template <int C>
__device__ __forceinline__ void pcm_pack_run(const float *__restrict__ x, pcm_i64 n_s, pcm_i64 s0, int fmt, float divisor,
                                             unsigned char *__restrict__ dst) {
    const int nv = (int)(n_s - s0 < PCM_RUN ? n_s - s0 : PCM_RUN);
    uint32_t w[C];
    pcm_pack_words<C>(x + s0, nv, fmt, divisor, w);
    unsigned char *d = dst + s0 * C;
    if (nv == PCM_RUN && ((uintptr_t)d & 3) == 0) {
#pragma unroll
        for (int i = 0; i < C; ++i) ((uint32_t *)d)[i] = w[i];
    } else {
#pragma unroll
        for (int i = 0; i < PCM_RUN * C; ++i)
            if (i < nv * C) d[i] = (unsigned char)(w[i >> 2] >> (8 * (i & 3)));
    }
}

__global__ __launch_bounds__(AMT_PCM_THREADS) void pcm_pack_kernel(
    const float *__restrict__ wave, const pcm_i64 *__restrict__ base, const pcm_i64 *__restrict__ len, pcm_i64 max_len,
    int fmt, const float *__restrict__ peak, unsigned char *__restrict__ out, const pcm_i64 *__restrict__ out_base,
    pcm_i64 out_bytes) {
    const int b = blockIdx.y;
    const pcm_i64 n_s = amt_clamp_len(len[b], max_len), ob = out_base[b];
    if (pcm_pack_bytes(n_s, ob, fmt, out_bytes) == 0) return;                  // the signal's bytes would leave `out`
    const float *x = wave + base[b];
    const float divisor = peak ? pcm_norm_divisor(peak[b]) : 0.f;
    unsigned char *dst = out + ob;
    for (pcm_i64 t0 = (pcm_i64)blockIdx.x * AMT_PCM_TILE; t0 < n_s; t0 += (pcm_i64)gridDim.x * AMT_PCM_TILE) {
        const pcm_i64 s0 = t0 + (pcm_i64)threadIdx.x * PCM_RUN;
        if (s0 >= n_s) continue;
        if (fmt == PCM_FMT_PCM16) pcm_pack_run<2>(x, n_s, s0, fmt, divisor, dst);
        else if (fmt == PCM_FMT_PCM24) pcm_pack_run<3>(x, n_s, s0, fmt, divisor, dst);
        else pcm_pack_run<4>(x, n_s, s0, fmt, divisor, dst);
    }
}

static unsigned pcm_grid_x(long long longest, long long per_group) {
    long long g = (longest + per_group - 1) / per_group;
    if (g < 1) g = 1;
    return (unsigned)(g > AMT_PCM_MAX_GRID ? AMT_PCM_MAX_GRID : g);
}

extern "C" {

int amt_pcm_unpack_ragged(const unsigned char *data, long long data_bytes, const long long *stream_meta, int n,
                          long long max_frames, float *out, int *out_pcm, long long out_values, void *stream) {
    if (!data || !stream_meta || !out || n < 1 || n > 65535 || data_bytes < 0 || max_frames < 0 || out_values < 0)
        return AMT_E_INVALID;
    const dim3 grid(pcm_grid_x(max_frames, AMT_PCM_TILE), (unsigned)n);
    pcm_unpack_kernel<<<grid, AMT_PCM_THREADS, 0, (hipStream_t)stream>>>(data, data_bytes, stream_meta, out, out_pcm,
                                                                          out_values);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

int amt_pcm_peak_ragged(const float *wave, const long long *base, const long long *len, int n, long long max_len,
                        float *peak_out, void *stream) {
    if (!wave || !base || !len || !peak_out || n < 1 || n > 65535 || max_len < 0) return AMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    AMT_HIP_CHECK(hipMemsetAsync(peak_out, 0, sizeof(float) * (size_t)n, st));
    // every workgroup ends in one atomic on its signal's word, and atomics on one address are served one after another:
    // about AMT_PCM_PEAK_GROUPS workgroups in all (four per CU), each walking its share, not one per span
    unsigned gx = pcm_grid_x(max_len, AMT_PCM_PEAK_SPAN);
    const unsigned cap = (unsigned)((AMT_PCM_PEAK_GROUPS + n - 1) / n);
    if (gx > cap) gx = cap;
    const dim3 grid(gx, (unsigned)n);
    pcm_peak_kernel<<<grid, AMT_PCM_THREADS, 0, st>>>(wave, base, len, max_len, peak_out);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

int amt_pcm_pack_ragged(const float *wave, const long long *base, const long long *len, int n, long long max_len,
                        int fmt, const float *peak, unsigned char *out, const long long *out_base, long long out_bytes,
                        void *stream) {
    if (!wave || !base || !len || !out || !out_base || n < 1 || n > 65535 || max_len < 0 || out_bytes < 0 ||
        pcm_fmt_bytes(fmt) == 0)
        return AMT_E_INVALID;
    const dim3 grid(pcm_grid_x(max_len, AMT_PCM_TILE), (unsigned)n);
    pcm_pack_kernel<<<grid, AMT_PCM_THREADS, 0, (hipStream_t)stream>>>(wave, base, len, max_len, fmt, peak, out, out_base,
                                                                        out_bytes);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

}  // extern "C"
