// Spectral subtraction + ReLU + next ref_mag, fused, for gfx950.
//
// Replaces audio_complete.subtract (/root/reference/util_audio.py:221-259):
//     mag_sub  = guess.mag * (self.ref_mag / guess.ref_mag)   [normalize]
//     mag_sub *= overkill_factor
//     self.mag[:, off:off+Tg'] -= mag_sub[:, :Tg']             (Tg' clipped to the window end)
//     self.mag = max(self.mag, 0)                              [relu]
// and the np.max(self.mag) the reference re-evaluates on the next ref_mag read
// (the mag setter clears _ref_mag, util_audio.py:149-157, :170-174).
//
// HBM-bound elementwise pass over frame-major [T][ldf] windows: float4 (16 B
// per lane) loads/stores, one atomicMax per workgroup.  Arithmetic is kept
// un-fused (__fmul_rn / __fsub_rn, IEEE divide) so the residual is bit-identical
// to numpy's float32 result on the same inputs.
//
// subtract_span_kernel<true> is the span step that also keeps what it removed: before - after of every element, added
// into the stem of the note's instrument group at the song's own pool frames (what the reference dumps as _guessed.flac
// beside _after_subtr.flac, training.py:426-447).  The compiler is free to use packed-FP32 instructions in this file
// (DESIGN 10.1): every launch of it belongs on the one compute stream, never beside the networks on a side stream.
#include "amt_ordered.h"

// The step on a float4, stated once.  r - (q * scale) * overkill, un-fused and in this operand order, is numpy's
// float32 `mag_sub = guess * scale; mag_sub *= overkill; mag -= mag_sub` bit for bit; sub_relu4 is the step with its
// `max(mag, 0)`.  The whole-window kernel applies the two halves apart: its ReLU is optional and covers every frame.
__device__ __forceinline__ float4 sub4(float4 r, float4 q, float scale, float overkill) {
    r.x = __fsub_rn(r.x, __fmul_rn(__fmul_rn(q.x, scale), overkill));
    r.y = __fsub_rn(r.y, __fmul_rn(__fmul_rn(q.y, scale), overkill));
    r.z = __fsub_rn(r.z, __fmul_rn(__fmul_rn(q.z, scale), overkill));
    r.w = __fsub_rn(r.w, __fmul_rn(__fmul_rn(q.w, scale), overkill));
    return r;
}
__device__ __forceinline__ float4 relu4(float4 r) {
    return make_float4(fmaxf(r.x, 0.f), fmaxf(r.y, 0.f), fmaxf(r.z, 0.f), fmaxf(r.w, 0.f));
}
__device__ __forceinline__ float4 sub_relu4(float4 r, float4 q, float scale, float overkill) {
    return relu4(sub4(r, q, scale, overkill));
}
// max(m, the bins of r -- bins f .. f + 3 of a row -- that lie below F): pad columns stay out of the max
__device__ __forceinline__ float max_live4(float m, float4 r, int f, int F) {
    if (f < F) m = fmaxf(m, r.x);
    if (f + 1 < F) m = fmaxf(m, r.y);
    if (f + 2 < F) m = fmaxf(m, r.z);
    if (f + 3 < F) m = fmaxf(m, r.w);
    return m;
}

__global__ __launch_bounds__(256) void subtract_kernel(amt_subtract_args a,
                                                        unsigned int *__restrict__ new_max_ord) {
    __shared__ float red[16];
    const int b = blockIdx.y;
    const int g = a.guess_index ? a.guess_index[b] : b;
    const int tg = a.guess_frames ? a.guess_frames[b] : a.guess_frames_all;
    int off = a.offset_frames ? a.offset_frames[b] : 0;
    if (off < 0) off = 0;
    int t_end = off + tg;                               // exclusive; clipped to T (:250-251)
    if (t_end > a.T) t_end = a.T;
    float scale = 1.0f;
    if (a.normalize) scale = __fdiv_rn(a.resid_max[b], a.guess_max[g]);
    const float overkill = a.overkill_factor;

    float4 *r4 = reinterpret_cast<float4 *>(a.resid + (size_t)b * a.resid_stride);
    const float4 *g4 = reinterpret_cast<const float4 *>(a.guess + (size_t)g * a.guess_stride);
    const int ld4 = a.ldf >> 2;
    const int n4 = a.T * ld4;
    float m = -INFINITY;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x) {
        const int t = i / ld4;
        const int f4 = i - t * ld4;
        float4 r = r4[i];
        if (t >= off && t < t_end) r = sub4(r, g4[(size_t)(t - off) * ld4 + f4], scale, overkill);
        if (a.relu) r = relu4(r);                       // the whole window's, outside the span too (util_audio.py:259)
        r4[i] = r;
        m = max_live4(m, r, f4 << 2, a.F);
    }
    if (new_max_ord) {
        m = block_max(m, red);
        if (threadIdx.x == 0) atomicMax(new_max_ord + b, float_to_ordered(m));
    }
}

// ---- the same step on the frames that change ------------------------------------------------------------------------
// Only frames [off, t_end) of a window differ after the subtraction (util_audio.py:250-259 slices them out); when the
// residual is non-negative everywhere -- magnitudes, or the result of an earlier ReLU -- the ReLU leaves every other
// frame as it is, and np.max(self.mag) is the maximum of per-frame maxima of which only those frames' change.  With a
// per-frame maximum array kept beside the spectrogram (amt_compress_bands_fmax writes it while it has each frame in
// registers) the step reads and writes the guess's span instead of the window: ~2.0 instead of 4.9 MB per window and
// iteration at the loop's 173-frame guesses.  One wave per frame, float4 per lane, subtract_kernel's arithmetic
// (sub_relu4): bit-identical residuals and maxima.
//
// STEMS: the step keeps what it removed, a third stream.  Window row t of slot b is song frame offset[b] + t, pool row
// frame_base[b] + that, of stem prog_group[clamp(program[b])] (the clamp of note_select_kernel; the group clamped into
// [0, G)).  The removed amount is before - after with after the ReLU'd residual -- the clipped amount, not the scaled
// guess -- so that residual + sum of stems telescopes back to the song's magnitudes.  Rows at or past t_song (zero
// padding in the window, ANOTHER song's region in the pool) or outside the pool are subtracted like every other row but
// their stem row is neither read nor written: a += 0 there would race with the other song's wave.  One wave owns a
// (slot, frame) row and slots own disjoint regions: plain loads and stores, no atomics.  __fsub_rn / __fadd_rn as in
// sub_relu4: numpy float32 reproduces every bit of the stems too.  Residual, frame_max and new_max are the same
// statements in both instantiations, bit for bit.
template <bool STEMS>
__global__ __launch_bounds__(256) void subtract_span_kernel(amt_subtract_args a, float *__restrict__ frame_max,
                                                             amt_stem_args s) {
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int g = a.guess_index ? a.guess_index[b] : b;
    const int tg = a.guess_frames ? a.guess_frames[b] : a.guess_frames_all;
    int off = a.offset_frames ? a.offset_frames[b] : 0;
    if (off < 0) off = 0;
    int t_end = off + tg;
    if (t_end > a.T) t_end = a.T;
    const int t = off + blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (t >= t_end) return;                                  // whole wave
    float scale = 1.0f;
    if (a.normalize) scale = __fdiv_rn(a.resid_max[b], a.guess_max[g]);
    const float overkill = a.overkill_factor;
    const int ld4 = a.ldf >> 2;
    float4 *r4 = reinterpret_cast<float4 *>(a.resid + (size_t)b * a.resid_stride) + (size_t)t * ld4;
    const float4 *g4 = reinterpret_cast<const float4 *>(a.guess + (size_t)g * a.guess_stride) + (size_t)(t - off) * ld4;
    int grp = 0;
    long long row = 0;                                       // the pool row of this window row
    bool keep = false;                                       // whole wave: the row has a stem row
    if constexpr (STEMS) {
        if (s.program && s.prog_group) {
            int pr = s.program[b];
            pr = pr < 0 ? 0 : (pr >= s.n_prog ? s.n_prog - 1 : pr);
            grp = s.prog_group[pr];
        }
        grp = grp < 0 ? 0 : (grp >= s.G ? s.G - 1 : grp);
        const long long sf = (long long)s.offset[b] + t;     // song frame of this window row
        row = s.frame_base[b] + sf;
        keep = sf >= 0 && sf < s.t_song[b] && row >= 0 && row < s.pool_frames;
    }
    float m = 0.f;
    if (keep) {
        float4 *s4 = reinterpret_cast<float4 *>(s.stems + ((size_t)grp * (size_t)s.pool_frames + (size_t)row) * a.ldf);
        for (int f4 = lane; f4 < ld4; f4 += 64) {
            const float4 o = r4[f4];                         // the three loads of an element ahead of its arithmetic
            const float4 q = g4[f4];
            float4 k = s4[f4];
            const float4 r = sub_relu4(o, q, scale, overkill);
            k.x = __fadd_rn(k.x, __fsub_rn(o.x, r.x));
            k.y = __fadd_rn(k.y, __fsub_rn(o.y, r.y));
            k.z = __fadd_rn(k.z, __fsub_rn(o.z, r.z));
            k.w = __fadd_rn(k.w, __fsub_rn(o.w, r.w));
            r4[f4] = r;
            s4[f4] = k;
            m = max_live4(m, r, f4 << 2, a.F);
        }
    } else {
        for (int f4 = lane; f4 < ld4; f4 += 64) {
            const float4 r = sub_relu4(r4[f4], g4[f4], scale, overkill);
            r4[f4] = r;
            m = max_live4(m, r, f4 << 2, a.F);
        }
    }
    m = wave_max(m);
    if (lane == 0) frame_max[(size_t)b * a.T + t] = m;
}
__global__ __launch_bounds__(256) void frames_max_kernel(const float *__restrict__ frame_max, int T, float *__restrict__ out) {
    __shared__ float red[16];
    const float *row = frame_max + (size_t)blockIdx.x * T;
    float m = 0.f;
    for (int t = threadIdx.x; t < T; t += 256) m = fmaxf(m, row[t]);
    m = block_max(m, red);
    if (threadIdx.x == 0) out[blockIdx.x] = m;
}

// the host checks every entry shares, in the order their status codes are pinned; need_relu: the span step's refusal
static int subtract_check(const amt_subtract_args *args, bool need_relu) {
    if (!args || !args->resid || !args->guess) return AMT_E_INVALID;
    const amt_subtract_args &a = *args;
    if (a.B <= 0 || a.T <= 0 || a.F <= 0 || a.ldf < a.F || (a.ldf & 3)) return AMT_E_SHAPE;
    if ((a.resid_stride & 3) || (a.guess_stride & 3)) return AMT_E_SHAPE;
    if (a.resid_stride < (size_t)a.T * a.ldf) return AMT_E_SHAPE;
    if (need_relu && !a.relu) return AMT_E_UNSUPPORTED;       // the other frames are only untouched by a ReLU of >= 0 values
    if (a.normalize && (!a.resid_max || !a.guess_max)) return AMT_E_INVALID;
    if (!a.guess_frames && a.guess_frames_all < 0) return AMT_E_INVALID;
    return AMT_OK;
}

// the span step behind its two entries: the checks (the stem's after the step's own), the launch, the window maxima
template <bool STEMS>
static int span_launch(const amt_subtract_args *args, float *frame_max, int span_cap, const amt_stem_args *stem,
                       void *stream) {
    if (!frame_max) return AMT_E_INVALID;
    const int status = subtract_check(args, true);
    if (status != AMT_OK) return status;
    const amt_subtract_args &a = *args;
    if (span_cap <= 0) return AMT_E_INVALID;                  // >= every window's guess_frames (the guess tensor's frame count)
    // a uniform frame count beyond the launch's frame grid would be left unsubtracted (per-window counts live on the
    // device: their bound is the caller's contract, span_cap = the guess tensor's frame count)
    if (!a.guess_frames && a.guess_frames_all > span_cap) return AMT_E_SHAPE;
    if (STEMS) {
        if (!stem || !stem->stems || !stem->frame_base || !stem->offset || !stem->t_song) return AMT_E_INVALID;
        if (stem->G < 1 || stem->pool_frames < 1) return AMT_E_INVALID;
        if (stem->program && stem->prog_group && stem->n_prog < 1) return AMT_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    const int cap = span_cap < a.T ? span_cap : a.T;
    subtract_span_kernel<STEMS><<<dim3((cap + 3) / 4, a.B), 256, 0, st>>>(a, frame_max, STEMS ? *stem : amt_stem_args{});
    if (a.new_max) frames_max_kernel<<<a.B, 256, 0, st>>>(frame_max, a.T, a.new_max);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

extern "C" int amt_subtract_span(const amt_subtract_args *args, float *frame_max, int span_cap, void *stream) {
    return span_launch<false>(args, frame_max, span_cap, nullptr, stream);
}

extern "C" int amt_subtract_span_stems(const amt_subtract_args *args, float *frame_max, int span_cap,
                                       const amt_stem_args *stem, void *stream) {
    return span_launch<true>(args, frame_max, span_cap, stem, stream);
}

extern "C" int amt_subtract(const amt_subtract_args *args, void *stream) {
    const int status = subtract_check(args, false);
    if (status != AMT_OK) return status;
    const amt_subtract_args &a = *args;
    hipStream_t st = (hipStream_t)stream;
    unsigned int *nm = reinterpret_cast<unsigned int *>(a.new_max);
    if (nm) ordered_init_kernel<><<<(a.B + 255) / 256, 256, 0, st>>>(nm, a.B);
    const int n4 = a.T * (a.ldf >> 2);
    int gx = (n4 + 256 * 4 - 1) / (256 * 4);            // ~4 float4 per thread
    if (gx < 1) gx = 1;
    // cap the grid at ~16 workgroups per CU worth of blocks and grid-stride the rest
    const long cap = 4096;
    if ((long)gx * a.B > cap) { gx = (int)(cap / a.B); if (gx < 1) gx = 1; }
    subtract_kernel<<<dim3(gx, a.B), 256, 0, st>>>(a, nm);
    if (nm) ordered_decode_kernel<><<<(a.B + 255) / 256, 256, 0, st>>>(nm, a.B);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}
