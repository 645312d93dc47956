// The song-resident sliding window (training.py:284, :296-328) for B songs at once, on the device.
//
// One live window W[b] = [T][ldf] magnitudes + [T][ldf][2] unit phases per song, cut from that song's spectrogram
// S[b] (one STFT per song, all songs packed frame-major in one buffer, frame_base[b] = first frame of song b).  Per step
// the host launches, for all songs and without reading anything back:
//   song_decide   onset / count / window maximum / finished -> the step's slide and detect masks (training.py:313-317)
//   song_wave     what audio_complete.wf holds for a window nothing was subtracted from yet: raw song samples
//                 (util_audio.py:322-327 section, :355-357 slice, :378 concat)
//   song_pack     the step's event records
//   song_slide    slice(half, 2 half) + section(offset + half, None, half) + concat (training.py:318-323)
// Decisions live in int32 masks; a song that neither slides nor detects is carried along untouched.
#include <type_traits>
#include "amt_common.h"

// ---- decision ----------------------------------------------------------------------------------------------------------
// One workgroup per song: the window maximum is the maximum of the per-frame maxima amt_compress_bands_fmax left
// (np.max(audio_w.mag), what audio_complete.ref_mag re-evaluates at the next subtraction, util_audio.py:170-174).
__global__ __launch_bounds__(256) void song_decide_kernel(
        const int32_t *__restrict__ onset, const float *__restrict__ frame_max, int T, const float *__restrict__ ref_mag,
        float silence, int half, int max_notes, const int32_t *__restrict__ finished, int32_t *__restrict__ count,
        int32_t *__restrict__ clean, int32_t *__restrict__ slide, int32_t *__restrict__ detect,
        int32_t *__restrict__ kind, int32_t *__restrict__ guess_frames, float *__restrict__ window_max) {
    __shared__ float red[16];
    const int b = blockIdx.x;
    const float *row = frame_max + (size_t)b * T;
    float m = 0.f;
    for (int t = threadIdx.x; t < T; t += 256) m = fmaxf(m, row[t]);
    m = block_max(m, red);
    if (threadIdx.x != 0) return;
    window_max[b] = m;
    int k, sl = 0, de = 0;
    if (finished[b]) k = AMT_SONG_FINISHED;
    else if (onset[b] >= half) { k = AMT_SONG_SLIDE; sl = 1; }
    else if (count[b] >= max_notes || m <= __fmul_rn(silence, ref_mag[b])) { k = AMT_SONG_FORCED_SLIDE; sl = 1; }
    else { k = AMT_SONG_DETECT; de = 1; }
    kind[b] = k;
    slide[b] = sl;
    detect[b] = de;
    if (de) { count[b] += 1; clean[b] = 0; }
    else if (guess_frames) guess_frames[b] = 0;          // amt_subtract / amt_subtract_span touch no frame of this song
}

// ---- the window's waveform while nothing has been subtracted ------------------------------------------------------------
// seg [B][K][S][3] = (first sample in the row, first sample in the song, length) for window position k = offset / half
// (host table: the sample arithmetic of section / slice / concat is Python float arithmetic on lengths, not data).
// Rows of songs that had a subtraction keep the iSTFT the caller wrote into their first `l_istft` samples; their tail
// is zeroed.
__global__ __launch_bounds__(256) void song_wave_kernel(
        const float *__restrict__ samples, const int64_t *__restrict__ sample_base, const int32_t *__restrict__ seg,
        int K, int S, const int32_t *__restrict__ offset, int half, const int32_t *__restrict__ clean,
        const int32_t *__restrict__ finished, float *__restrict__ wave, int L, size_t wave_stride, int l_istft) {
    const int b = blockIdx.y;
    float *row = wave + (size_t)b * wave_stride;
    const int k = offset[b] / half;
    if (!clean[b] || finished[b] || k >= K) {
        for (int j = l_istft + blockIdx.x * 256 + threadIdx.x; j < L; j += gridDim.x * 256) row[j] = 0.f;
        return;
    }
    const int32_t *sg = seg + ((size_t)b * K + k) * S * 3;
    const float *src = samples + sample_base[b];
    for (int j = blockIdx.x * 256 + threadIdx.x; j < L; j += gridDim.x * 256) {
        float v = 0.f;
        for (int s = 0; s < S; ++s) {
            const int d0 = sg[3 * s], s0 = sg[3 * s + 1], n = sg[3 * s + 2];
            if (j >= d0 && j < d0 + n) v = src[s0 + (j - d0)];
        }
        row[j] = v;
    }
}

// ---- events ----------------------------------------------------------------------------------------------------------
// {song, step, kind, pitch, program, velocity, onset_frame, end_frame, offset_frame}; onset / end are song frames
// (offset + the window frame); the note fields are -1 unless kind == detect, everything but song / step / kind / offset
// is -1 for a finished song.  The song index is read per slot where a slot carries one song after the other (slot_song,
// the song queue), song0 + slot where it does not.
__global__ void song_pack_kernel(int n, const int32_t *__restrict__ slot_song, int song0, int step,
                                 const int32_t *__restrict__ kind, const int32_t *__restrict__ pitch,
                                 const int32_t *__restrict__ program, const int32_t *__restrict__ velocity,
                                 const int32_t *__restrict__ onset, const int32_t *__restrict__ end,
                                 const int32_t *__restrict__ offset, int32_t *__restrict__ events /* [n][9] */) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int k = kind[i];
    const bool det = k == AMT_SONG_DETECT, live = k != AMT_SONG_FINISHED;
    int32_t *e = events + (size_t)i * 9;
    e[0] = slot_song ? slot_song[i] : song0 + i;
    e[1] = step;
    e[2] = k;
    e[3] = det && pitch ? pitch[i] : -1;
    e[4] = det && program ? program[i] : -1;
    e[5] = det && velocity ? velocity[i] : -1;
    e[6] = live ? offset[i] + onset[i] : -1;
    e[7] = live ? offset[i] + end[i] : -1;
    e[8] = offset[i];
}

// ---- slide -----------------------------------------------------------------------------------------------------------
// For every song with slide[b] != 0: rows half .. 2 half of the window move to 0 .. half (residual kept) and rows
// half .. 2 half are refilled with song frames [offset + 2 half, offset + 3 half) -- the second half of the window at
// the new offset -- zero past the song's last frame.  T = 2 half: source and destination rows of the move are
// disjoint, and one thread carries an element through both halves (read S, read W, write W, write W), so each byte
// moves once.  A row is ldf magnitudes + 2 ldf phase floats = 3 ldf / 4 float4.  State (offset, count, finished)
// advances in a second launch, after every workgroup has read the old offset.
//
// KEEP: in addition window rows r = 0 .. half - 1 (the residual that leaves the window, as it is before the move) are
// stored into pool frames frame_base[b] + offset[b] + r, for rows with offset[b] + r < t_song[b]: rows at or past the
// song's last frame are zero padding in the window and ANOTHER song's region in the pool.  Magnitudes only: the
// subtraction never touches a phase (util_audio.py:253-259), s_ph already is the residual's phase.
// Aliasing: `s_mag` is then read and written through the same pointer, which is therefore not __restrict__ (the plain
// slide's is, and the phases, only read, keep theirs).  Per song the kernel writes pool frames [offset, offset + half)
// and reads pool frames [offset + 2 half, offset + 3 half) of the same region: disjoint, and a region belongs to one
// song, so no thread reads a float another thread (of this or any workgroup) writes and no ordering between them is
// needed (the source order -- every load of an element before its stores -- would be right even if they did overlap;
// measured: the same time as with the store first).  The written frames have been consumed for good: the walk only
// reads forward (the next slides fetch later frames, an admission reads frames [0, T) of NEW regions).  Per row ldf
// floats more read and ldf more written than the plain slide's 12 ldf: 14 / 12 of its bytes.
template <bool KEEP> using pool_mag_t = std::conditional_t<KEEP, float *, const float *__restrict__>;
template <bool KEEP>
__global__ __launch_bounds__(256) void song_slide_kernel(
        float *__restrict__ w_mag, float *__restrict__ w_ph, size_t w_stride /* floats of one window's mag */,
        pool_mag_t<KEEP> s_mag, const float *__restrict__ s_ph,
        const int64_t *__restrict__ frame_base, const int32_t *__restrict__ t_song, const int32_t *__restrict__ slide,
        const int32_t *__restrict__ offset, int half, int ld4) {
    const int b = blockIdx.y;
    if (!slide[b]) return;                                        // whole workgroup: the window stays as it is
    const int row4 = 3 * ld4;
    const int n4 = half * row4;
    const int off = offset[b];
    const int first = off + 2 * half;                             // song frame that lands in window row `half`
    const int ts = t_song[b];
    const int64_t fb = frame_base[b];
    float4 *wm = reinterpret_cast<float4 *>(w_mag + (size_t)b * w_stride);
    float4 *wp = reinterpret_cast<float4 *>(w_ph + (size_t)b * w_stride * 2);
    auto *sm = reinterpret_cast<std::conditional_t<KEEP, float4 *, const float4 *>>(s_mag);
    const float4 *sp = reinterpret_cast<const float4 *>(s_ph);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int r = i / row4, c = i - r * row4;
        const int f = first + r;
        const bool have = f < ts;
        float4 fresh = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < ld4) {
            // every load first, then the stores: no load of s_mag has to wait behind a store through the same pointer
            float4 out;
            if constexpr (KEEP) out = wm[(size_t)r * ld4 + c];
            if (have) fresh = sm[(size_t)(fb + f) * ld4 + c];
            const float4 moved = wm[(size_t)(half + r) * ld4 + c];
            if constexpr (KEEP)
                if (off + r < ts) sm[(size_t)(fb + off + r) * ld4 + c] = out;
            wm[(size_t)r * ld4 + c] = moved;
            wm[(size_t)(half + r) * ld4 + c] = fresh;
        } else {
            const int c2 = c - ld4;
            if (have) fresh = sp[(size_t)(fb + f) * 2 * ld4 + c2];
            wp[(size_t)r * 2 * ld4 + c2] = wp[(size_t)(half + r) * 2 * ld4 + c2];
            wp[(size_t)(half + r) * 2 * ld4 + c2] = fresh;
        }
    }
}

__global__ void song_advance_kernel(int n, int half, const int32_t *__restrict__ slide, const int32_t *__restrict__ t_song,
                                    int32_t *__restrict__ offset, int32_t *__restrict__ count,
                                    int32_t *__restrict__ finished) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !slide[i]) return;
    const int o = offset[i] + half;
    offset[i] = o;
    count[i] = 0;
    if (o >= t_song[i]) finished[i] = 1;                           // training.py:296
}

// ---- admission (song queue) ------------------------------------------------------------------------------------------
// A finished slot is handed to the next song of the queue: admit[b] = 0 leaves slot b alone, admit[b] = 1 + j gives it
// the j-th newly admitted song (the new_* arrays are in admission order, the order the ragged STFT wrote them in).
// The window becomes song.section(0, None, T) (training.py:284): rows [0, T) = song frames [0, T), zero rows past the
// song's last frame.  Same shape as the slide: grid (chunks, B), a workgroup of a slot that is not admitted returns at
// once, a row is 3 ldf / 4 float4 (magnitudes, then phases), each byte moves once.  The slot's integers and tables are
// written by a second, small grid (one workgroup per slot); this kernel reads none of them -- only admit and the
// new_* arrays -- so the order of the two launches carries no meaning.
__global__ __launch_bounds__(256) void song_admit_kernel(
        float *__restrict__ w_mag, float *__restrict__ w_ph, size_t w_stride, const float *__restrict__ s_mag,
        const float *__restrict__ s_ph, const int32_t *__restrict__ admit, int n_new,
        const int64_t *__restrict__ new_frame_base, const int32_t *__restrict__ new_t_song, int T, int ld4) {
    const int b = blockIdx.y;
    const int j = admit[b] - 1;
    if (j < 0 || j >= n_new) return;                              // whole workgroup: the window stays as it is
    const int row4 = 3 * ld4;
    const int n4 = T * row4;
    const int ts = new_t_song[j];
    const int64_t fb = new_frame_base[j];
    float4 *wm = reinterpret_cast<float4 *>(w_mag + (size_t)b * w_stride);
    float4 *wp = reinterpret_cast<float4 *>(w_ph + (size_t)b * w_stride * 2);
    const float4 *sm = reinterpret_cast<const float4 *>(s_mag);
    const float4 *sp = reinterpret_cast<const float4 *>(s_ph);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int r = i / row4, c = i - r * row4;
        const bool have = r < ts;
        float4 fresh = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < ld4) {
            if (have) fresh = sm[(size_t)(fb + r) * ld4 + c];
            wm[(size_t)r * ld4 + c] = fresh;
        } else {
            const int c2 = c - ld4;
            if (have) fresh = sp[(size_t)(fb + r) * 2 * ld4 + c2];
            wp[(size_t)r * 2 * ld4 + c2] = fresh;
        }
    }
}

// one workgroup per slot: the slot's scalars by thread 0, its K x S x 3 rows of the piece table by all threads
__global__ __launch_bounds__(256) void song_admit_state_kernel(amt_song_admit_args a) {
    const int b = blockIdx.x;
    const int j = a.admit[b] - 1;
    if (j < 0 || j >= a.n_new) return;
    const int row = a.K * a.S * 3;
    if (a.seg && a.new_seg)
        for (int i = threadIdx.x; i < row; i += 256) a.seg[(size_t)b * row + i] = a.new_seg[(size_t)j * row + i];
    if (threadIdx.x != 0) return;
    a.frame_base[b] = a.new_frame_base[j];
    a.t_song[b] = a.new_t_song[j];
    if (a.sample_base) a.sample_base[b] = a.new_sample_base[j];
    if (a.slot_song) a.slot_song[b] = a.new_song[j];
    for (int k = 0; k < 4; ++k)
        if (a.ref[k] && a.new_ref[k]) a.ref[k][b] = a.new_ref[k][j];
    a.offset[b] = 0;
    a.count[b] = 0;
    a.finished[b] = 0;
    a.clean[b] = 1;
}

// the two event entries: slot_song NULL = records numbered song0 + slot
static int pack_events(int n, const int32_t *slot_song, int song0, int step, const int32_t *kind, const int32_t *pitch,
                       const int32_t *program, const int32_t *velocity, const int32_t *onset, const int32_t *end,
                       const int32_t *offset, int32_t *events, void *stream) {
    if (!kind || !onset || !end || !offset || !events || n <= 0) return AMT_E_INVALID;
    song_pack_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(n, slot_song, song0, step, kind, pitch, program,
                                                                        velocity, onset, end, offset, events);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

// the two slide entries: checks, the slide's grid, then the state
template <bool KEEP>
static int slide_launch(float *w_mag, float *w_ph, int B, int T, int ldf, size_t w_stride, pool_mag_t<KEEP> s_mag,
                        const float *s_ph, const int64_t *frame_base, const int32_t *t_song, const int32_t *slide,
                        int32_t *offset, int32_t *count, int32_t *finished, void *stream) {
    if (!w_mag || !w_ph || !s_mag || !s_ph || !frame_base || !t_song || !slide || !offset || !count || !finished)
        return AMT_E_INVALID;
    if (B <= 0 || T < 2 || (T & 1)) return AMT_E_INVALID;         // odd T: the two halves of the move would overlap
    if (ldf <= 0 || (ldf & 3) || (w_stride & 3) || w_stride < (size_t)T * ldf) return AMT_E_SHAPE;
    const int half = T / 2, ld4 = ldf >> 2;
    hipStream_t st = (hipStream_t)stream;
    int gx = (half * 3 * ld4 + 256 * 4 - 1) / (256 * 4);          // ~4 float4 (two reads, two writes each) per thread
    if (gx < 1) gx = 1;
    song_slide_kernel<KEEP><<<dim3(gx, B), 256, 0, st>>>(w_mag, w_ph, w_stride, s_mag, s_ph, frame_base, t_song, slide,
                                                         offset, half, ld4);
    song_advance_kernel<<<(B + 255) / 256, 256, 0, st>>>(B, half, slide, t_song, offset, count, finished);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

extern "C" {

int amt_song_admit(const amt_song_admit_args *args, void *stream) {
    if (!args) return AMT_E_INVALID;
    const amt_song_admit_args &a = *args;
    if (!a.w_mag || !a.w_ph || !a.s_mag || !a.s_ph || !a.admit || !a.new_frame_base || !a.new_t_song || !a.frame_base ||
        !a.t_song || !a.offset || !a.count || !a.finished || !a.clean)
        return AMT_E_INVALID;
    if ((a.sample_base && !a.new_sample_base) || (a.slot_song && !a.new_song) || (a.seg && !a.new_seg))
        return AMT_E_INVALID;
    if (a.B <= 0 || a.B > 65535 || a.n_new <= 0 || a.T <= 0) return AMT_E_INVALID;
    if (a.ldf <= 0 || (a.ldf & 3) || (a.w_stride & 3) || a.w_stride < (size_t)a.T * a.ldf) return AMT_E_SHAPE;
    if (a.seg && (a.K <= 0 || a.S <= 0)) return AMT_E_SHAPE;
    const int ld4 = a.ldf >> 2;
    hipStream_t st = (hipStream_t)stream;
    int gx = (a.T * 3 * ld4 + 256 * 4 - 1) / (256 * 4);          // ~4 float4 (one read, one write each) per thread
    if (gx < 1) gx = 1;
    song_admit_kernel<<<dim3(gx, a.B), 256, 0, st>>>(a.w_mag, a.w_ph, a.w_stride, a.s_mag, a.s_ph, a.admit, a.n_new,
                                                     a.new_frame_base, a.new_t_song, a.T, ld4);
    song_admit_state_kernel<<<a.B, 256, 0, st>>>(a);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

int amt_song_decide(const int32_t *onset, const float *frame_max, int B, int T, const float *ref_mag, float silence,
                    int half, int max_notes, const int32_t *finished, int32_t *count, int32_t *clean, int32_t *slide,
                    int32_t *detect, int32_t *kind, int32_t *guess_frames, float *window_max, void *stream) {
    if (!onset || !frame_max || !ref_mag || !finished || !count || !clean || !slide || !detect || !kind || !window_max)
        return AMT_E_INVALID;
    if (B <= 0 || T <= 0 || half <= 0 || max_notes < 1 || !(silence >= 0.f)) return AMT_E_INVALID;
    song_decide_kernel<<<B, 256, 0, (hipStream_t)stream>>>(onset, frame_max, T, ref_mag, silence, half, max_notes, finished,
                                                           count, clean, slide, detect, kind, guess_frames, window_max);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

int amt_song_wave(const float *samples, const int64_t *sample_base, const int32_t *seg, int B, int K, int S,
                  const int32_t *offset, int half, const int32_t *clean, const int32_t *finished, float *wave, int L,
                  size_t wave_stride, int l_istft, void *stream) {
    if (!samples || !sample_base || !seg || !offset || !clean || !finished || !wave) return AMT_E_INVALID;
    if (B <= 0 || K <= 0 || S <= 0 || half <= 0 || L <= 0 || l_istft < 0 || l_istft > L || wave_stride < (size_t)L)
        return AMT_E_SHAPE;
    int gx = (L + 256 * 8 - 1) / (256 * 8);
    song_wave_kernel<<<dim3(gx < 1 ? 1 : gx, B), 256, 0, (hipStream_t)stream>>>(
        samples, sample_base, seg, K, S, offset, half, clean, finished, wave, L, wave_stride, l_istft);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

int amt_song_pack_events(int n, int song0, int step, const int32_t *kind, const int32_t *pitch, const int32_t *program,
                         const int32_t *velocity, const int32_t *onset, const int32_t *end, const int32_t *offset,
                         int32_t *events, void *stream) {
    return pack_events(n, nullptr, song0, step, kind, pitch, program, velocity, onset, end, offset, events, stream);
}

int amt_song_pack_events_slots(int n, const int32_t *slot_song, int step, const int32_t *kind, const int32_t *pitch,
                               const int32_t *program, const int32_t *velocity, const int32_t *onset, const int32_t *end,
                               const int32_t *offset, int32_t *events, void *stream) {
    if (!slot_song) return AMT_E_INVALID;
    return pack_events(n, slot_song, 0, step, kind, pitch, program, velocity, onset, end, offset, events, stream);
}

int amt_song_slide(float *w_mag, float *w_ph, int B, int T, int ldf, size_t w_stride, const float *s_mag,
                   const float *s_ph, const int64_t *frame_base, const int32_t *t_song, const int32_t *slide,
                   int32_t *offset, int32_t *count, int32_t *finished, void *stream) {
    return slide_launch<false>(w_mag, w_ph, B, T, ldf, w_stride, s_mag, s_ph, frame_base, t_song, slide, offset, count,
                               finished, stream);
}

int amt_song_slide_keep(float *w_mag, float *w_ph, int B, int T, int ldf, size_t w_stride, float *s_mag,
                        const float *s_ph, const int64_t *frame_base, const int32_t *t_song, const int32_t *slide,
                        int32_t *offset, int32_t *count, int32_t *finished, void *stream) {
    return slide_launch<true>(w_mag, w_ph, B, T, ldf, w_stride, s_mag, s_ph, frame_base, t_song, slide, offset, count,
                              finished, stream);
}

}  // extern "C"
