/*
 * amt_saga.h -- C ABI of the MI355X (gfx950) hot path of AMT-SAGA.
 *
 * Drop-in boundary.  The reference (RobertKajnak/AMT-SAGA) is pure Python and
 * has no FFI; the boundary it does have is the object surface that
 * training.py calls.  Each entry point below names the
 * reference interface it replaces (paths relative to the upstream repo).  The
 * Python host shim in amt-saga_amd/amt_saga binds these with ctypes and keeps
 * the reference's class / method names on top.
 *
 * Conventions
 *   - every function returns an int status: AMT_OK (0) or a negative AMT_E_*;
 *     no exceptions cross the ABI.  amt_strerror() gives the text the Python
 *     shim raises as ValueError / RuntimeError (the reference raises
 *     ValueError, util_train_test.py:109-112, util_audio.py:207,505).
 *   - all data pointers are DEVICE pointers owned by the caller; sizes are
 *     explicit; `stream` is a hipStream_t passed as void*.  Calls enqueue work
 *     and return; nothing synchronises the device except amt_*_create.
 *   - spectra are FRAME-MAJOR in HBM:  spec[b][t][f], f contiguous, row pitch
 *     `ldf` floats (ldf >= n_fft/2+1, multiple of 4), window pitch
 *     `spec_stride` elements.  The reference's numpy layout is [f][t]; the
 *     Python shim transposes at the boundary.  Pad columns f in [F, ldf) are
 *     written as zero by every producer.
 *   - no hidden global state besides the handles returned by *_create.
 */
#ifndef AMT_SAGA_H
#define AMT_SAGA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMT_OK            0
#define AMT_E_INVALID    -1   /* bad argument (null pointer, non power-of-two n_fft, ...) */
#define AMT_E_SHAPE      -2   /* shape mismatch ("Invalid Input shape", util_train_test.py:109) */
#define AMT_E_HIP        -3   /* a HIP runtime call failed; see amt_last_hip_error() */
#define AMT_E_NOMEM      -4
#define AMT_E_UNSUPPORTED -5  /* topology / size outside what the kernels are built for */
#define AMT_E_ATTRIB     -6   /* "Requested attribute does not exist" (util_audio.py:207) */

int         amt_version(void);                 /* ABI version, currently 1 */
const char *amt_strerror(int status);
const char *amt_last_hip_error(void);          /* text of the last failing HIP call (thread-local) */
int         amt_device_info(int *cu_count, int *lds_bytes, char *arch, int arch_len);

/* ------------------------------------------------------------------------ *
 * STFT / iSTFT   (replaces librosa.stft / magphase / istft as called from
 * audio_complete.F / .mag / .ph / .wf, util_audio.py:88-168)
 * ------------------------------------------------------------------------ */
typedef struct amt_stft_plan amt_stft_plan;

/* n_fft: power of two in [256, 4096]; hop > 0; center as librosa (reflect pad
 * n_fft/2).  Uploads the twiddle / window table (computed in double). */
int amt_stft_plan_create(amt_stft_plan **plan, int n_fft, int hop, int center);
int amt_stft_plan_destroy(amt_stft_plan *plan);
/* frames produced for a signal of L samples: center ? 1 + L/hop : 1 + (L-n_fft)/hop */
int amt_stft_frames(const amt_stft_plan *plan, int L);

/* audio_complete.mag / .ph / .ref_mag (util_audio.py:139-174) in one pass:
 *   wave  [B][wave_stride]  f32, L valid samples per window
 *   mag   [B][T][ldf]       f32 = |STFT|
 *   phase [B][T][ldf]       float2 = exp(i*angle(STFT)) (1+0i where STFT == 0); may be NULL
 *   ref_max [B]             f32 = max(mag) per window (np.max(self.mag), :173); may be NULL
 * T must equal amt_stft_frames(plan, L). */
int amt_stft_mag(const amt_stft_plan *plan, const float *wave, int B, int L,
                 size_t wave_stride, float *mag, float *phase_ri, float *ref_max,
                 int T, int ldf, size_t spec_stride, void *stream);

/* amt_stft_mag for n signals of unequal lengths in ONE launch -- one STFT per song (training.py:265-269), center
 * (reflect) padding at each signal's own ends: signal i = samples[sample_base[i] .. + length[i]) of a packed buffer
 * of n_samples floats; its 1 + length[i] / hop frames are written frame-major from frame frame_base[i] of the packed
 * pool mag [pool_frames][ldf] / phase [pool_frames][ldf] float2 (may be NULL); ref_max [n] (may be NULL).
 * sample_base / frame_base int64 [n], length int32 [n]: device.  max_len = the longest length, total_len = the sum
 * of the lengths (host values: they size the grid).  The per-frame arithmetic is amt_stft_mag's: every signal's
 * result is bit-identical to amt_stft_mag on that signal alone.  A signal outside the buffers or too short for the
 * padding (length <= n_fft / 2) is left unwritten; the caller checks lengths and regions beforehand. */
int amt_stft_mag_ragged(const amt_stft_plan *plan, const float *samples, const int64_t *sample_base,
                        const int32_t *length, int n, int max_len, long long n_samples, long long total_len,
                        float *mag, float *phase_ri, float *ref_max, const int64_t *frame_base, long long pool_frames,
                        int ldf, void *stream);

/* audio_complete.wf getter, the `mag * ph -> librosa.istft` branch
 * (util_audio.py:94-97): wave_out[b][0 .. Lout) f32, Lout = hop*(T-1) centred,
 * n_fft + hop*(T-1) otherwise; wave_stride >= Lout.
 *   mag   [B][T][ldf] f32 and phase_ri [B][T][ldf] float2: spec_stride counts
 *         bins, as in amt_stft_mag (>= T*ldf; both arrays use it).
 *   phase_ri == NULL: `mag` is interleaved complex F, [B][T][ldf] float2 (row
 *         pitch 2*ldf floats).  spec_stride then counts FLOATS of that array,
 *         the elements as stored: one window is 2*T*ldf, and spec_stride must
 *         be even and >= 2*T*ldf.
 * A stride below one window (or odd, complex input) is AMT_E_SHAPE. */
int amt_istft(const amt_stft_plan *plan, const float *mag, const float *phase_ri,
              int B, int T, int ldf, size_t spec_stride, float *wave_out,
              size_t wave_stride, void *stream);

/* amt_istft for n signals of unequal lengths in ONE launch, the mirror of amt_stft_mag_ragged -- the song-length
 * audio_complete.wf of a residual spectrogram (util_audio.py:94-97), what the reference dumps to listen to what a
 * subtraction left (training.py:438-447: _full_window / _guessed / _after_subtr .flac).  Signal i = frames
 * [frame_base[i], + t_frames[i]) of the packed pool mag [pool_frames][ldf] / phase_ri [pool_frames][ldf] float2; its
 * hop * (t_frames[i] - 1) samples (centred) go to out[out_base[i] ...] of a buffer of n_out floats (any alignment).
 * frame_base / out_base int64 [n], t_frames int32 [n]: device.  max_frames = the longest t_frames (host value: it
 * sizes the grid; a longer signal is left unwritten).  Every signal is cut into segments as amt_istft cuts it for
 * B = 1, T = t_frames[i], with the same per-segment arithmetic: its samples are bit-identical to that call, whatever
 * else the launch holds.  A signal of one frame has no samples.  A signal whose frames or samples leave either buffer
 * is left unwritten; the caller checks regions beforehand.  Plans: the streaming form's, hop == n_fft / 4, n_fft in
 * {1024, 2048, 4096}, center = 1; anything else is AMT_E_UNSUPPORTED.  Packed-FP32 code: launch it on the one compute
 * stream, never beside the networks on a side stream. */
int amt_istft_ragged(const amt_stft_plan *plan, const float *mag, const float *phase_ri, const int64_t *frame_base,
                     const int32_t *t_frames, int n, int max_frames, long long pool_frames, int ldf, float *out,
                     const int64_t *out_base, long long n_out, void *stream);

/* np.max over each window's [T][ldf] block (audio_complete.ref_mag, :170-174) */
int amt_window_max(const float *spec, int B, int T, int ldf, size_t spec_stride,
                   float *out_max, void *stream);

/* ------------------------------------------------------------------------ *
 * Sample-rate conversion  (replaces the `sr=` argument and the mono=True downmix
 * of librosa.load as called from audio_from_file, util_audio.py:962-964)
 *
 * Rational polyphase resampling with a Kaiser-windowed sinc, zero phase:
 *   g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g, R = max(L, M), Z = 32, beta = 10, rolloff = 0.88
 *   h[k] = L (rolloff / R) sinc(rolloff k / R) I0(beta sqrt(1 - (k / (Z R))^2)) / I0(beta),   integer |k| <= Z R
 *   y[n] = sum over m with |n M - m L| <= Z R of x[m] h[n M - m L],   x[m] = 0 outside [0, n_in)
 * Output n sits at time n / sr_out: no delay to compensate.
 * ------------------------------------------------------------------------ */
typedef struct amt_resampler amt_resampler;

/* librosa.load(sr=...) (util_audio.py:962-964): the coefficient table of one rate pair, computed in double and
 * uploaded as f32.  AMT_E_INVALID: a rate <= 0, equal rates (the filter would still low-pass: the caller passes the
 * signal through instead), or R > 2048 (a table of more than 512 KB; 44100 against 48001). */
int amt_resampler_create(amt_resampler **rs, int sr_in, int sr_out);
int amt_resampler_destroy(amt_resampler *rs);
/* samples librosa.load(sr=...) (util_audio.py:962-964) returns for n_in of them: ceil(n_in L / M) */
long long amt_resample_length(const amt_resampler *rs, long long n_in);

/* librosa.load(sr=..., mono=True) (util_audio.py:962-964) for n signals in ONE launch: signal i is
 * in[in_base[i] .. + in_len[i] * channels), `channels` (1 .. 8) interleaved floats per sample, x[m] their mean; its
 * amt_resample_length(in_len[i]) outputs go to out[out_base[i] ..).  in_base / in_len / out_base int64 [n]: device.
 * in_floats / out_floats: sizes of the two buffers; max_out_len: the longest output (a host value: it sizes the
 * grid).  A signal whose region leaves either buffer is left unwritten; nothing outside the output regions is
 * written.  Every output is an f32 sum over its taps in ascending m: a signal's result depends on its samples alone
 * and is bit-identical alone and inside a batch, at any base. */
int amt_resample_ragged(const amt_resampler *rs, const float *in, const int64_t *in_base, const int64_t *in_len,
                        int n, int channels, long long in_floats, long long max_out_len,
                        float *out, const int64_t *out_base, long long out_floats, void *stream);

/* ------------------------------------------------------------------------ *
 * FLAC encoder  (replaces the soundfile.write of audio_to_flac, util_audio.py:966-968, for audio that is already on
 * the device: the residual and the stems of a song walk)
 *
 * Mono, bps in {16, 24}, fixed block size in [16, 4096] (the last block of a signal shorter), one subframe per frame:
 * CONSTANT, FIXED order 0..4 with partitioned Rice2 coding, or VERBATIM, chosen by exact bit count (smallest bits,
 * then smallest partition order, then smallest predictor order; VERBATIM unless a FIXED form is strictly smaller).
 * q = clip(rint(y 2^(bps-1))), NaN -> 0.  All integer: every byte is defined.
 * ------------------------------------------------------------------------ */
/* audio_to_flac (util_audio.py:966-968): the largest frame in bytes, 13 + ceil((8 + blocksize bps) / 8) + 2 -- header,
 * VERBATIM subframe, CRC-16.  Negative (AMT_E_INVALID) for bps not in {16, 24} or blocksize outside [16, 4096].
 * Host only. */
long long amt_flac_frame_bound(int blocksize, int bps);
/* audio_to_flac (util_audio.py:966-968): bytes of `scratch` amt_flac_encode_ragged needs for n signals of at most
 * max_len samples, as amt_flac_make_layout (csrc/amt_scratch.h) lays it out: one slot of amt_flac_frame_bound bytes per
 * frame of an [n][frames(max_len)] grid, then the slots' int64 offsets.  Negative for invalid arguments.  Host only. */
long long amt_flac_scratch_bytes(int n, long long max_len, int blocksize, int bps);
/* audio_to_flac (util_audio.py:966-968) for n signals in ONE call: signal i = wave[base[i] .. + len[i]) (floats; base
 * may be any offset, negative included, that lands in memory the caller owns; a len above max_len is cut to max_len).
 * Its frames, numbered first_frame, first_frame + 1, ..., go to out[stream_off[i] .. stream_off[i + 1]) back to back;
 * frame_bytes [n][frames(max_len)] receives every frame's size (0 past a signal's last frame), stream_off [n + 1] the
 * byte offsets of the streams and their total, frame_minmax [2 n] each signal's smallest and largest frame (0, 0 for
 * an empty signal), md5 [16 n] the MD5 of each signal's little-endian PCM, as STREAMINFO wants it.  base, len and all
 * outputs: device.  max_len (host) sizes the grid.
 * AMT_E_INVALID: a NULL pointer, n < 1, bps not in {16, 24}, blocksize outside [16, 4096], first_frame < 0 or
 * first_frame + frames(max_len) >= 2^31.  AMT_E_SHAPE: scratch_bytes < amt_flac_scratch_bytes(...), or out_bytes <
 * frames(max_len) * bound (the longest signal alone must fit).  out_bytes >= (sum of the signals' frame counts) * bound
 * always suffices; a frame that would pass out_bytes is not copied, and stream_off[n] > out_bytes tells the caller.
 * All checks return before any HIP call.  Integer code without packed-FP32 instructions: any stream. */
int amt_flac_encode_ragged(const float *wave, const long long *base, const long long *len, int n, long long max_len,
                           int blocksize, int bps, long long first_frame, unsigned char *scratch,
                           long long scratch_bytes, unsigned char *out, long long out_bytes, long long *frame_bytes,
                           long long *stream_off, int *frame_minmax, unsigned char *md5, void *stream);
/* audio_to_flac (util_audio.py:966-968) as soundfile writes it, with linear prediction: amt_flac_encode_ragged with one
 * more family of candidates per block, LPC subframes of order m = 1 .. lpc_order (blocksize > m) after the FIXED orders.
 * Analysis (csrc/amt_flac_lpc_core.h): a Welch-like integer window, the exact int64 autocorrelation, a
 * float64 Levinson-Durbin recurrence in one written-out operation order, coefficients of 14 (24 bit) or 12 (16 bit) bits
 * with a shift in 0 .. 15; bits = 8 + m bps + 4 + 5 + m P + 6 + the residual coding of the fixed orders.  A candidate
 * replaces the best so far only if strictly smaller (FIXED wins a tie, then the smaller order); an order with a residual
 * |r| >= 2^27 is no candidate.  So no frame is larger than amt_flac_encode_ragged's for the same block: the frame bound,
 * the scratch layout and every other argument are that entry's, and so are its errors; in addition AMT_E_INVALID for
 * lpc_order outside 1 .. 12.  Every byte is defined (tests/flac_lpc_reference.py).  All checks return before any HIP
 * call.  No packed-FP32 instructions: any stream. */
int amt_flac_encode_lpc_ragged(const float *wave, const long long *base, const long long *len, int n, long long max_len,
                               int blocksize, int bps, long long first_frame, int lpc_order, unsigned char *scratch,
                               long long scratch_bytes, unsigned char *out, long long out_bytes, long long *frame_bytes,
                               long long *stream_off, int *frame_minmax, unsigned char *md5, void *stream);

/* ------------------------------------------------------------------------ *
 * FLAC decoder (replaces the librosa.load of audio_from_file, util_audio.py:962-964, for files whose bytes are put
 * on the device: the front of the song queue)
 *
 * The host parses STREAMINFO and lists the plausible frame headers (amt_saga/flac.py: read_streaminfo,
 * frame_candidates); the device decodes every candidate speculatively, follows the chain of frames that the
 * sequential reader would visit, checks CRC-16 and MD5, and writes interleaved samples.  Subset: 1 .. 8 channels,
 * all four channel assignments, CONSTANT / VERBATIM / FIXED 0..4 / LPC 1..32 subframes, Rice and Rice2 with escapes,
 * wasted bits, block sizes 1 .. 65536, bps 4 .. 24 (above 24 is refused: float32 is exact to 24 bits).  DESIGN.md 16.
 * ------------------------------------------------------------------------ */
/* audio_from_file (util_audio.py:962-964): bytes of `scratch` amt_flac_decode_ragged needs for n_cand candidates whose
 * slots (channels * block size int32 each) sum to slot_ints, as fd_make_layout (csrc/amt_flacdec_core.h) lays it out:
 * the slots, then two int64 per candidate.  Negative for invalid arguments.  Host only. */
long long amt_flac_decode_scratch_bytes(long long n_cand, long long slot_ints);
/* audio_from_file (util_audio.py:962-964) for n streams in ONE call.  data [data_bytes]: the files' bytes.
 * stream_meta int64 [n][9]: byte offset in data, size, first frame byte (relative to the offset), channels, bps, total
 * samples per channel, first output value, first and one-past-last candidate.  cand_meta int64 [n_cand][7], sorted by
 * position inside a stream: stream, position (relative), header bytes (CRC-8 included), block size, channel
 * assignment, frame bps, slot offset in int32.  expect_md5 [n][16]: STREAMINFO's digests (all zero: none).
 * verify: 0 nothing, 1 CRC-16 of every on-chain frame, 2 CRC-16 and MD5.
 * out [out_values] float32 pcm 2^-(bps-1), stream i at its first output value, interleaved [samples][channels];
 * out_pcm: the int32 PCM in the same layout, or NULL.  status int64 [n][4]: code (0 ok, 1 no candidate where the chain
 * arrived, 2 the frame there does not decode, 5 a table entry out of range), the byte it speaks of, the first byte of
 * the lowest frame whose CRC-16 fails (INT64_MAX: none), 1 if the MD5 differs.  cand_out int64 [n_cand][3]: end byte,
 * frame error (0 ok, 1 stream ends inside, 2 format, 3 sample out of range, 4 bps above 24, 5 table), on-chain flag.
 * md5 [n][16]: written with verify 2.  All tables and outputs: device.  Every stream-derived index is checked on the
 * device; nothing outside the outputs and the scratch is written, whatever the bytes or the tables hold.
 * AMT_E_INVALID: a NULL pointer (out_pcm excepted), n < 1, a negative size, verify outside 0 .. 2.  AMT_E_SHAPE:
 * scratch_bytes < amt_flac_decode_scratch_bytes(n_cand, slot_ints).  All checks return before any HIP call.  Integer
 * code without packed-FP32 instructions: any stream. */
int amt_flac_decode_ragged(const unsigned char *data, long long data_bytes, const long long *stream_meta, int n,
                           const long long *cand_meta, long long n_cand, const unsigned char *expect_md5, int verify,
                           unsigned char *scratch, long long scratch_bytes, long long slot_ints, float *out,
                           int *out_pcm, long long out_values, long long *status, long long *cand_out,
                           unsigned char *md5, void *stream);

/* ------------------------------------------------------------------------ *
 * WAV sample data  (replaces, for WAV files, the librosa.load of audio_from_file, util_audio.py:962-964, and the
 * librosa.output.write_wav of audio_complete.save(flac=False), util_audio.py:526-527)
 *
 * The host walks the RIFF chunks and writes the file headers (amt_saga/wav.py); the device turns the data chunk into
 * floats and floats into a data chunk.  Reading -- integer PCM, container c = 1 .. 4 bytes little-endian (c = 1
 * unsigned, u - 128), valid bits b = 1 .. 8 c, MSB-justified: q = container >> (8 c - b), wave = float32(q) 2^-(b-1)
 * (nearest even), pcm = q; float32: the bits as they are; float64: rounded to float32, nearest even.  Writing -- mono,
 * fmt 0 = PCM-16, 1 = PCM-24: q = clip(rint(y 2^(b-1)), -2^(b-1), 2^(b-1) - 1) on the float32 product, NaN -> 0 (the
 * FLAC encoder's rule); 2 = float32, the bits as they are.  DESIGN.md 18.
 * ------------------------------------------------------------------------ */
/* audio_from_file (util_audio.py:962-964) for the data chunks of n WAV files in ONE launch.  data [data_bytes]: the
 * files' bytes.  stream_meta int64 [n][8]: byte offset in data of the first sample (any value modulo 4), frames,
 * channels (1 .. 8), kind (0 integer, 1 float), container bytes, valid bits, first output value, reserved.  max_frames
 * (host) sizes the grid.  out [out_values] float32, file i at its first output value, interleaved [frames][channels];
 * out_pcm: the int32 q in the same layout, or NULL (rows of float kind write none).  Tables and buffers: device.
 * No byte at or past data_bytes is read and nothing at or past out_values is written, whatever the table holds: a row
 * whose geometry is none of the above, or whose bytes or values would leave either buffer, is left unwritten -- a bad
 * table costs output, never a fault.  AMT_E_INVALID: a NULL pointer (out_pcm excepted), n outside 1 .. 65535, a
 * negative size.  All checks return before any HIP call.  Integer code without packed-FP32 instructions: any stream. */
int amt_pcm_unpack_ragged(const unsigned char *data, long long data_bytes, const long long *stream_meta, int n,
                          long long max_frames, float *out, int *out_pcm, long long out_values, void *stream);
/* librosa.output.write_wav(norm=True) (util_audio.py:526-527), its inf-norm: peak_out[i] = max |y| over signal i =
 * wave[base[i] .. + len[i]) (conventions of amt_flac_encode_ragged), NaNs skipped; 0 for an empty or all-NaN signal.
 * A maximum: exact in any order.  peak_out float32 [n], device; zeroed by the call on `stream`.  AMT_E_INVALID: a NULL
 * pointer, n outside 1 .. 65535, max_len < 0. */
int amt_pcm_peak_ragged(const float *wave, const long long *base, const long long *len, int n, long long max_len,
                        float *peak_out, void *stream);
/* librosa.output.write_wav (util_audio.py:526-527) without the header, for n signals in ONE launch: signal i =
 * wave[base[i] .. + len[i]) (floats; base any offset the caller owns, a len above max_len is cut to max_len) becomes
 * the data bytes of `fmt` (0 PCM-16, 1 PCM-24, 2 float32) at out[out_base[i] ..).  peak: NULL, or float32 [n] -- each
 * sample is first y / peak[i], an IEEE float32 division; a peak of 0 or a non-finite one leaves the signal as it is.
 * base, len, peak, out_base: device.  A signal whose bytes would leave out[0 .. out_bytes) is left unwritten.
 * AMT_E_INVALID: a NULL pointer (peak excepted), n outside 1 .. 65535, a negative size, fmt outside 0 .. 2. */
int amt_pcm_pack_ragged(const float *wave, const long long *base, const long long *len, int n, long long max_len,
                        int fmt, const float *peak, unsigned char *out, const long long *out_base, long long out_bytes,
                        void *stream);

/* ------------------------------------------------------------------------ *
 * Spectrogram images on the device (replaces the librosa.display.specshow + matplotlib savefig of
 * audio_complete.plot_spec, util_audio.py:509-518, and plot_specs, util_audio.py:938-960)
 *
 * Two stages: magnitudes -> 8-bit level images (a comparison against 255 thresholds, no logarithm), and 8-bit images ->
 * complete PNG files (row filters, deflate with run-length matches and stored / fixed / dynamic Huffman blocks, Adler-32,
 * CRC-32, all on the device).  The rule of both lives in csrc/amt_png_core.h.  DESIGN.md 26.
 * ------------------------------------------------------------------------ */
/* The dB picture of audio_complete.D (util_audio.py:176-180) as plot_spec shows it (util_audio.py:509-518), for n
 * spectrograms in ONE launch.  mag: float32, frame-major; image i reads mag[mag_base + t ldf + f].  image_meta int64
 * [n][10], device: mag_base (floats), T, ldf, F, W, H, first int of its row table in `tables`, first int of its column
 * table, first output byte, reserved.  A row table is H pairs [bin lo, bin hi), row 0 the top of the image; a column
 * table is W pairs [frame lo, frame hi).  Pixel (j, i) = the number of k in 1 .. 255 with v >= thr[k - 1] * ref[image] (one
 * float32 product, rounded to nearest), v the float32 maximum over its bins and frames, NaN skipped, starting from 0.
 * thr float32 [255] ascending, ref float32 [n]: device.  A ref that is not finite or below 2^-100 gives an all-zero
 * image.  max_w, max_h (host) size the grid.  Nothing outside mag[0 .. mag_floats), tables[0 .. table_ints) or
 * out[0 .. out_bytes) is touched whatever the tables hold: an image whose geometry would leave them is left unwritten,
 * a table entry outside its axis is clamped.  AMT_E_INVALID: a NULL pointer, n outside 1 .. 65535, max_w or max_h
 * outside 1 .. 16384, a negative size. */
int amt_spec_levels_ragged(const float *mag, long long mag_floats, const long long *image_meta, int n, int max_w,
                           int max_h, const int *tables, long long table_ints, const float *thr, const float *ref,
                           unsigned char *out, long long out_bytes, void *stream);
/* Bytes of the largest PNG file amt_png_encode_ragged writes for a w x h image (palette: 0 or 1); negative
 * (AMT_E_INVALID) for w or h outside 1 .. 16384. */
long long amt_png_file_bound(int w, int h, int palette);
/* Scratch bytes of amt_png_encode_ragged for the n images of image_meta (host); negative for what that call refuses. */
long long amt_png_scratch_bytes(const long long *image_meta, int n);
/* matplotlib's savefig of plot_spec (util_audio.py:509-518) without the figure: n 8-bit images -> n complete PNG files
 * in one call (pieces -> sizes -> scan -> gather, as amt_flac_encode_ragged).  The call uploads its two small tables
 * into the scratch and waits for that upload on `stream`; the kernels are only enqueued.  image_meta int64 [n][3], HOST: first
 * byte of the image in pix, W, H; the image is H rows of W bytes.  pix [pix_bytes], device.  palette: 768 device bytes
 * (R, G, B of 256 entries; colour type 3), or NULL (greyscale, colour type 0).  out [out_bytes], device: file i at
 * [file_off[i], file_off[i + 1]); file_off int64 [n + 1], device.  out_bytes >= the sum of amt_png_file_bound over the
 * images and scratch_bytes >= amt_png_scratch_bytes, else AMT_E_SHAPE.  AMT_E_INVALID with nothing written: a NULL
 * pointer (palette excepted), a scratch that is not 16-byte aligned, n outside 1 .. 65535, W or H outside 1 .. 16384, an image outside pix. */
int amt_png_encode_ragged(const unsigned char *pix, long long pix_bytes, const long long *image_meta, int n,
                          const unsigned char *palette, void *scratch, long long scratch_bytes, unsigned char *out,
                          long long out_bytes, long long *file_off, void *stream);

/* ------------------------------------------------------------------------ *
 * Scoring transcriptions against gold notes (stands where the reference's users call mir_eval.transcription on the
 * MIDI/audio pairs it trains on, main.py:7).  The rule lives in csrc/amt_score_core.h.  DESIGN.md 27.
 *
 * Times are int64 microseconds, rint(seconds * 1e6) made on the host.  A pair is an estimated and a reference note list,
 * a note {pitch 0..127, program 0..127, on, off}, both lists sorted by (pitch, on, off, program).  An estimate e matches
 * a reference r when e.pitch == r.pitch and |e.on - r.on| <= 50000; in the offset variants also |e.off - r.off| <=
 * max(50000, (r.off - r.on) / 5), an integer division taken as 0 when r.off <= r.on; in the program variants also
 * group[e.program] == group[r.program].  The true positives of a variant are the size of a MAXIMUM-cardinality
 * matching of its graph (not of a first-fit pass).  Frame k >= 0 is the instant 10000 k us; cell (k, pitch) of a list is
 * set when a note of that pitch has on <= 10000 k < off; n_frames counts the k with 10000 k below the largest off of
 * either list.  Each pair yields int64 [10]: n_est, n_ref, tp_on, tp_onoff, tp_on_prog, tp_onoff_prog, frame_tp
 * (est & ref), frame_fp (est & ~ref), frame_fn (~est & ref), n_frames.
 * ------------------------------------------------------------------------ */
typedef struct amt_score_args {
    const int32_t *est_pitch, *est_program;   /* device [n_est_total]: the estimates of all pairs back to back */
    const int64_t *est_on, *est_off;
    const int32_t *ref_pitch, *ref_program;   /* device [n_ref_total] */
    const int64_t *ref_on, *ref_off;
    const int64_t *est_offsets_host;          /* HOST [n_pairs + 1]: pair i holds estimates [est_offsets[i], est_offsets[i + 1]) */
    const int64_t *ref_offsets_host;          /* HOST [n_pairs + 1] */
    const int64_t *est_offsets, *ref_offsets; /* device [n_pairs + 1]: the same numbers, what the kernel reads */
    const int32_t *group;                     /* device [128]: program -> group of the program variants */
    void          *scratch;                   /* device, 16-byte aligned: owner / visited / stack of the matchings */
    int64_t        scratch_bytes;             /* >= amt_score_scratch_bytes(est_offsets[n_pairs], ref_offsets[n_pairs]) */
    int64_t       *out;                       /* device [n_pairs][10] */
    int64_t        n_pairs;
} amt_score_args;
/* Scratch bytes of amt_score_pairs for that many notes per side over the whole call; negative (AMT_E_INVALID) for a
 * negative count or one above 2^40. */
long long amt_score_scratch_bytes(long long n_est_total, long long n_ref_total);
/* HOST arrays [n]: AMT_OK when every pitch and every program lies in 0..127, else AMT_E_INVALID.  The caller runs it on
 * what it is about to upload: the kernel masks a program and never indexes by a pitch, so a bad note costs a count,
 * never a fault, but it has no meaning under the rule. */
int amt_score_check_notes(const int32_t *pitch, const int32_t *program, long long n);
/* Any number of pairs in ONE launch; out is zeroed and the kernel enqueued on `stream`, nothing is waited for.  The work
 * item is one (pair, pitch): four waves find the four maximum matchings by augmenting paths with the candidates of a
 * reference spread over the lanes, a fifth sweeps the frames.  Lists of any length and augmenting paths of any length:
 * the matcher's arrays are in `scratch`.  The kernel reads the device offsets and holds every range inside the arrays
 * whatever they say; lists that are not sorted give other counts, never a fault.  All checks come before any HIP call.
 * AMT_E_INVALID: a NULL pointer, a scratch that is not 16-byte aligned, n_pairs < 0 or above 2^33, host offsets that
 * begin below 0 or decrease, a pair with more than 2^31 - 1 notes on a side.  AMT_E_SHAPE: scratch_bytes too small. */
int amt_score_pairs(const amt_score_args *args, void *stream);

/* ------------------------------------------------------------------------ *
 * Piano-roll images of note lists (stands where the reference's users plot a piano roll of a transcription against the
 * gold MIDI of the MIDI/audio pairs it trains on, main.py:7, with matplotlib).  The rule lives in csrc/amt_roll_core.h.
 * DESIGN.md 29.
 *
 * Times and lists are those of the scoring section: int64 microseconds, lists sorted by (pitch, on, off, program).  An
 * image is int64 [10]: W, row_px, pitch_lo, pitch_hi, t0, t1, tick, pair, first output byte, reserved (0) -- W in
 * 1..16384, 0 <= pitch_lo <= pitch_hi <= 127, row_px >= 1 with H = (pitch_hi - pitch_lo + 1) row_px <= 16384,
 * W <= t1 - t0 <= 2^40, |t0| <= 2^61, tick in 0..2^40, pair 0 or 1.  Column x is [c_x, c_{x+1}), c_x = t0 +
 * floor(x (t1 - t0) / W); pitch p owns rows (pitch_hi - p) row_px .. + row_px - 1.  A note covers [on, max(off, on + 1)).
 * Per side and pixel: j = the pitch's last note with on < c_{x+1}; onset = on_j >= c_x; covered = max_{i <= j} end_i >
 * c_x; the drawn note is j if it still sounds, else the first to attain that maximum.  Pixel: 0 / 1 (white / black key
 * row) + 2 on a column that holds a multiple of tick where nothing is covered; 16 + 2 (group[program of the drawn note]
 * mod 16) + onset for one list; 64 + 4 (est_covered | 2 gold_covered) + est_onset + 2 gold_onset for a pair.
 * ------------------------------------------------------------------------ */
typedef struct amt_roll_args {
    const int32_t *est_pitch, *est_program;   /* device [n_est_total]: the estimates of all images back to back */
    const int64_t *est_on, *est_off;
    const int32_t *gold_pitch, *gold_program; /* device [n_gold_total]; read for the images with pair = 1 */
    const int64_t *gold_on, *gold_off;
    const int64_t *est_offsets_host;          /* HOST [n_images + 1]: image i draws estimates [est_offsets[i], est_offsets[i + 1]) */
    const int64_t *gold_offsets_host;         /* HOST [n_images + 1] */
    const int64_t *est_offsets, *gold_offsets;/* device [n_images + 1]: the same numbers, what the kernel reads */
    const int64_t *image_meta_host;           /* HOST [n_images][10] */
    const int64_t *image_meta;                /* device [n_images][10]: the same numbers */
    const int32_t *group;                     /* device [128]: program -> group, drawn mod 16 */
    void          *scratch;                   /* device, 16-byte aligned: the running maxima */
    int64_t        scratch_bytes;             /* >= amt_roll_scratch_bytes(est_offsets[n_images], gold_offsets[n_images]) */
    uint8_t       *out;                       /* device [out_bytes]: image i is H rows of W bytes from its first output byte */
    int64_t        out_bytes;
    int64_t        n_images;
} amt_roll_args;
/* Scratch bytes of amt_roll_draw for that many notes per side over the whole call (what a piano-roll plot of the
 * reference's pairs, main.py:7, needs beside the lists); negative (AMT_E_INVALID) for a negative count or one above
 * 2^40. */
long long amt_roll_scratch_bytes(long long n_est_total, long long n_gold_total);
/* The piano rolls of any number of transcriptions, alone or against gold (the plot a user of the reference's MIDI/audio
 * pairs, main.py:7, makes on the host), in ONE launch enqueued on `stream`; nothing is waited for.  The work item is one
 * (image, pitch): a workgroup scans the pitch's notes into running maxima of their ends, finds every column's note by
 * binary search, and stores the pitch's row_px equal rows as one run with 16-byte stores.  No atomics: a byte does not
 * depend on the schedule.  The kernel reads the device tables and holds every range inside the arrays whatever they say;
 * an image whose device geometry would leave `out` is left unwritten; lists that are not sorted give other pixels, never a
 * fault.  Images must not overlap in `out`.  All checks come before any HIP call.  AMT_E_INVALID with nothing written: a
 * NULL pointer, a scratch that is not 16-byte aligned, n_images < 0 or above 2^24, host offsets that begin below 0 or
 * decrease, an image with more than 2^31 - 1 notes on a side, a geometry outside the limits above, an image outside
 * out[0 .. out_bytes).  AMT_E_SHAPE: scratch_bytes too small. */
int amt_roll_draw(const amt_roll_args *args, void *stream);

/* ------------------------------------------------------------------------ *
 * Harmonic/percussive separation of magnitude spectrograms by median filtering (Fitzgerald 2010), in front of the
 * transcription: the reference renders drum tracks into every training song (util_audio.py:843) and hands the heads
 * pitched notes only (relevant_notes(..., include_drums=False), util_train_test.py:83; validate_note rejects is_drum,
 * util_train_test.py:159), so a drum hit is energy no head can explain.  The rule lives in csrc/amt_hpss_core.h.
 * DESIGN.md 30.
 *
 * S [T][ldf] float32 frame-major with F <= ldf live bins, finite values in [0, 2^100].  idx(j, n) = j mod 2n
 * (non-negative), mapped to 2n - 1 - j where that is >= n.  Ht[t][f] = the median of S[idx(t + d, T)][f] over the kt
 * frames around t, Pf[t][f] the median of S[t][idx(f + d, F)] over the kf bins around f: exact, an input value.
 * soft(X, R): Z = max(X, R); Z < FLT_MIN -> 0.5 when both margins are 1, else 0; otherwise a = X / Z, b = R / Z, squared
 * when power == 2, a / (a + b), every operation single-rounded float32.  mask_h = soft(Ht, Pf margin_h), mask_p =
 * soft(Pf, Ht margin_p); power = inf: mask_h = (Ht >= Pf margin_h), mask_p = (Pf > Ht margin_p).  Sh = S mask_h,
 * Sp = S mask_p, and on request Sr = max((S - Sh) - Sp, 0).
 * ------------------------------------------------------------------------ */
typedef struct amt_hpss_args {
    const float   *mag;                       /* device [pool_frames][ldf]: the pool the signals lie in */
    float         *out_h, *out_p;             /* device, pools of the same shape: harmonic and percussive magnitudes */
    float         *out_r;                     /* device, a pool of the same shape, or NULL: max((S - Sh) - Sp, 0) */
    float         *med_t, *med_f;             /* device, pools of the same shape, or NULL: Ht and Pf */
    const int64_t *frame_base;                /* device [n]: signal i is frames [frame_base[i], + t_frames[i]) */
    const int32_t *t_frames;                  /* device [n] */
    int64_t        n;
    int64_t        pool_frames;
    int32_t        max_frames;                /* HOST value: the longest t_frames; it sizes the grid, a longer signal is left unwritten */
    int32_t        ldf, F;                    /* row pitch in floats (a multiple of 4) and live bins */
    int32_t        kt, kf;                    /* odd, 1..63 */
    float          power;                     /* 1, 2 or +inf */
    float          margin_h, margin_p;        /* 1..100 */
} amt_hpss_args;
/* The split of any number of spectrograms in ONE launch enqueued on `stream`, ahead of a transcription whose heads know
 * pitched notes only (util_audio.py:843, util_train_test.py:83, util_train_test.py:159); nothing is waited for.  The
 * tables are amt_istft_ragged's.  Outputs go to the signal's own frames of out_h / out_p (and out_r / med_t / med_f), pad columns
 * F..ldf-1 as zero; frames that belong to no signal are not written.  Reflection happens at the signal's own ends: a
 * signal's result is bit-identical to the same signal alone, whatever else the launch holds.  No atomics.  The kernel
 * reads the device tables and holds every range inside the pools whatever they say: a signal whose frames would leave
 * the pool, or with t_frames outside 1..max_frames, is left unwritten.  Signals must not overlap.  n = 0 and
 * max_frames = 0 are AMT_OK with nothing launched.  All checks come before any HIP call.  AMT_E_INVALID with nothing
 * written: a NULL pointer (out_r / med_t / med_f excepted), an output that is the input or another output, an even or
 * out-of-range kernel, a power other than the three, a margin outside [1, 100], F < 1, F > ldf, ldf % 4 != 0, a negative
 * count. */
int amt_hpss_ragged(const amt_hpss_args *args, void *stream);

/* ------------------------------------------------------------------------ *
 * Beat tracking by dynamic programming (Ellis 2007), behind the transcription: the reference stops at fixed-tempo
 * note_sequence files (add_note / save, util_audio.py:594-639, :790-792), so its MIDI has no bar a beat falls on.  The
 * rule lives in csrc/amt_beat_core.h: c = (int)(sqrtf(min(mag / ref, 1)) 1024 + 0.5f) in float32, integers from there on
 * -- flux, its excess over a local mean of half-width w, e in 1/256 of the excess's rms (uint16), the tempo from the
 * autocorrelation of e under a host-built prior, C[t] = ls[t] + max(0, max_tau (C[t - tau] - pen[P - lag_lo][tau])),
 * the backtrace and the trim.  Every tie rule is written out there.  DESIGN.md 31.
 *
 * Limits: F <= 2049, max_frames < 2^20, 1 <= lag_lo <= lag_hi <= 1024, w >= 0, n <= 2^24.
 * ------------------------------------------------------------------------ */
typedef struct amt_beat_env_args {
    const float   *mag;                       /* device [pool_frames][ldf]: the pool the songs lie in */
    const float   *ref;                       /* device [n]: each song's maximum magnitude; <= 0 or NaN: a song without beats */
    const int64_t *frame_base;                /* device [n]: song i is frames [frame_base[i], + t_frames[i]) */
    const int32_t *t_frames;                  /* device [n] */
    uint16_t      *env;                       /* device [pool_frames]: e, one value per frame */
    int32_t       *flux;                      /* device [pool_frames], or NULL: the flux before the local mean */
    void          *scratch;                   /* device, 16-byte aligned */
    int64_t        scratch_bytes;             /* >= amt_beat_scratch_bytes(n, pool_frames, 0, 0) */
    int64_t        n;
    int64_t        pool_frames;
    int32_t        max_frames;                /* HOST value: the longest t_frames; a longer song is left unwritten */
    int32_t        ldf, F;                    /* row pitch in floats and live bins */
    int32_t        w;                         /* half-width of the local mean, frames */
} amt_beat_env_args;
typedef struct amt_beat_track_args {
    const uint16_t *env;                      /* device [pool_frames] */
    const int64_t *frame_base;                /* device [n] */
    const int32_t *t_frames;                  /* device [n] */
    const int32_t *prior;                     /* device [lag_hi - lag_lo + 1], values <= 32767 */
    const int32_t *pen;                       /* device [lag_hi - lag_lo + 1][2 lag_hi + 1]: row P - lag_lo, entry tau */
    const int64_t *beat_base;                 /* device [n]: song i owns beats[beat_base[i], + t_frames[i] / ceil(lag_lo / 2) + 1) */
    int32_t       *period, *count;            /* device [n] */
    int32_t       *beats;                     /* device [beats_total]: count[i] ascending frames from beat_base[i] on */
    int64_t       *C;                         /* device [pool_frames], or NULL: the DP's scores */
    int32_t       *back;                      /* device [pool_frames], or NULL: the DP's predecessors */
    void          *scratch;                   /* device, 16-byte aligned */
    int64_t        scratch_bytes;             /* >= amt_beat_scratch_bytes(n, pool_frames, lag_hi, beats_total) */
    int64_t        n;
    int64_t        pool_frames;
    int64_t        beats_total;
    int32_t        max_frames;                /* HOST value: the longest t_frames */
    int32_t        lag_lo, lag_hi;
} amt_beat_track_args;
/* Scratch bytes of the two calls below, as amt_beat_make_layout (csrc/amt_scratch.h) lays it out (amt_beat_envelope
 * needs the bytes of lag_hi = 0, beats_total = 0; the larger size serves both); negative (AMT_E_INVALID) for a negative
 * count, lag_hi > 1024 or n > 2^24. */
long long amt_beat_scratch_bytes(long long n, long long pool_frames, int lag_hi, long long beats_total);
/* The onset envelopes of any number of spectrograms, the input of a beat track the reference's fixed-tempo files
 * (util_audio.py:594-639) lack: two launches enqueued on `stream`, nothing is waited for.  The tables are
 * amt_hpss_ragged's.  Each magnitude is read once (and one frame per run of 16 twice); pad columns F..ldf-1 are never
 * read; frames of no song are not written.  Integer reductions only: a song's result is bit-identical to the same song
 * alone.  The kernels read the device tables and hold every range inside the pool whatever they say: a song whose frames
 * would leave the pool, or with t_frames outside 0..max_frames, is left unwritten.  n = 0 and max_frames = 0 are AMT_OK
 * with nothing launched.  All checks come before any HIP call.  AMT_E_INVALID: a NULL pointer (flux excepted), a scratch
 * that is not 16-byte aligned, a limit above exceeded, F < 1, F > ldf, a negative count.  AMT_E_SHAPE: scratch_bytes
 * too small. */
int amt_beat_envelope(const amt_beat_env_args *args, void *stream);
/* Period, beat count and beat frames of every song from its envelope, for the tempo map the reference's note_sequence
 * files (util_audio.py:594-639) do not have: two launches enqueued on `stream` (the autocorrelations; then tempo, DP,
 * backtrace and trim, one workgroup per song), nothing is waited for and the period never leaves the device.  A song
 * without beats (amt_beat_core.h) gets period 0 and count 0.  A song whose frames would leave the pool, with t_frames
 * outside 0..max_frames or whose beats would leave `beats` gets period 0, count 0 and nothing else.  n = 0 is AMT_OK
 * with nothing launched.  All checks come before any HIP call.  AMT_E_INVALID: a NULL pointer (C and back excepted), a
 * scratch that is not 16-byte aligned, a limit above exceeded, a negative count.  AMT_E_SHAPE: scratch_bytes too small. */
int amt_beat_track(const amt_beat_track_args *args, void *stream);

/* ------------------------------------------------------------------------ *
 * Spectral subtraction (replaces audio_complete.subtract, util_audio.py:221-259)
 * ------------------------------------------------------------------------ */
typedef struct amt_subtract_args {
    float       *resid;          /* [B][T][ldf] in place (self.mag)                          */
    const float *resid_max;      /* [B] current ref_mag of each window, or NULL              */
    const float *guess;          /* base of the guess magnitudes, frame-major [.][Tg][ldf]   */
    const float *guess_max;      /* [n_guess] ref_mag of each guess, or NULL                 */
    const int32_t *guess_index;  /* [B] which guess each window subtracts; NULL => b         */
    const int32_t *guess_frames; /* [B] frames of each window's guess; NULL => guess_frames_all */
    const int32_t *offset_frames;/* [B] first frame (already max(..-attack_compensation,0));
                                    NULL => 0                                                */
    float       *new_max;        /* [B] out: np.max(self.mag) after the step, or NULL        */
    size_t       resid_stride;   /* elements between windows                                 */
    size_t       guess_stride;   /* elements between guesses                                 */
    int32_t      B, T, ldf, F;
    int32_t      guess_frames_all;
    int32_t      normalize;      /* scale by resid_max/guess_max (needs both arrays)         */
    int32_t      relu;
    float        overkill_factor;
} amt_subtract_args;

int amt_subtract(const amt_subtract_args *args, void *stream);

/* The same step on the frames that change (util_audio.py:250-259 writes only self.mag[:, off:off + Tg]): reads and
 * writes frames [offset, offset + guess_frames) of every window, updates their entries of frame_max [B][T] and sets
 * new_max[b] = max over t of frame_max[b][t].  Preconditions, the caller's: relu != 0; resid >= 0 everywhere (magnitudes,
 * or the output of an earlier step), so that the ReLU leaves the other frames as they are; frame_max[b][t] = the maximum
 * of resid's frame t over the F bins (amt_compress_bands_fmax leaves it).  span_cap >= every window's guess frame count
 * (the guess tensor's frames).  Residual and maxima are bit-identical to amt_subtract's. */
int amt_subtract_span(const amt_subtract_args *args, float *frame_max, int span_cap, void *stream);

/* amt_subtract_span that keeps what it removed -- the instrument stems of a song walk (the reference dumps exactly this
 * pair per subtraction, _guessed.flac beside _after_subtr.flac, training.py:426-447; the step itself is
 * audio_complete.subtract, util_audio.py:221-259).  Window row t of slot b is song frame offset[b] + t, i.e. pool row
 * frame_base[b] + offset[b] + t of every stem; the step adds before - after of each element of the row (after =
 * max(before - guess * scale * overkill, 0): the clipped amount, not the scaled guess) into stem
 * prog_group[clamp(program[b], 0, n_prog - 1)], the group clamped into [0, G).  program or prog_group NULL: stem 0.
 * Rows with offset[b] + t >= t_song[b] (zero padding in the window, another song's region in the pool) or outside
 * [0, pool_frames) are subtracted as ever, but their stem row is neither read nor written.  One wave owns a row and
 * slots own disjoint regions: no atomics.  Un-fused float32 (numpy reproduces every bit); residual, frame_max and
 * new_max are bit-identical to amt_subtract_span's on the same inputs.  Checks: amt_subtract_span's, and AMT_E_INVALID
 * for a NULL stems / frame_base / offset / t_song, G < 1, pool_frames < 1.  Packed-FP32 code: launch it on the one
 * compute stream, never beside the networks on a side stream. */
typedef struct amt_stem_args {
    float         *stems;        /* [G][pool_frames][ldf] */
    const int64_t *frame_base;   /* [B] first pool frame of the slot's song */
    const int32_t *offset;       /* [B] song frame of the window's frame 0 */
    const int32_t *t_song;       /* [B] frames of the slot's song */
    const int32_t *program;      /* [B] or NULL => stem 0 */
    const int32_t *prog_group;   /* [n_prog] or NULL => stem 0 */
    int32_t        n_prog, G;
    int64_t        pool_frames;
} amt_stem_args;
int amt_subtract_span_stems(const amt_subtract_args *args, float *frame_max, int span_cap,
                            const amt_stem_args *stem, void *stream);

/* ------------------------------------------------------------------------ *
 * Feature gathers (audio_complete.compress_bands :436-466, ._resize :384-409,
 * .resize :469-507, .section_power :334-349 and the recipe of
 * training.py:333-363).  Outputs are the NHWC head inputs [B][bands][frames].
 * ------------------------------------------------------------------------ */
/* C_timing = _resize(compress_bands(mag, bands), target) / ref   (training.py:333-336)
 *   edges [bands+1] int32 device (row ranges over f: util_audio.py:451-456)
 *   ref [B] device or NULL (=> 1): the song-level ref_mag the recipe divides by
 *   src_frame [target_frames] device or NULL (=> identity): source frame of every
 *   output column (-1 => zero column), i.e. _resize's tile/crop rule as a table
 *   out [B][bands][target_frames] f32 */
int amt_compress_bands(const float *mag, int B, int T, int F, int ldf, size_t spec_stride,
                       const int32_t *edges, int bands, const float *ref,
                       const int32_t *src_frame, float *out, int target_frames,
                       void *stream);
/* The same, also leaving frame_max [B][T] = max over the F bins of every frame (the kernel has the frame in registers):
 * what amt_subtract_span needs.  Identity frame map only (src_frame NULL, target_frames == T).  Any sign: the pad bins
 * beyond F take no part.  Spectra hold no NaN; if one does, fmaxf passes over it (a frame of NaNs alone gives -inf). */
int amt_compress_bands_fmax(const float *mag, int B, int T, int F, int ldf, size_t spec_stride,
                            const int32_t *edges, int bands, const float *ref,
                            const int32_t *src_frame, float *out, int target_frames,
                            float *frame_max, void *stream);

/* short-window gather: for every window b take frames src_frame[b][0..frames)
 * (-1 => zeros; the table realises _resize's tile/crop rule) and rows
 * [band_min[b], band_min[b]+bands) (zero past F; band_min NULL => 0):
 *   mode 0: out = mag / ref[b]  (ref NULL => 1)             (F_sw_inst_foc / _const, :350,:360)
 *   mode 1: out = log10(mag*1000+1) / max over the window  (.._log10, :353-354,:358-359)
 *   mode 2: out = (angle(phase)+3.15)/6.3                  (ph, :361-362)
 * out [B][bands][frames] f32. */
int amt_short_window(const float *mag, const float *phase_ri, int B, int T, int F,
                     int ldf, size_t spec_stride, const int32_t *src_frame,
                     int frames, const int32_t *band_min, int bands,
                     const float *ref, int mode, float *out, void *stream);

/* The FFT-side instrument towers of one step in ONE launch (training.py:347-363): for every window b the rows
 * [lo, lo + bands), lo = tone_bin[clamp(pitch[b] - tone_lo, 0, n_tones - 1)], of the frames src_frame[b][0..frames)
 * (zero where the frame is < 0 or >= T or the bin >= F), scaled three ways:
 *   out_lin   = mag / ref[b]  (ref NULL => 1)                         (F_sw_inst_foc / _const, :352,:361)
 *   out_log10 = log10(mag*1000+1) / its maximum over the window's tile (.._log10, :350-351,:359-360)
 *   out_phase = (angle(phase)+3.15)/6.3                               (ph, :362-363)
 * each NULL (not wanted) or [B][bands][frames] f32; a magnitude is read once however many are wanted.  Every output is
 * bit for bit what amt_short_window writes in the respective mode with band_min[b] = lo.
 *   pitch [B] int32 device: the step's decided MIDI pitches; NULL => const_tone for every window (the _const models'
 *   C4, training.py:289-290).  tone_bin [n_tones] int32 device: audio_complete.midi_tone_to_FFT (util_audio.py:278-284)
 *   of the tones tone_lo .. tone_lo + n_tones - 1, built on the host.
 * AMT_E_INVALID: a missing table, a non-positive count, or no output at all; AMT_E_ATTRIB: an output whose spectrum is
 * NULL; AMT_E_SHAPE: ldf < F; AMT_E_UNSUPPORTED: a tile (bands x (frames | 1) floats per staged output) beyond the LDS
 * of a workgroup. */
int amt_note_features(const float *mag, const float *phase_ri, int B, int T, int F, int ldf, size_t spec_stride,
                      const int32_t *src_frame, int frames, const int32_t *pitch, int const_tone,
                      const int32_t *tone_bin, int tone_lo, int n_tones, int bands, const float *ref,
                      float *out_lin, float *out_log10, float *out_phase, void *stream);

/* window management as index maps: audio_complete.section :286-328, .slice :351-365, .concat :374-382,
 * .resize :469-507 (column selection with zero padding) and .section_power :334-349 (band of bins):
 *   out[b][j][k] = src[b][src_frame[b*table_stride + j]][band_min + k]
 * zero where the frame index is < 0 or >= T, or the bin is >= F or k >= bands.  elem = floats per bin
 * (1 = magnitude / dB, 2 = unit phase or complex F).  table_stride 0 = one table for all windows.
 * out rows have ldf_out bins (>= bands); the pad is written as zero. */
int amt_gather_frames(const float *src, int B, int T, int F, int ldf_src, size_t src_stride, int elem,
                      const int32_t *src_frame, int table_stride, int n_out, int band_min, int bands,
                      float *out, int ldf_out, size_t out_stride, void *stream);

/* audio_complete.D getter (util_audio.py:176-180 -> librosa.amplitude_to_db(mag, ref=ref_mag)):
 *   D = 20 log10(max(amin, |mag|)) - 20 log10(max(amin, ref[b])), floored at max(D) - top_db
 * window_max[b] = max(mag[b]) (amt_window_max or the fused STFT max) supplies max(D); top_db < 0 = no floor.
 * librosa defaults: amin = 1e-5, top_db = 80. */
int amt_amplitude_to_db(const float *mag, int B, int T, int F, int ldf, size_t spec_stride, const float *ref,
                        const float *window_max, float amin, float top_db, float *out_db, void *stream);
/* librosa.db_to_amplitude as used by the mag / F / wf getters when only D is set (util_audio.py:101,124,145):
 *   mag = ref[b] * 10^(D / 20) */
int amt_db_to_amplitude(const float *db, int B, int T, int F, int ldf, size_t spec_stride, const float *ref,
                        float *out_mag, void *stream);

/* audio_complete.spectral_flatness (util_audio.py:330-332 -> librosa.feature.spectral_flatness, power 2):
 * out[b][t] = exp(mean_f log max(amin, mag^2)) / mean_f max(amin, mag^2); the reference takes np.mean over t
 * and skips a song whose render is white noise (> 0.3, training.py:266).  librosa default amin = 1e-10. */
int amt_spectral_flatness(const float *mag, int B, int T, int F, int ldf, size_t spec_stride, float amin,
                          float *out, void *stream);

/* ------------------------------------------------------------------------ *
 * Constant-Q slices (replaces audio_complete.slice_C, util_audio.py:411-434,
 * i.e. |librosa.cqt| evaluated only at the frames _resize keeps).  The
 * transform is the build's own spec (oracle/cqt.py); parity vs librosa is
 * unpinned.
 * ------------------------------------------------------------------------ */
typedef struct amt_cqt_args {
    const float   *wave;        /* [B][wave_stride], L valid samples                    */
    const int32_t *src_frame;   /* [B][frames] STFT-frame index of each output column, -1 => zeros; every index
                                 * lies in -1 .. T - 1, T = 1 + L / hop (the caller's duty: not checked on the device) */
    const int32_t *bin0;        /* [B] first bin of the table for each window, or NULL => 0 */
    const uint32_t *phase_inc;  /* [n_table] per-bin frequency, cycles/sample * 2^32    */
    const int32_t *length;      /* [n_table] filter length N_k in samples               */
    const float   *ref;         /* [B] divisor (ref_C_*, training.py:340-388) or NULL    */
    const float   *coef;        /* [n_table][192] per-bin phasor table from amt_cqt_coef() */
    float         *out;         /* [B][n_bins][frames]                                   */
    size_t         wave_stride;
    int32_t        B, L, hop, frames, n_bins, n_table;
} amt_cqt_args;

/* Block-sum kernel (needs coef) when hop is a power of two in 128..2048 and L / hop <= 1692, i.e. L < 1693 hop (the
 * block sums of L / hop + 3 blocks and their prefix sums live in 159 KiB of LDS); otherwise every frame is summed
 * directly over its own N_k samples (any L and hop, coef unused). */
int amt_cqt_slices(const amt_cqt_args *args, void *stream);

/* Complex form (util_audio.py:424-429 with magnitude_only=False: librosa.cqt's complex output is returned as is):
 * args->out receives the real parts, out_im the imaginary parts, both [B][n_bins][frames].  The phase refers to the
 * frame's centre (sample t * hop), where the analysis filter's own phase is zero -- the convention of a centred filter
 * bank; like the magnitudes, the values follow the build's CQT definition (oracle/cqt.py), not librosa's recursion. */
int amt_cqt_slices_complex(const amt_cqt_args *args, float *out_im, void *stream);

/* Per-bin phasor table of a CQT grid (32 x 3 unit complex numbers per bin, f64-evaluated): computed once per
 * (phase_inc, length) table and passed to amt_cqt_slices / amt_cqt_window_max.  coef: [n_table][192] floats. */
int amt_cqt_coef(const uint32_t *phase_inc, const int32_t *length, int n_table, float *coef, void *stream);

/* Song-level CQT normalisers (training.py:271-282: ref_C_* = np.max(mid_wf.slice_C(0, duration,
 * n_frames, pitch_frames, bins_per_tone=...)), the maximum of the whole CQT): out_max[b] = max over the
 * n_bins rows of the table and over EVERY frame t = 0 .. L/hop of |C[k, t]| of signal b -- a window, or a whole
 * song.  O(L) per bin whatever the filter length (prefix sums of per-hop block sums); hop a power of two in
 * 128..2048.  Up to L / hop = 1692 the block sums live in LDS; longer signals need
 * amt_cqt_window_max_workspace(L, hop, n_bins, B) bytes of device scratch (AMT_E_NOMEM if it is missing). */
size_t amt_cqt_window_max_workspace(int L, int hop, int n_bins, int B);
int amt_cqt_window_max(const float *wave, int B, int L, size_t wave_stride, int hop,
                       const uint32_t *phase_inc, const int32_t *length, const float *coef, int n_bins,
                       float *out_max, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------ *
 * Loop glue: predicted note -> integer decisions, gather tables, guess pick,
 * event records.  Restates per window what training.py:296-449 does with the
 * gold note (the reference never rounds: predict returns floats,
 * RDCNN.py:591-597; the rounding rules are rint / first argmax, as numpy).
 * ------------------------------------------------------------------------ */
/* out[i] = clamp(rint(x[i*stride]), lo, hi)  (half-to-even; NaN -> lo) */
int amt_round_clamp(const float *x, int n, int stride, int lo, int hi, int32_t *out,
                    void *stream);
/* out[i] = first argmax of p[i][0..K)  (np.argmax on a row without NaN).  A NaN is never selected: the
 * result is the first largest of the row's other elements (-inf included); a row of NaNs alone gives 0.
 * That is a decision, not numpy's rule (np.argmax returns the first NaN). */
int amt_argmax_rows(const float *p, int n, int K, int32_t *out, void *stream);
/* out[b][j] = source frame of column j of _resize(X[:, start[b]:end[b]], frames)
 * (util_audio.py:384-409 with numpy slice clamping to [0,T]); -1 = zero column */
int amt_resize_table(const int32_t *start, const int32_t *end, int n, int T, int frames,
                     int32_t *out, void *stream);
/* guess_index = prog_group[program]*n_pitch + (pitch-pitch_lo) (clamped);
 * guess_frames = min(max(end-onset,0) + tail_frames, bank_frames)
 * (the rendered guess = note + 1 s release, util_audio.py:876).  program /
 * prog_group may be NULL (=> group 0). */
int amt_note_select(const int32_t *program, const int32_t *pitch, const int32_t *onset,
                    const int32_t *end, const int32_t *prog_group, int n_prog, int n,
                    int pitch_lo, int n_pitch, int tail_frames, int bank_frames,
                    int32_t *guess_index, int32_t *guess_frames, void *stream);
/* events[i] = {window0+i, iter, pitch, program, velocity, onset_frame, end_frame}
 * (int32 x 7); NULL inputs are recorded as -1 */
int amt_pack_events(int n, int window0, int iter, const int32_t *pitch,
                    const int32_t *program, const int32_t *velocity, const int32_t *onset,
                    const int32_t *end, int32_t *events, void *stream);
/* out[i] = x[i]*mul + add (bin offsets of the focused CQT grids) */
int amt_affine_i32(const int32_t *x, int n, int mul, int add, int32_t *out, void *stream);

/* ------------------------------------------------------------------------ *
 * Song-resident sliding window (training.py:284, :296-328): one live window of
 * T = 2 half frames per song, cut from the song's own spectrogram.  All songs'
 * spectrograms are packed frame-major in one buffer (song b starts at frame
 * frame_base[b] and has t_song[b] frames), all songs' samples in another
 * (sample_base[b]).  Per-song state, int32 [B] on the device: offset (frames, a
 * multiple of half), count (notes detected at this offset), finished, clean
 * (1 until the first subtraction).  The predicted note stands where the
 * reference has the gold note; max_notes and silence stand for "no gold note
 * left in the window" (training.py:313-314) and are build-defined.
 * ------------------------------------------------------------------------ */
#define AMT_SONG_DETECT       0
#define AMT_SONG_SLIDE        1   /* onset >= half (training.py:317) */
#define AMT_SONG_FORCED_SLIDE 2   /* count == max_notes, or max(window) <= silence * ref_mag */
#define AMT_SONG_FINISHED     3   /* the song was finished before this step: an idle slot */
/* The step's decision for every song (training.py:313-317) from the rounded onset [B], the per-frame maxima of the
 * window (frame_max [B][T], as amt_compress_bands_fmax leaves them), the song-level ref_mag [B] and the state:
 *   finished                                      -> kind FINISHED
 *   onset >= half                                 -> kind SLIDE,        slide = 1
 *   count >= max_notes or window max <= silence * ref_mag (float32 product)
 *                                                 -> kind FORCED_SLIDE, slide = 1
 *   otherwise                                     -> kind DETECT, detect = 1, count += 1, clean = 0
 * window_max [B] = np.max(window mag) (what audio_complete.ref_mag re-evaluates before a subtraction,
 * util_audio.py:170-174).  guess_frames [B] (may be NULL) is set to 0 for every song that does not detect, which
 * makes amt_subtract / amt_subtract_span leave that song's window untouched. */
int amt_song_decide(const int32_t *onset, const float *frame_max, int B, int T, const float *ref_mag, float silence,
                    int half, int max_notes, const int32_t *finished, int32_t *count, int32_t *clean, int32_t *slide,
                    int32_t *detect, int32_t *kind, int32_t *guess_frames, float *window_max, void *stream);
/* audio_complete.wf of the live window (what slice_C reads, util_audio.py:411-434) for songs nothing was subtracted
 * from yet (clean != 0): the raw song samples that section (:322-327), slice (:355-357) and concat (:378) carry along.
 * seg [B][K][S][3] int32 = up to S pieces (first sample in the row, first sample in the song, length; length 0 =
 * unused) for each window position k = offset / half; the rest of the row is zero.  Rows of the other songs hold
 * the caller's iSTFT (:94-97) in their first l_istft samples; their tail [l_istft, L) is zeroed. */
int amt_song_wave(const float *samples, const int64_t *sample_base, const int32_t *seg, int B, int K, int S,
                  const int32_t *offset, int half, const int32_t *clean, const int32_t *finished, float *wave, int L,
                  size_t wave_stride, int l_istft, void *stream);
/* events[i] = {song0+i, step, kind, pitch, program, velocity, onset_frame, end_frame, offset_frame} (int32 x 9);
 * onset / end are song frames (offset + window frame); pitch / program / velocity are -1 unless kind == DETECT (and
 * where the pointer is NULL), onset / end are -1 for kind FINISHED. */
int amt_song_pack_events(int n, int song0, int step, const int32_t *kind, const int32_t *pitch, const int32_t *program,
                         const int32_t *velocity, const int32_t *onset, const int32_t *end, const int32_t *offset,
                         int32_t *events, void *stream);
/* training.py:318-323 for every song with slide[b] != 0: audio_w.slice(half, 2 half) (util_audio.py:351-365), then
 * concat (:374-382) of mid_wf.section(offset + half, None, half) (:286-328) at the advanced offset -- window rows
 * half..T move to 0..half (magnitudes w_mag [B][T][ldf] and unit phases w_ph [B][T][ldf][2], residual kept), rows
 * half..T are refilled with song frames [offset + T, offset + T + half), zero rows past t_song[b]; then
 * offset += half, count = 0, finished = (offset >= t_song) (:296).  Other songs are not touched.  w_stride = floats
 * between windows of w_mag (w_ph: twice that).  T must be even (the halves of an odd window overlap): AMT_E_INVALID.
 * Any per-frame maxima cached for the window are stale afterwards. */
int amt_song_slide(float *w_mag, float *w_ph, int B, int T, int ldf, size_t w_stride, const float *s_mag,
                   const float *s_ph, const int64_t *frame_base, const int32_t *t_song, const int32_t *slide,
                   int32_t *offset, int32_t *count, int32_t *finished, void *stream);
/* amt_song_slide that keeps what leaves the window: in addition, window rows r = 0 .. half - 1 of w_mag, as they are
 * before the move (the residual of every subtraction, training.py:449), are stored into pool frames
 * frame_base[b] + offset[b] + r of s_mag, for rows with offset[b] + r < t_song[b] only (later rows are zero padding in
 * the window and another song's region in the pool).  Phases are not written back: the subtraction changes magnitudes
 * only (util_audio.py:253-259).  The written frames [offset, offset + half) and the fetched ones [offset + T,
 * offset + T + half) are disjoint, and the walk never reads a frame again once it has left the window.  Every frame
 * below t_song leaves the window exactly once before `finished` is set, so a finished song's region [frame_base,
 * + t_song) of s_mag is its residual spectrogram -- with s_ph, what util_audio.py:94-97 resynthesises and
 * training.py:438-447 writes out (amt_istft_ragged).  Window and state end exactly as after amt_song_slide. */
int amt_song_slide_keep(float *w_mag, float *w_ph, int B, int T, int ldf, size_t w_stride, float *s_mag,
                        const float *s_ph, const int64_t *frame_base, const int32_t *t_song, const int32_t *slide,
                        int32_t *offset, int32_t *count, int32_t *finished, void *stream);

/* Song queue: a finished slot takes the next song (the reference walks one song after the other per worker,
 * training.py:623-634; here B slots do).  admit [B]: 0 = leave the slot alone, 1 + j = the slot takes the j-th of
 * the n_new songs described by the new_* arrays (device, admission order).  For an admitted slot:
 *   window rows [0, T) = song frames [0, T) of s_mag / s_ph from new_frame_base[j] (audio_w = section(0, None,
 *   timing_frames), training.py:284), zero rows past new_t_song[j];
 *   frame_base, t_song, sample_base, slot_song, ref[k] (the song-level constants of training.py:269-282, up to four,
 *   NULL = unused), the slot's [K][S][3] rows of amt_song_wave's piece table <- the new song's;
 *   offset = 0, count = 0, finished = 0, clean = 1.
 * Other slots are not touched.  Two launches, independent of each other: the window rows, then the slot's integers
 * and tables (the first reads none of them).  Any per-frame maxima cached for the windows are stale afterwards. */
typedef struct amt_song_admit_args {
    float *w_mag, *w_ph;                 /* [B][T][ldf], [B][T][ldf][2] */
    const float *s_mag, *s_ph;           /* the packed spectrogram pool */
    const int32_t *admit;                /* [B] */
    const int64_t *new_frame_base;       /* [n_new] */
    const int32_t *new_t_song;           /* [n_new] */
    const int64_t *new_sample_base;      /* [n_new] */
    const int32_t *new_song;             /* [n_new] song indices */
    const int32_t *new_seg;              /* [n_new][K][S][3] or NULL */
    const float *new_ref[4];             /* [n_new] each or NULL */
    int64_t *frame_base;                 /* [B] per-slot tables ... */
    int32_t *t_song;
    int64_t *sample_base;
    int32_t *slot_song;
    int32_t *seg;                        /* [B][K][S][3] or NULL */
    float *ref[4];
    int32_t *offset, *count, *finished, *clean;   /* [B] per-slot state */
    size_t w_stride;                     /* floats between windows of w_mag */
    int32_t B, n_new, T, ldf, K, S;
} amt_song_admit_args;
int amt_song_admit(const amt_song_admit_args *args, void *stream);
/* amt_song_pack_events with the song index of record i read from slot_song[i] (device) instead of song0 + i */
int amt_song_pack_events_slots(int n, const int32_t *slot_song, int step, const int32_t *kind, const int32_t *pitch,
                               const int32_t *program, const int32_t *velocity, const int32_t *onset, const int32_t *end,
                               const int32_t *offset, int32_t *events, void *stream);

/* ------------------------------------------------------------------------ *
 * Guess synthesis (stand-in for note_sequence.render(), util_audio.py:758-786:
 * fluidsynth + soundfont are not available).  Additive synth defined in
 * amt_saga/synth.py; window scaling follows render() (:778-781).
 * ------------------------------------------------------------------------ */
/* notes [B][max_notes][5] f32 = {preset group 0..2, midi pitch (<0 = unused slot),
 * velocity, onset s, duration s}; wave [B][wave_stride] f32 out (L samples);
 * peak_scratch [B] f32 device scratch. */
int amt_synth_windows(const float *notes, int max_notes, int B, int L, float sample_rate,
                      float *wave, size_t wave_stride, float *peak_scratch, void *stream);
/* Per-program timbres ("per-program timbres"; util_audio.py:758-786 renders every MIDI program through
 * its own soundfont preset): notes[..][0] indexes a caller-supplied table timbres [n_timbres][5] f32 (device) =
 * {harmonics H, spectral slope, decay tau s (0 = sustained), attack s, weight of the even harmonics}; the build's
 * table for the 128 General MIDI programs is amt_saga/synth.py:gm_timbre_table.  timbres == NULL: the three built-in
 * groups of amt_synth_windows. */
int amt_synth_windows_timbres(const float *notes, int max_notes, int B, int L, float sample_rate,
                              const float *timbres, int n_timbres, float *wave, size_t wave_stride,
                              float *peak_scratch, void *stream);
/* SoundFont 2 sample playback ("optionally SF2 sample playback if a soundfont is supplied";
 * util_audio.py:758-786 renders through fluidsynth + main.py's -soundfont_path): notes[..][0] is the MIDI program;
 * samples [n_samples] f32 = the font's 16-bit pool / 32768; zones [n_zones][20] f32 and first [n_prog + 1] i32 as
 * amt_saga/sf2.py:SoundFont.tables() lays them out (flattened preset x instrument zones of bank 0: ranges, sample
 * and loop points, tuning, attenuation, volume envelope).  Same amplitude law and 1 s tail as amt_synth_windows.
 * A note whose program is outside 0 .. n_prog - 1 plays nothing, like a program the font has no preset for (it is
 * still one of the window's notes for the amplitude law).
 * The zone table is trusted (the host parser validates offsets against the pool). */
int amt_sf2_synth_windows(const float *notes, int max_notes, int B, int L, float sample_rate, const float *samples,
                          int n_samples, const float *zones, int n_zones, const int32_t *first, int n_prog,
                          float *wave, size_t wave_stride, float *peak_scratch, void *stream);
/* one guess note per window from the loop's integer decisions:
 * {prog_group[program], pitch, velocity (or default), 0, min((end-onset)*frame_seconds, max_dur)}
 * (training.py:421-424 builds the guessed note the same way, from the gold values) */
int amt_guess_notes(const int32_t *program, const int32_t *pitch, const int32_t *velocity,
                    const int32_t *onset, const int32_t *end, const int32_t *prog_group,
                    int n_prog, int n, float frame_seconds, float max_dur,
                    float default_velocity, float *notes, void *stream);

/* ------------------------------------------------------------------------ *
 * RDCNN forward (replaces res_net.predict, RDCNN.py:591-597, for the graph
 * built by RDCNN.py:176-233).
 * ------------------------------------------------------------------------ */
typedef struct amt_rdcnn amt_rdcnn;

typedef struct amt_rdcnn_desc {
    int32_t n_towers;                    /* 1 or 2 (instrument_dual)                    */
    int32_t in_h[2], in_w[2];            /* input_shapes (bands, frames), Cin = 1        */
    int32_t kh[2], kw[2];                /* kernel_sizes                                 */
    int32_t pool_h[2], pool_w[2];        /* pool_sizes                                   */
    int32_t conv_layers;                 /* convolutional_layer_count                    */
    int32_t feature_expand_frequency;
    int32_t pool_layer_frequency;
    int32_t residual_frequency;          /* residual_layer_frequencies = [r]; 0 = none   */
    int32_t dense_units;                 /* 300                                          */
    int32_t output_classes;              /* 1 => sigmoid + range scaling; >1 => softmax  */
    float   out_lo, out_hi;              /* output_range                                 */
} amt_rdcnn_desc;

/* Weights: one host blob of f32 in the canonical order documented in
 * amt-saga_amd/amt_saga/rdcnn.py (pack_weights); n_floats is checked against
 * the descriptor.  Uploads and pre-arranges them for the MFMA kernels. */
int amt_rdcnn_create(amt_rdcnn **net, const amt_rdcnn_desc *desc,
                     const float *weights_host, size_t n_floats);
int amt_rdcnn_destroy(amt_rdcnn *net);
size_t amt_rdcnn_param_count(const amt_rdcnn_desc *desc);
/* device scratch needed for a batch of B windows */
size_t amt_rdcnn_workspace_bytes(const amt_rdcnn *net, int B);
/* x[t]: [B][in_h][in_w] f32 (NHWC with C = 1) per tower; y: [B][output_classes] f32
 * (scaled regression value or softmax probabilities); logits (optional, may be
 * NULL): [B][output_classes] pre-activation of the last Dense. */
int amt_rdcnn_forward(const amt_rdcnn *net, const float *const *x, int B,
                      float *y, float *logits, void *workspace,
                      size_t workspace_bytes, void *stream);
/* Arithmetic of the convolutions: 0 = v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate);
 * 1 = "split-bf16": every f32 operand is split exactly into three bf16 terms and the
 * six significant cross products run on v_mfma_f32_32x32x16_bf16 with f32
 * accumulation -- same accuracy class as f32 (dropped terms <= 2^-26), 2.67x fewer
 * matrix-pipe cycles.  Layers the split kernel is not built for keep mode 0. */
int amt_rdcnn_set_mode(amt_rdcnn *net, int mode);
/* FLOPs (2*MAC) of one window's forward, for roofline accounting */
double amt_rdcnn_flops_per_window(const amt_rdcnn *net);
/* Measurement hook: when enabled, every convolution launch of amt_rdcnn_forward
 * is bracketed by HIP events on the caller's stream.  amt_rdcnn_profile_read
 * waits for the recorded events and returns one row per conv layer:
 * desc[r] = {tower, layer, kh, kw, cin, cout, H, W}, ms[r] = summed kernel time,
 * windows[r] = windows processed, flops_per_window[r] = 2*H*W*kh*kw*cin*cout.
 * n_rows receives the number of layers (call with cap = 0 to size buffers). */
int amt_rdcnn_profile(amt_rdcnn *net, int enable);
int amt_rdcnn_profile_read(amt_rdcnn *net, int32_t *desc, double *ms, double *windows,
                           double *flops_per_window, int cap, int *n_rows, int reset);

/* ------------------------------------------------------------------------ *
 * RDCNN training step (replaces res_net.train / res_net.test, RDCNN.py:503-526, :559-589: Keras
 * train_on_batch / test_on_batch of the model compiled at RDCNN.py:245-254 with Adagrad and
 * mean_squared_error (one output) or sparse_categorical_crossentropy).
 * ------------------------------------------------------------------------ */
typedef struct amt_trainer amt_trainer;

/* weights_host: the canonical blob of amt_rdcnn_create (trainable tensors AND the BN moving statistics).
 * lr / epsilon <= 0 select Keras' Adagrad defaults (0.01, 1e-7).  initial_accumulator: starting value of the
 * squared-gradient accumulators -- 0 in Keras 2.2 / tf.keras 1.13, 0.1 in tf.keras >= 1.14 (the reference's
 * `keras.optimizers.Adagrad()`, RDCNN.py:246-253, pins neither version). */
int amt_trainer_create(amt_trainer **trainer, const amt_rdcnn_desc *desc, const float *weights_host,
                       size_t n_floats, float lr, float epsilon, float initial_accumulator);
int amt_trainer_destroy(amt_trainer *trainer);
/* One batch.  x[t]: device [B][in_h][in_w] per tower; y: device [B] f32 -- the class index (softmax heads)
 * or the target ALREADY scaled to the activation range (RDCNN.py:304-306, :513-514).
 * update != 0: train_on_batch -- BatchNormalization with batch statistics (moving statistics updated with
 *   momentum 0.99), backward pass, Adagrad step.
 * update == 0: test_on_batch -- inference-mode forward and the loss only.
 * loss_host (may be NULL): the batch loss; reading it synchronises the stream.
 * pred (may be NULL): device [B][output_classes], sigmoid activation / softmax probabilities. */
int amt_trainer_step(amt_trainer *trainer, const float *const *x, const float *y, int B, int update,
                     float *loss_host, float *pred, void *stream);
/* canonical blob back to the host (synchronises): current weights / the gradients of the last step
 * (zeros for the BN moving statistics) */
int amt_trainer_get_weights(amt_trainer *trainer, float *weights_host, size_t n_floats);
int amt_trainer_get_grads(amt_trainer *trainer, float *grads_host, size_t n_floats);

/* MFMA form of amt_cqt_window_max for batches of windows (np.max(mid_wf.slice_C(0, duration, n_frames, ...)),
 * training.py:271-282, with each window standing for its song): the per-block sums as one split-fp16 GEMM per window
 * against a per-bin phasor table on a bin-independent block grid (amt_cqt.hip).  Same definition, same result to the
 * 1e-4 the VALU form is held to; hop a power of two in 256..2048 and at most 544 hop-blocks per window
 * (AMT_E_UNSUPPORTED otherwise: use amt_cqt_window_max).
 *   amt_cqt_mfma_table_bytes(hop, n_bins)   bytes of the device phasor table for a bin grid
 *   amt_cqt_mfma_table(...)                 builds it (once per grid and hop)
 *   amt_cqt_window_max_mfma(...)            out_max[b] = max over bins and frames 0 .. L / hop; amax_scratch: [B] f32 */
size_t amt_cqt_mfma_table_bytes(int hop, int n_bins);
int amt_cqt_mfma_table(const uint32_t *phase_inc, const int32_t *length, int n_bins, int hop, void *table,
                       void *stream);
int amt_cqt_window_max_mfma(const float *wave, int B, int L, size_t wave_stride, int hop,
                            const uint32_t *phase_inc, const int32_t *length, const void *table, int n_bins,
                            float *out_max, float *amax_scratch, void *stream);

/* ------------------------------------------------------------------------ *
 * FFT-domain form of ONE Conv2D(32 -> 32, (4, 16), 'same') + BatchNormalization + sigmoid (+ Add + BatchNormalization)
 * layer of res_net (RDCNN.py:186-193) on an H x W image, W <= 561: the stand-alone entry the parity tests and the
 * layer microbenchmark use; inside amt_rdcnn_forward the same kernels run chained (conv mode 3).
 *   kernel_host [4][16][32][32] (kh, kw, cin, cout); s1, t1: folded BN (+ bias) [32]; s2, t2: the BN after the Add, or
 *   NULL; in / shortcut / out: device [B][H][W][32]; workspace: amt_fftconv_workspace_bytes(B, H) of device memory.
 * ------------------------------------------------------------------------ */
typedef struct amt_fftconv_layer amt_fftconv_layer;
int amt_fftconv_create(amt_fftconv_layer **layer, const float *kernel_host, const float *s1, const float *t1,
                       const float *s2, const float *t2);
int amt_fftconv_destroy(amt_fftconv_layer *layer);
size_t amt_fftconv_workspace_bytes(int B, int H);
int amt_fftconv_run(const amt_fftconv_layer *layer, const float *in, const float *shortcut, int B, int H, int W,
                    float *out, void *workspace, size_t workspace_bytes, int repeat_gemm, void *stream);

/* ------------------------------------------------------------------------ *
 * The same layer kind on the 10 x 64 images behind the first pooling of the timing classifier
 * (timing_classifier.py:13-36; Conv2D(64, (4, 16), 'same') + BatchNormalization + sigmoid (+ Add + BatchNormalization),
 * RDCNN.py:186-198) in the packed-image FFT-domain form (amt_fftpk.hip): the whole image is one 1152-point sequence per
 * channel pair, one 128 x 128 GEMM per frequency pair with the windows as rows.  Stand-alone entry for the parity tests
 * and the layer microbenchmark; inside amt_rdcnn_forward the same kernels run chained (conv mode 3).
 *   kernel_host [4][16][64][64]; s1, t1, s2, t2 [64]; in / shortcut / out: device [B][10][64][64];
 *   chain: extra applications of the layer (BN + sigmoid, no shortcut) with the hand-over in the frequency domain before the
 *   final one; repeat_gemm: the final GEMM launched that many times (timing).
 * ------------------------------------------------------------------------ */
typedef struct amt_fftpk_layer amt_fftpk_layer;
int amt_fftpk_create(amt_fftpk_layer **layer, const float *kernel_host, const float *s1, const float *t1,
                     const float *s2, const float *t2);
int amt_fftpk_destroy(amt_fftpk_layer *layer);
size_t amt_fftpk_workspace_bytes(int B);
int amt_fftpk_run(const amt_fftpk_layer *layer, const float *in, const float *shortcut, int B, float *out,
                  void *workspace, size_t workspace_bytes, int chain, int repeat_gemm, void *stream);

/* ------------------------------------------------------------------------ *
 * Measurement probe (no reference counterpart; bench.py's roofline object).  Sustained rate of back-to-back
 * v_mfma_f32_16x16x32_f16 on register operands with `waves_per_simd` waves per SIMD on every CU, `iters` x 8
 * MFMAs per wave and launch, best of `launches`; random_operands != 0: random non-zero f16 operands (the rate
 * the power limit allows on live data), 0: zeros (the cycle-limited rate).  Synchronises the stream.
 * ------------------------------------------------------------------------ */
int amt_probe_mfma_f16(int waves_per_simd, int iters, int random_operands, int launches,
                       double *tflops_best, double *ms_best, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AMT_SAGA_H */
