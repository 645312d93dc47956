// Spectrogram images on the device for gfx950: a ragged batch of magnitude spectrograms -> 8-bit level images in one
// launch, and a ragged batch of 8-bit images -> complete PNG files in one call (pieces -> sizes -> scan -> gather).
//
// Replaces the librosa.display.specshow + savefig of audio_complete.plot_spec (util_audio.py:509-518) and of plot_specs
// (util_audio.py:938-960 of the reference): the dB picture of audio_complete.D on a log or linear frequency axis, as a
// file.  The host builds the axis tables, the thresholds and the palette (amt_saga/png.py); everything per pixel and per
// byte is here.  The rule of every output byte is amt_png_core.h's.
//
// Design:
//  * levels: a 256-thread workgroup takes tiles of 64 rows x 64 columns of one image.  A wave takes a column, its lanes
//    the 64 rows: the lanes read neighbouring bins of one frame (the contiguous axis of the frame-major spectrogram),
//    take the maximum over their bins and frames and count thresholds by binary search in LDS (255 products of
//    thr[k] * ref, one __fmul_rn each, made once per workgroup).  The tile is transposed through LDS and leaves along
//    time, the contiguous axis of the image.
//  * encoder, kernel 1: one workgroup per piece (at most 32768 filtered bytes, one deflate block, one IDAT chunk).  A wave
//    filters a row: five sums of absolute residues by shuffles, the chosen filter's bytes into LDS.  Every thread then
//    owns a span of the piece and the runs that BEGIN in it (the first run start behind each span comes from a table in
//    LDS), so counting, pricing and writing the tokens are closed per thread.  Symbol counts by LDS atomics; the used
//    symbols are sorted by rank in parallel; ONE lane builds the 286-symbol code lengths and the 19-symbol code
//    (png_code_lengths, as one lane runs the Levinson recurrence of the LPC encoder).  The kind is chosen from the three
//    sizes; the bit offsets of the threads come from a block scan and every thread ORs its tokens into the chunk in LDS
//    (OR commutes: no order between writers).  CRC-32 of the chunk: every thread its span by table, joined with
//    x^(8 bytes behind it) mod the polynomial, XOR over the threads.  Adler-32: per-piece sums, joined later.
//  * kernel 2 (one workgroup): Adler-32 and the last chunk's CRC per image, file sizes, their scan, chunk offsets.
//  * kernel 3: a workgroup per chunk copies it to its place; a workgroup per image writes signature, IHDR, PLTE, IEND.
//  * integer code apart from the one multiply and the comparisons of the levels; no packed-FP32 instructions: any stream.
#include "amt_launch.h"
#include "amt_png_core.h"
#include "amt_wg.h"

#define PNG_THREADS 256
#define PNG_TILE 64                       /* rows and columns of a levels tile */
#define PNG_TILE_PITCH 68
#define PNG_LDS_CAP (72 * 1024)           /* dynamic LDS of the piece kernel: the filtered bytes and the chunk */
#define PNG_LEVELS_MAX_GRID 4096

// ---------------------------------------------------------------------------------------------------------------
// levels
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PNG_THREADS) void spec_levels_kernel(
    const float *__restrict__ mag, png_i64 mag_floats, const png_i64 *__restrict__ meta, const int *__restrict__ tables,
    png_i64 table_ints, const float *__restrict__ thr, const float *__restrict__ ref, unsigned char *__restrict__ out,
    png_i64 out_bytes) {
    __shared__ float prod[256];
    __shared__ unsigned char tile[PNG_TILE * PNG_TILE_PITCH];
    png_i64 row[PNG_LEVEL_META];
#pragma unroll
    for (int k = 0; k < PNG_LEVEL_META; ++k) row[k] = meta[(png_i64)blockIdx.y * PNG_LEVEL_META + k];
    if (!png_levels_row_ok(row, mag_floats, table_ints, out_bytes)) return;            // (whole workgroup)
    const int T = (int)row[1], F = (int)row[3], W = (int)row[4], H = (int)row[5];
    const png_i64 ldf = row[2];
    const float *m = mag + row[0];
    const int *rows = tables + row[6], *cols = tables + row[7];
    unsigned char *o = out + row[8];
    const int tx = (W + PNG_TILE - 1) / PNG_TILE, ty = (H + PNG_TILE - 1) / PNG_TILE;
    if ((int)blockIdx.x >= tx * ty) return;
    const float r = ref[blockIdx.y];
    const bool live = png_ref_ok(r);
    if (threadIdx.x < PNG_THRESHOLDS) prod[threadIdx.x] = live ? png_fmul(thr[threadIdx.x], r) : 0.f;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int t = blockIdx.x; t < tx * ty; t += gridDim.x) {
        const int j0 = (t / tx) * PNG_TILE, i0 = (t % tx) * PNG_TILE;
        const int j = j0 + lane;
        int f_lo = 0, f_hi = 0;
        if (j < H) {
            f_lo = png_clamp(rows[2 * j], 0, F);
            f_hi = png_clamp(rows[2 * j + 1], f_lo, F);
        }
        for (int ci = wave; ci < PNG_TILE; ci += PNG_THREADS / 64) {
            const int i = i0 + ci;
            if (i >= W) break;                                                        // (uniform over the wave)
            int level = 0;
            if (live && j < H) {
                const int t_lo = png_clamp(cols[2 * i], 0, T), t_hi = png_clamp(cols[2 * i + 1], t_lo, T);
                float v = 0.f;
                for (int fr = t_lo; fr < t_hi; ++fr) {
                    const float *x = m + (png_i64)fr * ldf;
                    for (int f = f_lo; f < f_hi; ++f) v = png_cell_max(v, x[f]);
                }
                level = png_level(v, prod);
            }
            tile[lane * PNG_TILE_PITCH + ci] = (unsigned char)level;
        }
        __syncthreads();
        for (int k = threadIdx.x; k < PNG_TILE * PNG_TILE; k += PNG_THREADS) {
            const int jj = k >> 6, ii = k & 63;
            if (j0 + jj < H && i0 + ii < W) o[(png_i64)(j0 + jj) * W + i0 + ii] = tile[jj * PNG_TILE_PITCH + ii];
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// encoder
// ---------------------------------------------------------------------------------------------------------------
struct png_or_lds {
    uint32_t *w;
    __device__ void operator()(uint32_t i, uint32_t v) const { if (v) atomicOr(w + i, v); }
};
typedef png_bits<png_or_lds> png_writer;

struct png_piece_lds {
    uint32_t crc_table[256];
    uint32_t freq[288];
    uint32_t weight[2 * PNG_LITLEN];
    uint16_t parent[2 * PNG_LITLEN];
    uint16_t order[288];
    uint16_t code[288];
    unsigned char len[288];
    int first_start[PNG_THREADS];
    uint32_t red[8];
    uint32_t acc[8];            // fixed bits, extra bits, matches, used symbols, byte sum, weighted sum, CRC
    png_dyn_head head;
    int kind;
    uint32_t data_bits;         // block bits, header and end-of-block included
};

// meta int64 [n][4]: first byte in pix, W, H, first piece.  pieces int64 [P][4]: image, first row, rows, slot offset.
__global__ __launch_bounds__(PNG_THREADS) void png_piece_kernel(
    const unsigned char *__restrict__ pix, const png_i64 *__restrict__ meta, const png_i64 *__restrict__ pieces,
    unsigned char *__restrict__ slots, uint32_t *__restrict__ res, int cap) {
    extern __shared__ __align__(16) unsigned char png_dyn_lds[];
    __shared__ png_piece_lds s;
    unsigned char *fb = png_dyn_lds;                                   // [cap]
    uint32_t *ow = (uint32_t *)(png_dyn_lds + cap);                    // [(cap + 16) / 4]: the chunk from its type on
    unsigned char *ob = (unsigned char *)ow;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const png_i64 p = blockIdx.x;
    const png_i64 img = pieces[4 * p], row0 = pieces[4 * p + 1], prow = pieces[4 * p + 2], slot_off = pieces[4 * p + 3];
    const int W = (int)meta[4 * img + 1], H = (int)meta[4 * img + 2];
    const unsigned char *im = pix + meta[4 * img];
    const int n = (int)prow * (W + 1);                                 // <= cap by the host's layout
    const bool first = row0 == 0, last = row0 + prow == H;

    s.crc_table[tid] = png_crc_entry((uint32_t)tid);
    for (int k = tid; k < 288; k += PNG_THREADS) { s.freq[k] = k == PNG_EOB ? 1u : 0u; s.len[k] = 0; }
    for (int k = tid; k < (cap + 16) / 4; k += PNG_THREADS) ow[k] = 0;
    if (tid < 8) s.acc[tid] = 0;

    // ---- filters: a wave per row
    for (int r = wave; r < (int)prow; r += PNG_THREADS / 64) {
        const png_i64 y = row0 + r;
        const unsigned char *cur = im + y * W, *prev = y > 0 ? cur - W : nullptr;
        uint32_t sum[5] = {0, 0, 0, 0, 0};
        for (int x = lane; x < W; x += 64) {
            const int v = cur[x], a = x ? cur[x - 1] : 0, b = prev ? prev[x] : 0, c = (prev && x) ? prev[x - 1] : 0;
#pragma unroll
            for (int f = 0; f < 5; ++f) sum[f] += (uint32_t)png_abs_signed(png_filter_byte(f, v, a, b, c));
        }
#pragma unroll
        for (int f = 0; f < 5; ++f) sum[f] = amt_wave_reduce(sum[f], amt_sum{});
        const int f = png_pick_filter(sum);
        unsigned char *dst = fb + (png_i64)r * (W + 1);
        if (lane == 0) dst[0] = (unsigned char)f;
        for (int x = lane; x < W; x += 64) {
            const int v = cur[x], a = x ? cur[x - 1] : 0, b = prev ? prev[x] : 0, c = (prev && x) ? prev[x - 1] : 0;
            dst[1 + x] = (unsigned char)png_filter_byte(f, v, a, b, c);
        }
    }
    __syncthreads();

    // ---- spans, run starts, Adler sums, symbol counts
    const int span = (n + PNG_THREADS - 1) / PNG_THREADS;
    const int c0 = tid * span < n ? tid * span : n, c1 = c0 + span < n ? c0 + span : n;
    s.first_start[tid] = png_first_start(fb, c0, c1, n);
    {
        uint32_t bs = 0, ws = 0;                                       // <= 128 x 255 and <= 128 x 255 x 32768
        for (int i = c0; i < c1; ++i) { bs += fb[i]; ws += (uint32_t)(n - i) * fb[i]; }
        if (bs) { atomicAdd(&s.acc[4], bs % PNG_ADLER_MOD); atomicAdd(&s.acc[5], ws % PNG_ADLER_MOD); }
    }
    __syncthreads();
    int next_after = n;
    for (int u = tid + 1; u < PNG_THREADS; ++u)
        if (s.first_start[u] < n) { next_after = s.first_start[u]; break; }
    png_walk_runs(fb, c0, c1, next_after, [&](int, int L, int byte) {
        png_run_count(L, byte, [&](int sym, int c) { atomicAdd(&s.freq[sym], (uint32_t)c); });
    });
    __syncthreads();

    // ---- the used symbols by rank; the sums every kind's size needs
    for (int sym = tid; sym < PNG_LITLEN; sym += PNG_THREADS) {
        const uint32_t c = s.freq[sym];
        if (!c) continue;
        const uint32_t key = png_sort_key(c, sym);
        int rank = 0;
        for (int o = 0; o < PNG_LITLEN; ++o) rank += s.freq[o] && png_sort_key(s.freq[o], o) < key;
        s.order[rank] = (uint16_t)sym;
        atomicAdd(&s.acc[0], c * (uint32_t)png_fixed_len(sym));
        if (sym > PNG_EOB) {
            atomicAdd(&s.acc[1], c * (uint32_t)((sym >= 265 && sym < 285) ? (sym - 261) / 4 : 0));
            atomicAdd(&s.acc[2], c);
        }
        atomicAdd(&s.acc[3], 1u);
    }
    __syncthreads();

    // ---- one lane: code lengths, the dynamic header, the kind  (a piece has a literal and the end of block: >= 2 used)
    if (tid == 0) {
        png_code_lengths(s.freq, s.order, (int)s.acc[3], 15, s.len, s.weight, s.parent);
        png_dynamic_head(s.len, &s.head);
        uint32_t dyn = s.head.bits + s.acc[1] + s.acc[2];
        for (int sym = 0; sym < PNG_LITLEN; ++sym) dyn += s.freq[sym] * s.len[sym];
        const uint32_t fixed = 3 + s.acc[0] + s.acc[1] + 5 * s.acc[2];
        s.kind = png_pick_kind((uint32_t)n, fixed, dyn, last);
        s.data_bits = s.kind == PNG_KIND_DYNAMIC ? dyn : fixed;
        if (s.kind == PNG_KIND_DYNAMIC) png_canonical(s.len, PNG_LITLEN, s.code);
    }
    __syncthreads();
    const int kind = s.kind;
    const int hb = 4 + (first ? 2 : 0);                                // chunk type, zlib header
    uint32_t body;                                                     // bytes of the chunk from its type to its data's end
    if (kind == PNG_KIND_STORED) {
        body = (uint32_t)(hb + 5 + n);
        for (int i = tid; i < n; i += PNG_THREADS) ob[hb + 5 + i] = fb[i];
        if (tid == 0) {
            ob[hb] = last ? 1 : 0;
            ob[hb + 1] = (unsigned char)n; ob[hb + 2] = (unsigned char)(n >> 8);
            ob[hb + 3] = (unsigned char)~n; ob[hb + 4] = (unsigned char)(~n >> 8);
        }
    } else {
        if (kind == PNG_KIND_FIXED) {
            for (int sym = tid; sym < 288; sym += PNG_THREADS) {
                s.len[sym] = (unsigned char)png_fixed_len(sym);
                s.code[sym] = (uint16_t)png_fixed_code(sym);
            }
            __syncthreads();
        }
        const int dist_bits = kind == PNG_KIND_FIXED ? 5 : 1;
        uint32_t mine = 0;
        png_walk_runs(fb, c0, c1, next_after, [&](int, int L, int byte) { mine += png_run_bits(L, byte, s.len, dist_bits); });
        uint32_t total;
        const uint32_t before = amt_block_scan<uint32_t, PNG_THREADS>(mine, s.red, &total);
        const uint32_t head_bits = kind == PNG_KIND_FIXED ? 3 : s.head.bits;
        const uint32_t tok0 = 8u * hb + head_bits;                     // total + head_bits + len[EOB] == data_bits
        png_writer w(png_or_lds{ow}, tok0 + before);
        png_walk_runs(fb, c0, c1, next_after, [&](int, int L, int byte) { png_run_emit(w, L, byte, s.code, s.len, 0, dist_bits); });
        w.flush();
        if (tid == 0) {
            png_writer h(png_or_lds{ow}, 8u * hb);
            if (kind == PNG_KIND_FIXED) h.put((uint32_t)(last ? 1 : 0) | (1u << 1), 3);
            else png_dynamic_head_emit(h, s.len, &s.head, last);
            h.flush();
            png_writer e(png_or_lds{ow}, tok0 + total);
            e.put(s.code[PNG_EOB], s.len[PNG_EOB]);
            e.flush();
        }
        body = (uint32_t)hb + png_block_bytes(s.data_bits, last);
        if (tid == 1 && !last) {                                       // the empty stored block's FF FF; its zeros are there
            atomicOr(ow + ((body - 2) >> 2), 0xFFu << (8 * ((body - 2) & 3)));
            atomicOr(ow + ((body - 1) >> 2), 0xFFu << (8 * ((body - 1) & 3)));
        }
    }
    __syncthreads();
    if (tid == 0) {
        ob[0] = 'I'; ob[1] = 'D'; ob[2] = 'A'; ob[3] = 'T';
        if (first) { ob[4] = 0x78; ob[5] = 0x01; }
    }
    __syncthreads();

    // ---- CRC-32 of the chunk so far, and the chunk to its slot
    {
        const uint32_t bspan = (body + PNG_THREADS - 1) / PNG_THREADS;
        const uint32_t b0 = tid * bspan < body ? tid * bspan : body, b1 = b0 + bspan < body ? b0 + bspan : body;
        if (b1 > b0) {
            const uint32_t c = png_crc_bytes(s.crc_table, 0, ob + b0, b1 - b0);
            atomicXor(&s.acc[6], png_gf_mul(png_x_pow_bytes(body - b1), c));
        }
    }
    unsigned char *slot = slots + slot_off;
    uint32_t *sw = (uint32_t *)(slot + 4);                             // (slot offsets are multiples of 16)
    for (uint32_t k = tid; k < (body + 3) / 4; k += PNG_THREADS) sw[k] = ow[k];
    __syncthreads();
    if (tid == 0) {
        png_put_be32(slot, body - 4 + (last ? 4 : 0));
        if (!last) png_put_be32(slot + 4 + body, s.acc[6]);
        uint32_t *r = res + PNG_RES * p;
        r[0] = body; r[1] = s.acc[6]; r[2] = s.acc[4] % PNG_ADLER_MOD; r[3] = s.acc[5] % PNG_ADLER_MOD; r[4] = (uint32_t)n;
    }
}

// One workgroup: per image the Adler-32 and the last chunk's CRC, the file size; the scan; the chunk offsets.
__global__ __launch_bounds__(PNG_THREADS) void png_scan_kernel(
    const png_i64 *__restrict__ meta, const png_i64 *__restrict__ pieces, const uint32_t *__restrict__ res,
    unsigned char *__restrict__ slots, int n, int palette, png_i64 *__restrict__ sizes, png_i64 *__restrict__ piece_off,
    png_i64 *__restrict__ file_off) {
    __shared__ png_i64 part[PNG_THREADS / 64];
    const int tid = threadIdx.x;
    const int per = (n + PNG_THREADS - 1) / PNG_THREADS;
    const int i0 = tid * per < n ? tid * per : n, i1 = i0 + per < n ? i0 + per : n;
    png_i64 mine = 0;
    for (int i = i0; i < i1; ++i) {
        const int W = (int)meta[4 * i + 1], H = (int)meta[4 * i + 2];
        const png_i64 p0 = meta[4 * i + 3], np = png_pieces(W, H);
        uint32_t a = 1, b = 0;
        png_i64 size = png_head_bytes(palette) + 12;
        for (png_i64 p = p0; p < p0 + np; ++p) {
            const uint32_t *r = res + PNG_RES * p;
            png_adler_join(&a, &b, r[2], r[3], r[4]);
            size += 8 + (png_i64)r[0] + (p == p0 + np - 1 ? 4 : 0);
        }
        const uint32_t *r = res + PNG_RES * (p0 + np - 1);
        unsigned char *tail = slots + pieces[4 * (p0 + np - 1) + 3] + 4 + r[0];
        const uint32_t adler = (b << 16) | a;
        png_put_be32(tail, adler);
        uint32_t crc = r[1];
        for (int k = 0; k < 4; ++k) crc = png_crc_byte(crc, tail[k]);
        png_put_be32(tail + 4, crc);
        sizes[i] = size;
        mine += size;
    }
    png_i64 total, off = amt_block_scan<png_i64, PNG_THREADS>(mine, part, &total);
    if (tid == 0) file_off[n] = total;
    for (int i = i0; i < i1; ++i) {
        file_off[i] = off;
        const int W = (int)meta[4 * i + 1], H = (int)meta[4 * i + 2];
        const png_i64 p0 = meta[4 * i + 3], np = png_pieces(W, H);
        png_i64 at = off + png_head_bytes(palette);
        for (png_i64 p = p0; p < p0 + np; ++p) {
            piece_off[p] = at;
            at += 8 + (png_i64)res[PNG_RES * p] + (p == p0 + np - 1 ? 4 : 0);
        }
        off += sizes[i];
    }
}

// Workgroups [0, P): a chunk to its place.  Workgroups [P, P + n): the fixed chunks of a file.
__global__ __launch_bounds__(PNG_THREADS) void png_gather_kernel(
    const png_i64 *__restrict__ meta, const png_i64 *__restrict__ pieces, const uint32_t *__restrict__ res,
    const unsigned char *__restrict__ slots, png_i64 P, const unsigned char *__restrict__ palette,
    const png_i64 *__restrict__ piece_off, const png_i64 *__restrict__ file_off, unsigned char *__restrict__ out) {
    const png_i64 b = blockIdx.x;
    if (b < P) {
        const png_i64 img = pieces[4 * b], H = meta[4 * img + 2];
        const bool last = pieces[4 * b + 1] + pieces[4 * b + 2] == H;
        const png_i64 bytes = 8 + (png_i64)res[PNG_RES * b] + (last ? 4 : 0);
        const unsigned char *src = slots + pieces[4 * b + 3];
        unsigned char *dst = out + piece_off[b];
        for (png_i64 k = threadIdx.x; k < bytes; k += PNG_THREADS) dst[k] = src[k];
        return;
    }
    if (threadIdx.x) return;
    const png_i64 i = b - P;
    png_put_head(out + file_off[i], (int)meta[4 * i + 1], (int)meta[4 * i + 2], palette);
    png_put_end(out + file_off[i + 1] - 12);
}

extern "C" {

int amt_spec_levels_ragged(const float *mag, long long mag_floats, const long long *image_meta, int n, int max_w,
                           int max_h, const int *tables, long long table_ints, const float *thr, const float *ref,
                           unsigned char *out, long long out_bytes, void *stream) {
    if (!mag || !image_meta || !tables || !thr || !ref || !out || n < 1 || n > 65535 || !png_dims_ok(max_w, max_h) ||
        mag_floats < 0 || table_ints < 0 || out_bytes < 0)
        return AMT_E_INVALID;
    long long tiles = (long long)((max_w + PNG_TILE - 1) / PNG_TILE) * ((max_h + PNG_TILE - 1) / PNG_TILE);
    if (tiles > PNG_LEVELS_MAX_GRID) tiles = PNG_LEVELS_MAX_GRID;
    const dim3 grid((unsigned)tiles, (unsigned)n);
    spec_levels_kernel<<<grid, PNG_THREADS, 0, (hipStream_t)stream>>>(mag, mag_floats, image_meta, tables, table_ints, thr,
                                                                      ref, out, out_bytes);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

long long amt_png_file_bound(int w, int h, int palette) {
    if (!png_dims_ok(w, h)) return AMT_E_INVALID;
    return png_file_bound(w, h, palette != 0);
}

long long amt_png_scratch_bytes(const long long *image_meta, int n) {
    png_layout L;
    const png_i64 need = png_make_layout(nullptr, image_meta, n, 0, &L, nullptr);
    return need < 0 ? AMT_E_INVALID : need;
}

int amt_png_encode_ragged(const unsigned char *pix, long long pix_bytes, const long long *image_meta, int n,
                          const unsigned char *palette, void *scratch, long long scratch_bytes, unsigned char *out,
                          long long out_bytes, long long *file_off, void *stream) {
    if (!pix || !scratch || ((uintptr_t)scratch & 15) || !out || !file_off || pix_bytes < 0) return AMT_E_INVALID;
    png_layout L;
    std::vector<png_i64> tables;
    const png_i64 need = png_make_layout(scratch, image_meta, n, palette != nullptr, &L, &tables);
    if (need < 0) return AMT_E_INVALID;
    for (int i = 0; i < n; ++i) {
        const png_i64 bytes = image_meta[3 * i + 1] * image_meta[3 * i + 2];
        if (bytes > pix_bytes || image_meta[3 * i] > pix_bytes - bytes) return AMT_E_INVALID;
    }
    if (scratch_bytes < need || out_bytes < L.out_bound) return AMT_E_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    // the two small tables, the one upload of the call: it is waited for, since `tables` ends with this function
    AMT_HIP_CHECK(hipMemcpyAsync(L.meta, tables.data(), tables.size() * sizeof(png_i64), hipMemcpyHostToDevice, st));
    AMT_HIP_CHECK(hipStreamSynchronize(st));
    const size_t lds = (size_t)L.cap + (size_t)L.cap + 16;
    int rc = amt_launch<png_piece_kernel>(PNG_LDS_CAP, dim3((unsigned)L.P), dim3(PNG_THREADS), lds, st, pix, L.meta,
                                          L.pieces, L.slots, L.res, L.cap);
    if (rc != AMT_OK) return rc;
    png_scan_kernel<<<1, PNG_THREADS, 0, st>>>(L.meta, L.pieces, L.res, L.slots, n, palette != nullptr, L.sizes,
                                               L.piece_off, file_off);
    AMT_LAUNCH_CHECK();
    png_gather_kernel<<<(unsigned)(L.P + n), PNG_THREADS, 0, st>>>(L.meta, L.pieces, L.res, L.slots, L.P, palette,
                                                                   L.piece_off, file_off, out);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

}  // extern "C"
