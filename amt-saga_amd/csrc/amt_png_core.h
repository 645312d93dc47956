// Spectrogram level images and PNG files: the rule of both, plain C++ behind one macro, so the same functions compile
// into the kernels of amt_png.hip and into a stand-alone CPU program (tests/png_host_main.cpp, built with the address
// and undefined-behaviour sanitizers).  Restated independently in tests/png_reference.py.  They stand where the
// reference draws audio_complete.D with librosa.display.specshow and saves the figure (plot_spec, util_audio.py:509-518;
// plot_specs, util_audio.py:938-960).  DESIGN.md 26.
//
// LEVELS.  thr[k - 1], k = 1 .. 255: float32 of 10^(-(top_db / 20)(1 - (k - 0.5) / 255)), ascending (the host builds
// them).  A cell's value v: the float32 maximum of the magnitudes it covers, starting from 0, NaN skipped.  Its level:
// the number of k with v >= thr[k - 1] * ref, one float32 product rounded to nearest; the products ascend with k, so the
// count is a binary search.  A ref that is not finite or below 2^-100 (negative included): level 0 everywhere, which keeps
// every product a normal number.
//
// PNG.  Signature, IHDR (8 bits; colour type 3 with a 256-entry PLTE, or 0), IDAT chunks, IEND.
//   filters   every scanline takes the filter 0 .. 4 (None, Sub, Up, Average, Paeth) with the smallest sum over its bytes
//             of |residue as a signed byte|; ties: the lower number.  The row above the first counts as zeros.
//   pieces    the filtered bytes (H rows of 1 + W) are cut into pieces of R = max(1, 32768 / (W + 1)) whole rows; piece p
//             is ONE deflate block in its own IDAT chunk.  The first chunk begins with the zlib header 78 01; the last
//             block has BFINAL set and its chunk ends with the Adler-32 of all filtered bytes, combined from per-piece
//             (sum of bytes, position-weighted sum, length) mod 65521.  A block that is not the last and not stored is
//             followed by an empty stored block (00 00 00 FF FF after the padding), so every piece ends on a byte.
//   tokens    literals and matches of distance 1.  In a maximal run of L equal bytes (runs end at the piece's end): the
//             first byte is a literal; of the other m = L - 1, m / 258 matches of length 258, then m % 258 as one match
//             if it is >= 3, else as literals.  Closed per run: no serial parse.
//   kind      the smallest piece in bytes among stored (5 + n), fixed Huffman and dynamic Huffman; ties in that order.
//   dynamic   literal/length code lengths limited to 15, code-length code lengths to 7, by png_code_lengths below
//             (Huffman's algorithm on the sorted counts, then a Kraft-sum repair).  HLIT = 257 + the last used length
//             symbol; HDIST = 1, the one distance code sent with length 1 whether or not a match uses it.  The HLIT + 1
//             lengths are one sequence for the repeat codes: a run of z zeros takes 18 (up to 138) while z >= 11, then
//             17 if z >= 3, else zeros; a run of r equal non-zero lengths takes the length once, then 16 (up to 6) while
//             at least 3 remain, then the length itself.  HCLEN drops trailing zeros of the transmitted order, at least 4.
//
// Safety: every function works on the arrays it is handed with the counts it is handed; the callers (the kernels, the
// host program) size them from PNG_MAX_DIM and PNG_PIECE_BYTES.  png_levels_row_ok decides from a table row and the
// buffer sizes alone whether an image may be touched at all.
#ifndef AMT_PNG_CORE_H
#define AMT_PNG_CORE_H
#include <stdint.h>
#include <vector>
#include "amt_scratch.h"

#ifdef __HIP__
#define AMT_PNG_HD __host__ __device__ inline
#else
#define AMT_PNG_HD inline
#endif

#define PNG_MAX_DIM 16384
#define PNG_PIECE_BYTES 32768        /* a piece holds max(1, PNG_PIECE_BYTES / (W + 1)) rows: at most this many bytes */
#define PNG_THRESHOLDS 255
#define PNG_LEVEL_META 10            /* int64 per row of amt_spec_levels_ragged's table */
#define PNG_KIND_STORED 0
#define PNG_KIND_FIXED 1
#define PNG_KIND_DYNAMIC 2
#define PNG_LITLEN 286
#define PNG_EOB 256
#define PNG_CLSYMS 19
#define PNG_ADLER_MOD 65521u
#define PNG_CRC_POLY 0xEDB88320u
#define PNG_PLTE_BYTES 768

typedef long long png_i64;

// ---------------------------------------------------------------------------------------------------------------
// levels
// ---------------------------------------------------------------------------------------------------------------
AMT_PNG_HD uint32_t png_float_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }

// finite and >= 2^-100 (the sign bit makes the pattern larger than any finite one)
AMT_PNG_HD int png_ref_ok(float ref) {
    const uint32_t u = png_float_bits(ref);
    return u >= 0x0D800000u && u < 0x7F800000u;
}

AMT_PNG_HD float png_fmul(float a, float b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __fmul_rn(a, b);
#else
    volatile float p = a * b;                                         // one rounding: no excess precision, no fusing
    return p;
#endif
}

AMT_PNG_HD float png_cell_max(float v, float x) { return x > v ? x : v; }          // NaN compares false: skipped

// the number of products (ascending) that v reaches
AMT_PNG_HD int png_level(float v, const float *prod) {
    int lo = 0, hi = PNG_THRESHOLDS;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v >= prod[mid]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// row: mag_base, T, ldf, F, W, H, row table, column table, out base, reserved.  1 if every region of the image lies
// inside its buffer, with divisions and bounded factors, never a product that could overflow.
AMT_PNG_HD int png_levels_row_ok(const png_i64 *row, png_i64 mag_floats, png_i64 table_ints, png_i64 out_bytes) {
    const png_i64 mb = row[0], T = row[1], ldf = row[2], F = row[3], W = row[4], H = row[5], ro = row[6], co = row[7],
                  ob = row[8], big = (png_i64)1 << 30;
    if (T < 1 || T > big || F < 1 || ldf < F || ldf > big || W < 1 || W > PNG_MAX_DIM || H < 1 || H > PNG_MAX_DIM) return 0;
    if (mb < 0 || mag_floats < F || mb > mag_floats - F) return 0;
    if ((T - 1) > (mag_floats - F - mb) / ldf) return 0;                        // mb + (T - 1) ldf + F <= mag_floats
    if (ro < 0 || table_ints < 2 * H || ro > table_ints - 2 * H) return 0;
    if (co < 0 || table_ints < 2 * W || co > table_ints - 2 * W) return 0;
    if (ob < 0 || out_bytes < W * H || ob > out_bytes - W * H) return 0;
    return 1;
}

AMT_PNG_HD int png_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---------------------------------------------------------------------------------------------------------------
// geometry of a file
// ---------------------------------------------------------------------------------------------------------------
AMT_PNG_HD int png_dims_ok(png_i64 w, png_i64 h) { return w >= 1 && w <= PNG_MAX_DIM && h >= 1 && h <= PNG_MAX_DIM; }
AMT_PNG_HD int png_piece_rows(int w) { const int r = PNG_PIECE_BYTES / (w + 1); return r < 1 ? 1 : r; }
AMT_PNG_HD int png_pieces(int w, int h) { const int r = png_piece_rows(w); return (h + r - 1) / r; }
// the most bytes a piece's IDAT chunk takes: length, type, zlib header, stored block, Adler-32, CRC
AMT_PNG_HD png_i64 png_chunk_bound(png_i64 n) { return 4 + 4 + 2 + 5 + n + 4 + 4; }
AMT_PNG_HD png_i64 png_head_bytes(int palette) { return 8 + 25 + (palette ? 12 + PNG_PLTE_BYTES : 0); }
AMT_PNG_HD png_i64 png_file_bound(int w, int h, int palette) {
    const png_i64 r = png_piece_rows(w), full = h / r, rest = h % r;
    return png_head_bytes(palette) + full * png_chunk_bound(r * (w + 1)) + (rest ? png_chunk_bound(rest * (w + 1)) : 0) + 12;
}

// ---------------------------------------------------------------------------------------------------------------
// filters
// ---------------------------------------------------------------------------------------------------------------
AMT_PNG_HD int png_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// x the byte, a the one to its left, b the one above, c above-left (0 outside the image)
AMT_PNG_HD int png_filter_byte(int f, int x, int a, int b, int c) {
    int pred = 0;
    if (f == 1) pred = a;
    else if (f == 2) pred = b;
    else if (f == 3) pred = (a + b) >> 1;
    else if (f == 4) pred = png_paeth(a, b, c);
    return (x - pred) & 255;
}
AMT_PNG_HD int png_abs_signed(int r) { return r < 128 ? r : 256 - r; }
// the filter of a row from its five sums
AMT_PNG_HD int png_pick_filter(const uint32_t *sum) {
    int best = 0;
    for (int f = 1; f < 5; ++f)
        if (sum[f] < sum[best]) best = f;
    return best;
}

// ---------------------------------------------------------------------------------------------------------------
// checksums
// ---------------------------------------------------------------------------------------------------------------
AMT_PNG_HD uint32_t png_crc_entry(uint32_t i) {
    for (int k = 0; k < 8; ++k) i = (i >> 1) ^ ((i & 1u) ? PNG_CRC_POLY : 0u);
    return i;
}
// the CRC-32 of bytes appended to a message whose CRC-32 is crc (0 for the empty message), by table or bit by bit
AMT_PNG_HD uint32_t png_crc_bytes(const uint32_t *table, uint32_t crc, const unsigned char *p, png_i64 n) {
    crc = ~crc;
    for (png_i64 i = 0; i < n; ++i) crc = (crc >> 8) ^ table[(crc ^ p[i]) & 255u];
    return ~crc;
}
AMT_PNG_HD uint32_t png_crc_byte(uint32_t crc, uint32_t byte) {
    crc = ~crc ^ byte;
    for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ ((crc & 1u) ? PNG_CRC_POLY : 0u);
    return ~crc;
}
// a b mod the CRC polynomial; bit 31 is the coefficient of x^0
AMT_PNG_HD uint32_t png_gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & 0x80000000u) p ^= b;
        a <<= 1;
        b = (b >> 1) ^ ((b & 1u) ? PNG_CRC_POLY : 0u);
    }
    return p;
}
// x^(8 n) mod the polynomial: crc(A B) = png_gf_mul(png_x_pow_bytes(|B|), crc(A)) ^ crc(B)
AMT_PNG_HD uint32_t png_x_pow_bytes(png_i64 n) {
    uint32_t r = 0x80000000u, base = 0x00800000u;                     // 1 and x^8
    while (n > 0) {
        if (n & 1) r = png_gf_mul(r, base);
        base = png_gf_mul(base, base);
        n >>= 1;
    }
    return r;
}
AMT_PNG_HD uint32_t png_crc_join(uint32_t crc_a, uint32_t crc_b, png_i64 len_b) {
    return png_gf_mul(png_x_pow_bytes(len_b), crc_a) ^ crc_b;
}
// Adler-32 of pieces in order: (a, b) starts at (1, 0); a piece adds its byte sum s, its weighted sum w = sum of
// (n - i) d[i], and n times the a before it
AMT_PNG_HD void png_adler_join(uint32_t *a, uint32_t *b, uint32_t s, uint32_t w, uint32_t n) {
    *b = (uint32_t)(((uint64_t)*b + (uint64_t)n * *a + w) % PNG_ADLER_MOD);
    *a = (*a + s) % PNG_ADLER_MOD;
}

AMT_PNG_HD void png_put_be32(unsigned char *p, uint32_t v) {
    p[0] = (unsigned char)(v >> 24); p[1] = (unsigned char)(v >> 16); p[2] = (unsigned char)(v >> 8); p[3] = (unsigned char)v;
}
// a whole small chunk at p: length, type, data, CRC; returns its bytes
AMT_PNG_HD int png_put_chunk(unsigned char *p, const char *type, const unsigned char *data, int n) {
    png_put_be32(p, (uint32_t)n);
    uint32_t crc = 0;
    for (int i = 0; i < 4; ++i) { p[4 + i] = (unsigned char)type[i]; crc = png_crc_byte(crc, (unsigned char)type[i]); }
    for (int i = 0; i < n; ++i) { p[8 + i] = data[i]; crc = png_crc_byte(crc, data[i]); }
    png_put_be32(p + 8 + n, crc);
    return 12 + n;
}
// signature, IHDR and, with a palette, PLTE: png_head_bytes(palette != 0) bytes
AMT_PNG_HD int png_put_head(unsigned char *p, int w, int h, const unsigned char *palette) {
    const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    for (int i = 0; i < 8; ++i) p[i] = sig[i];
    unsigned char hd[13];
    png_put_be32(hd, (uint32_t)w);
    png_put_be32(hd + 4, (uint32_t)h);
    hd[8] = 8; hd[9] = palette ? 3 : 0; hd[10] = 0; hd[11] = 0; hd[12] = 0;
    int at = 8 + png_put_chunk(p + 8, "IHDR", hd, 13);
    if (palette) at += png_put_chunk(p + at, "PLTE", palette, PNG_PLTE_BYTES);
    return at;
}
AMT_PNG_HD int png_put_end(unsigned char *p) { return png_put_chunk(p, "IEND", p, 0); }

// ---------------------------------------------------------------------------------------------------------------
// tokens
// ---------------------------------------------------------------------------------------------------------------
// match length 3 .. 258 -> its length symbol; the number of extra bits; their value
AMT_PNG_HD int png_len_extra_bits(int len) {
    if (len < 11 || len == 258) return 0;
    const int l = len - 3;
    return 29 - __builtin_clz((unsigned)l);                          // floor(log2 l) - 2
}
AMT_PNG_HD int png_len_symbol(int len) {
    if (len < 11) return 257 + len - 3;
    if (len == 258) return 285;
    const int l = len - 3, e = png_len_extra_bits(len);
    return 261 + 4 * e + ((l >> e) & 3);
}
AMT_PNG_HD int png_len_extra_value(int len) { return (len - 3) & ((1 << png_len_extra_bits(len)) - 1); }

// a run of L equal bytes: literals it costs, whole 258-matches, and the last match (0: none)
AMT_PNG_HD void png_run_split(int L, int *lits, int *full, int *tail) {
    const int m = L - 1, rem = m % 258;
    *full = m / 258;
    *tail = rem >= 3 ? rem : 0;
    *lits = 1 + (rem >= 3 ? 0 : rem);
}

// The maximal runs that BEGIN in [c0, c1) of the piece fb[0 .. n): f(first, L, byte) for each, in order.  A run that
// passes c1 ends at next_after: the first run start at or after c1 (n if there is none).
template <class F>
AMT_PNG_HD void png_walk_runs(const unsigned char *fb, int c0, int c1, int next_after, F &&f) {
    int i = c0;
    if (i > 0)
        while (i < c1 && fb[i] == fb[i - 1]) ++i;
    while (i < c1) {
        const unsigned char v = fb[i];
        int e = i + 1;
        while (e < c1 && fb[e] == v) ++e;
        if (e == c1) e = next_after;
        f(i, e - i, (int)v);
        i = e;
    }
}
// the first run start in [c0, c1), or n
AMT_PNG_HD int png_first_start(const unsigned char *fb, int c0, int c1, int n) {
    for (int i = c0; i < c1; ++i)
        if (i == 0 || fb[i] != fb[i - 1]) return i;
    return n;
}

// what a run adds to the symbol counts (the caller owns the way of adding: atomics on the device)
template <class ADD>
AMT_PNG_HD void png_run_count(int L, int byte, ADD &&add) {
    int lits, full, tail;
    png_run_split(L, &lits, &full, &tail);
    add(byte, lits);
    if (full) add(285, full);
    if (tail) add(png_len_symbol(tail), 1);
}
// bits of a run under code lengths len[], a match's distance costing dist_bits
AMT_PNG_HD uint32_t png_run_bits(int L, int byte, const unsigned char *len, int dist_bits) {
    int lits, full, tail;
    png_run_split(L, &lits, &full, &tail);
    uint32_t b = (uint32_t)lits * len[byte] + (uint32_t)full * (len[285] + dist_bits);
    if (tail) b += len[png_len_symbol(tail)] + png_len_extra_bits(tail) + dist_bits;
    return b;
}

// ---------------------------------------------------------------------------------------------------------------
// Huffman codes
// ---------------------------------------------------------------------------------------------------------------
AMT_PNG_HD int png_fixed_len(int s) { return s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8)); }

// The sort key of a used symbol: ascending by (count, symbol).  Counts stay below 2^22 (a piece has at most 2^15 bytes).
AMT_PNG_HD uint32_t png_sort_key(uint32_t count, int sym) { return (count << 9) | (uint32_t)sym; }

// Fewer than two used symbols: the lowest-numbered unused ones count once, so that every code is complete.
AMT_PNG_HD void png_pad_counts(uint32_t *freq, int nsym) {
    int used = 0;
    for (int s = 0; s < nsym; ++s) used += freq[s] != 0;
    for (int s = 0; s < nsym && used < 2; ++s)
        if (freq[s] == 0) { freq[s] = 1; ++used; }
}

// THE code-length rule.  order[0 .. m): the used symbols ascending by png_sort_key, m >= 2.  Huffman's algorithm with
// two queues (of two equal weights the leaf goes first); a leaf deeper than `limit` counts as `limit`; then, while the
// Kraft sum exceeds 1: one code of length `limit` is dropped from the count and the longest shorter code becomes two
// codes one bit longer (each pass lowers the sum by 2^-limit).  The counts per length are handed out from the most
// frequent symbol down (of equal counts the larger symbol first): shortest codes first.  len[] is written for the used
// symbols only.  weight: 2 m words, parent: 2 m halfwords of workspace.
AMT_PNG_HD void png_code_lengths(const uint32_t *freq, const uint16_t *order, int m, int limit, unsigned char *len,
                                 uint32_t *weight, uint16_t *parent) {
    for (int i = 0; i < m; ++i) weight[i] = freq[order[i]];
    int leaf = 0, inner = m, nodes = m;
    while (nodes < 2 * m - 1) {
        int pick[2];
        for (int k = 0; k < 2; ++k) {
            if (leaf < m && (inner >= nodes || weight[leaf] <= weight[inner])) pick[k] = leaf++;
            else pick[k] = inner++;
        }
        weight[nodes] = weight[pick[0]] + weight[pick[1]];
        parent[pick[0]] = parent[pick[1]] = (uint16_t)nodes;
        ++nodes;
    }
    weight[2 * m - 2] = 0;                                           // from here on: depths
    for (int i = 2 * m - 3; i >= 0; --i) weight[i] = weight[parent[i]] + 1;
    uint32_t count[16];
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int i = 0; i < m; ++i) count[weight[i] < (uint32_t)limit ? weight[i] : (uint32_t)limit]++;
    uint32_t total = 0;
    for (int l = 1; l <= limit; ++l) total += count[l] << (limit - l);
    while (total > (1u << limit)) {
        count[limit]--;
        for (int l = limit - 1; l > 0; --l)
            if (count[l]) { count[l]--; count[l + 1] += 2; break; }
        --total;
    }
    int j = m;
    for (int l = 1; l <= limit; ++l)
        for (uint32_t c = 0; c < count[l]; ++c) len[order[--j]] = (unsigned char)l;
}

// the same from the counts alone (the serial sort of the host program and of the 19-symbol code): pads, sorts, builds.
// order: nsym halfwords of workspace.  len[] is zeroed first.
AMT_PNG_HD void png_code_lengths_of(uint32_t *freq, int nsym, int limit, unsigned char *len, uint16_t *order,
                                    uint32_t *weight, uint16_t *parent) {
    png_pad_counts(freq, nsym);
    int m = 0;
    for (int s = 0; s < nsym; ++s) {
        len[s] = 0;
        if (!freq[s]) continue;
        int i = m++;
        while (i > 0 && png_sort_key(freq[order[i - 1]], order[i - 1]) > png_sort_key(freq[s], s)) { order[i] = order[i - 1]; --i; }
        order[i] = (uint16_t)s;
    }
    png_code_lengths(freq, order, m, limit, len, weight, parent);
}

// canonical codes of len[0 .. nsym), already bit-reversed for the stream (deflate packs a code from its top bit)
AMT_PNG_HD void png_canonical(const unsigned char *len, int nsym, uint16_t *code) {
    uint32_t count[16], next[16];
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int s = 0; s < nsym; ++s) count[len[s]]++;
    count[0] = 0;
    uint32_t c = 0;
    for (int l = 1; l < 16; ++l) { c = (c + count[l - 1]) << 1; next[l] = c; }
    for (int s = 0; s < nsym; ++s) {
        const int l = len[s];
        uint32_t v = l ? next[l]++ : 0, r = 0;
        for (int k = 0; k < l; ++k) { r = (r << 1) | (v & 1u); v >>= 1; }
        code[s] = (uint16_t)r;
    }
}
AMT_PNG_HD uint32_t png_fixed_code(int s) {                          // bit-reversed, png_fixed_len(s) bits
    const int l = png_fixed_len(s);
    uint32_t v = s < 144 ? 0x30 + s : (s < 256 ? 0x190 + s - 144 : (s < 280 ? s - 256 : 0xC0 + s - 280)), r = 0;
    for (int k = 0; k < l; ++k) { r = (r << 1) | (v & 1u); v >>= 1; }
    return r;
}

// HLIT's count: 257 or one past the last used length symbol
AMT_PNG_HD int png_hlit(const unsigned char *len) {
    int n = PNG_LITLEN;
    while (n > 257 && len[n - 1] == 0) --n;
    return n;
}
// The code-length tokens of the sequence len[0 .. hlit) followed by the distance code's 1: f(symbol, extra bits, value).
template <class F>
AMT_PNG_HD void png_cl_tokens(const unsigned char *len, int hlit, F &&f) {
    int i = 0;
    const int n = hlit + 1;
    while (i < n) {
        const int v = i < hlit ? len[i] : 1;
        int e = i + 1;
        while (e < n && (e < hlit ? len[e] : 1) == v) ++e;
        int r = e - i;
        if (v == 0) {
            while (r >= 11) { const int t = r < 138 ? r : 138; f(18, 7, t - 11); r -= t; }
            if (r >= 3) { f(17, 3, r - 3); r = 0; }
            while (r-- > 0) f(0, 0, 0);
        } else {
            f(v, 0, 0);
            --r;
            while (r >= 3) { const int t = r < 6 ? r : 6; f(16, 2, t - 3); r -= t; }
            while (r-- > 0) f(v, 0, 0);
        }
        i = e;
    }
}
AMT_PNG_HD int png_cl_order(int k) {
    const unsigned char o[PNG_CLSYMS] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return o[k];
}
AMT_PNG_HD int png_hclen(const unsigned char *cl_len) {
    int n = PNG_CLSYMS;
    while (n > 4 && cl_len[png_cl_order(n - 1)] == 0) --n;
    return n;
}

// A dynamic block's tables from the literal/length code lengths: the code-length code, HLIT, HCLEN and the bits of the
// header (the 3 block bits included).  ws: PNG_CLSYMS halfwords + 2 PNG_CLSYMS words + 2 PNG_CLSYMS halfwords.
struct png_dyn_head { unsigned char cl_len[PNG_CLSYMS]; uint16_t cl_code[PNG_CLSYMS]; int hlit, hclen; uint32_t bits; };
AMT_PNG_HD void png_dynamic_head(const unsigned char *len, png_dyn_head *h) {
    uint32_t freq[PNG_CLSYMS], weight[2 * PNG_CLSYMS];
    uint16_t order[PNG_CLSYMS], parent[2 * PNG_CLSYMS];
    for (int s = 0; s < PNG_CLSYMS; ++s) freq[s] = 0;
    h->hlit = png_hlit(len);
    png_cl_tokens(len, h->hlit, [&](int s, int, int) { freq[s]++; });
    png_code_lengths_of(freq, PNG_CLSYMS, 7, h->cl_len, order, weight, parent);
    png_canonical(h->cl_len, PNG_CLSYMS, h->cl_code);
    h->hclen = png_hclen(h->cl_len);
    uint32_t bits = 3 + 5 + 5 + 4 + 3 * (uint32_t)h->hclen;
    const unsigned char *cl = h->cl_len;
    png_cl_tokens(len, h->hlit, [&](int s, int eb, int) { bits += cl[s] + eb; });
    h->bits = bits;
}

// bytes of a piece whose block takes `bits` bits (3 block bits included): padded, and followed by the empty stored
// block unless it is the last
AMT_PNG_HD uint32_t png_block_bytes(uint32_t bits, int last) { return last ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4; }
AMT_PNG_HD int png_pick_kind(uint32_t n, uint32_t fixed_bits, uint32_t dyn_bits, int last) {
    const uint32_t st = 5 + n, fx = png_block_bytes(fixed_bits, last), dy = png_block_bytes(dyn_bits, last);
    int kind = PNG_KIND_STORED;
    uint32_t best = st;
    if (fx < best) { best = fx; kind = PNG_KIND_FIXED; }
    if (dy < best) { best = dy; kind = PNG_KIND_DYNAMIC; }
    return kind;
}

// ---------------------------------------------------------------------------------------------------------------
// the bit stream: least significant bit first, into 32-bit words that several writers may share; OR is the store
// (plain on the host, atomic on the device).  The words are zero before the first put.
// ---------------------------------------------------------------------------------------------------------------
template <class OR32>
struct png_bits {
    OR32 or32;
    uint64_t acc;
    uint32_t fill, word;
    AMT_PNG_HD png_bits(OR32 o, uint32_t bit_pos) : or32(o), acc(0), fill(bit_pos & 31u), word(bit_pos >> 5) {}
    AMT_PNG_HD void put(uint32_t value, int nbits) {                  // nbits <= 25
        acc |= (uint64_t)value << fill;
        fill += (uint32_t)nbits;
        if (fill >= 32) { or32(word++, (uint32_t)acc); acc >>= 32; fill -= 32; }
    }
    AMT_PNG_HD void flush() {
        if (fill) or32(word, (uint32_t)acc);
        acc = 0; fill = 0;
    }
};

// the tokens of one run
template <class B>
AMT_PNG_HD void png_run_emit(B &w, int L, int byte, const uint16_t *code, const unsigned char *len, uint32_t dist_code,
                             int dist_bits) {
    int lits, full, tail;
    png_run_split(L, &lits, &full, &tail);
    w.put(code[byte], len[byte]);
    for (int k = 0; k < full; ++k) { w.put(code[285], len[285]); w.put(dist_code, dist_bits); }
    if (tail) {
        const int s = png_len_symbol(tail), eb = png_len_extra_bits(tail);
        w.put(code[s] | ((uint32_t)png_len_extra_value(tail) << len[s]), len[s] + eb);
        w.put(dist_code, dist_bits);
    } else {
        for (int k = 1; k < lits; ++k) w.put(code[byte], len[byte]);
    }
}

// the header of a dynamic block: block bits, HLIT, HDIST, HCLEN, the code-length code, the lengths
template <class B>
AMT_PNG_HD void png_dynamic_head_emit(B &w, const unsigned char *len, const png_dyn_head *h, int last) {
    w.put((uint32_t)(last ? 1 : 0) | (2u << 1), 3);
    w.put((uint32_t)(h->hlit - 257), 5);
    w.put(0, 5);
    w.put((uint32_t)(h->hclen - 4), 4);
    for (int k = 0; k < h->hclen; ++k) w.put(h->cl_len[png_cl_order(k)], 3);
    png_cl_tokens(len, h->hlit, [&](int s, int eb, int v) {
        w.put(h->cl_code[s] | ((uint32_t)v << h->cl_len[s]), h->cl_len[s] + eb);
    });
}

#define PNG_RES 8                    /* uint32 per piece result: body bytes, CRC, byte sum, weighted sum, bytes */

// The scratch of one amt_png_encode_ragged call, from the host's table [n][3] = first byte, W, H: the two tables the call
// uploads back to back (meta int64 [n][4], pieces int64 [P][4]: tables->data(), if asked for), then every region on a
// 16-byte boundary.  Returns the bytes of the scratch, -1 if the table is refused.
struct png_layout {
    png_i64 P, out_bound;
    int cap;                                                           // LDS bytes of the longest piece, 16-aligned
    png_i64 *meta, *pieces;                                            // [n][4], [P][4]
    uint32_t *res;                                                     // [P][PNG_RES]
    png_i64 *sizes, *piece_off;                                        // [n], [P]
    unsigned char *slots;
    png_i64 slot_bytes;
};
inline png_i64 png_make_layout(void *scratch, const long long *image_meta, int n, int palette, png_layout *L,
                               std::vector<png_i64> *tables) {
    if (!image_meta || n < 1 || n > 65535) return -1;
    png_i64 P = 0, slot = 0, bound = 0;
    int cap = 0;
    if (tables) tables->assign((size_t)4 * n, 0);
    for (int i = 0; i < n; ++i) {
        const png_i64 base = image_meta[3 * i], w = image_meta[3 * i + 1], h = image_meta[3 * i + 2];
        if (!png_dims_ok(w, h) || base < 0) return -1;
        const int r = png_piece_rows((int)w);
        if (tables) {
            png_i64 *m = tables->data() + 4 * i;
            m[0] = base; m[1] = w; m[2] = h; m[3] = P;
        }
        for (png_i64 y = 0; y < h; y += r) {
            const png_i64 rows = h - y < r ? h - y : r, bytes = rows * (w + 1);
            if (bytes > cap) cap = (int)bytes;
            if (tables) {
                const png_i64 row[4] = {i, y, rows, slot};
                tables->insert(tables->end(), row, row + 4);
            }
            slot += (png_chunk_bound(bytes) + 4 + 15) / 16 * 16;       // (+ 4: the chunk is copied in whole words)
            ++P;
        }
        bound += png_file_bound((int)w, (int)h, palette);
    }
    amt_carver c(scratch);
    L->P = P;
    L->out_bound = bound;
    L->cap = (cap + 15) / 16 * 16;
    L->meta = c.take<png_i64>(4 * (png_i64)n, 16);
    L->pieces = c.take<png_i64>(4 * P);
    L->res = c.take<uint32_t>(PNG_RES * P, 16);
    L->sizes = c.take<png_i64>(n, 16);
    L->piece_off = c.take<png_i64>(P, 16);
    L->slots = c.take<unsigned char>(slot, 16);
    L->slot_bytes = slot;
    return c.failed ? -1 : c.at;
}

#endif
