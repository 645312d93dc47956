// csrc/amt_png_core.h on the host alone: a serial PNG writer and the level rule put together from the functions the
// kernels of amt_png.hip compile, run over a case file (tests/test_png_cpu.py writes it) in buffers of exactly the
// stated sizes, so that the address and undefined-behaviour sanitizers see any step outside them.
//
//   case file: "PNGC", int32 cases; per case int32 type
//     0 (encode): int32 W, H, palette; [768 bytes]; W H pixel bytes; int64 n; n expected file bytes
//     1 (levels): int32 T, ldf, F, W, H; uint32 ref bits; 255 float32 thresholds; T ldf float32; 2 H + 2 W int32
//                 (row table, column table); W H expected bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "amt_png_core.h"

struct or_host {
    uint32_t *w;
    void operator()(uint32_t i, uint32_t v) const { w[i] |= v; }
};
typedef png_bits<or_host> writer;

static std::vector<unsigned char> encode(const unsigned char *pix, int W, int H, const unsigned char *palette) {
    std::vector<unsigned char> out((size_t)png_file_bound(W, H, palette != nullptr));
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; ++i) table[i] = png_crc_entry(i);
    size_t at = (size_t)png_put_head(out.data(), W, H, palette);
    const int R = png_piece_rows(W);
    uint32_t ad_a = 1, ad_b = 0;
    for (int y0 = 0; y0 < H; y0 += R) {
        const int rows = H - y0 < R ? H - y0 : R, n = rows * (W + 1);
        const bool first = y0 == 0, last = y0 + rows == H;
        std::vector<unsigned char> fb((size_t)n);
        for (int r = 0; r < rows; ++r) {
            const unsigned char *cur = pix + (size_t)(y0 + r) * W, *prev = y0 + r > 0 ? cur - W : nullptr;
            uint32_t sum[5] = {0, 0, 0, 0, 0};
            for (int f = 0; f < 5; ++f)
                for (int x = 0; x < W; ++x)
                    sum[f] += (uint32_t)png_abs_signed(png_filter_byte(f, cur[x], x ? cur[x - 1] : 0, prev ? prev[x] : 0,
                                                                       (prev && x) ? prev[x - 1] : 0));
            const int f = png_pick_filter(sum);
            unsigned char *dst = fb.data() + (size_t)r * (W + 1);
            dst[0] = (unsigned char)f;
            for (int x = 0; x < W; ++x)
                dst[1 + x] = (unsigned char)png_filter_byte(f, cur[x], x ? cur[x - 1] : 0, prev ? prev[x] : 0,
                                                            (prev && x) ? prev[x - 1] : 0);
        }
        uint64_t bs = 0, ws = 0;
        for (int i = 0; i < n; ++i) { bs += fb[i]; ws += (uint64_t)(n - i) * fb[i]; }
        png_adler_join(&ad_a, &ad_b, (uint32_t)(bs % PNG_ADLER_MOD), (uint32_t)(ws % PNG_ADLER_MOD), (uint32_t)n);
        // the runs in three spans with their own tables of starts, as the threads of the kernel take them
        const int cut[4] = {0, n / 3, n / 3 + (n - n / 3) / 2, n};
        int next_after[3];
        for (int k = 0; k < 3; ++k) {
            next_after[k] = n;
            for (int u = k + 1; u < 3 && next_after[k] == n; ++u) next_after[k] = png_first_start(fb.data(), cut[u], cut[u + 1], n);
        }
        uint32_t freq[288];
        for (int s = 0; s < 288; ++s) freq[s] = s == PNG_EOB ? 1u : 0u;
        for (int k = 0; k < 3; ++k)
            png_walk_runs(fb.data(), cut[k], cut[k + 1], next_after[k], [&](int, int L, int byte) {
                png_run_count(L, byte, [&](int s, int c) { freq[s] += (uint32_t)c; });
            });
        unsigned char len[288];
        uint16_t code[288], order[PNG_LITLEN], parent[2 * PNG_LITLEN];
        uint32_t weight[2 * PNG_LITLEN];
        memset(len, 0, sizeof(len));
        png_code_lengths_of(freq, PNG_LITLEN, 15, len, order, weight, parent);
        png_dyn_head head;
        png_dynamic_head(len, &head);
        uint32_t dyn = head.bits, fixed = 3;
        for (int s = 0; s < PNG_LITLEN; ++s) {
            const uint32_t extra = (s >= 265 && s < 285) ? (uint32_t)(s - 261) / 4 : 0;
            dyn += freq[s] * (len[s] + extra + (s > PNG_EOB ? 1 : 0));
            fixed += freq[s] * ((uint32_t)png_fixed_len(s) + extra + (s > PNG_EOB ? 5 : 0));
        }
        const int kind = png_pick_kind((uint32_t)n, fixed, dyn, last);
        const int hb = 4 + (first ? 2 : 0);
        std::vector<uint32_t> ow((size_t)(n + 16) / 4 + 1, 0u);
        unsigned char *ob = (unsigned char *)ow.data();
        uint32_t body;
        if (kind == PNG_KIND_STORED) {
            body = (uint32_t)(hb + 5 + n);
            ob[hb] = last ? 1 : 0;
            ob[hb + 1] = (unsigned char)n; ob[hb + 2] = (unsigned char)(n >> 8);
            ob[hb + 3] = (unsigned char)~n; ob[hb + 4] = (unsigned char)(~n >> 8);
            memcpy(ob + hb + 5, fb.data(), (size_t)n);
        } else {
            int dist_bits = 1;
            uint32_t head_bits = head.bits;
            if (kind == PNG_KIND_FIXED) {
                for (int s = 0; s < 288; ++s) { len[s] = (unsigned char)png_fixed_len(s); code[s] = (uint16_t)png_fixed_code(s); }
                dist_bits = 5;
                head_bits = 3;
            } else {
                png_canonical(len, PNG_LITLEN, code);
            }
            writer h(or_host{ow.data()}, 8u * hb);
            if (kind == PNG_KIND_FIXED) h.put((uint32_t)(last ? 1 : 0) | (1u << 1), 3);
            else png_dynamic_head_emit(h, len, &head, last);
            h.flush();
            uint32_t pos = 8u * hb + head_bits;
            for (int k = 0; k < 3; ++k) {                              // every span its own writer at its own bit
                uint32_t bits = 0;
                png_walk_runs(fb.data(), cut[k], cut[k + 1], next_after[k],
                              [&](int, int L, int byte) { bits += png_run_bits(L, byte, len, dist_bits); });
                writer w(or_host{ow.data()}, pos);
                png_walk_runs(fb.data(), cut[k], cut[k + 1], next_after[k],
                              [&](int, int L, int byte) { png_run_emit(w, L, byte, code, len, 0, dist_bits); });
                w.flush();
                pos += bits;
            }
            writer e(or_host{ow.data()}, pos);
            e.put(code[PNG_EOB], len[PNG_EOB]);
            e.flush();
            const uint32_t data_bits = kind == PNG_KIND_DYNAMIC ? dyn : fixed;
            if (pos + len[PNG_EOB] - 8u * hb != data_bits) { printf("block bits differ from the priced bits\n"); exit(3); }
            body = (uint32_t)hb + png_block_bytes(data_bits, last);
            if (!last) { ob[body - 2] = 0xFF; ob[body - 1] = 0xFF; }
        }
        memcpy(ob, "IDAT", 4);
        if (first) { ob[4] = 0x78; ob[5] = 0x01; }
        uint32_t crc = png_crc_bytes(table, 0, ob, body);
        const uint32_t half = body / 3;                               // the join the kernel's threads use
        if (png_crc_join(png_crc_bytes(table, 0, ob, half), png_crc_bytes(table, 0, ob + half, body - half), body - half) != crc) {
            printf("CRC join differs\n");
            exit(3);
        }
        png_put_be32(out.data() + at, body - 4 + (last ? 4 : 0));
        memcpy(out.data() + at + 4, ob, body);
        at += 4 + body;
        if (last) {
            png_put_be32(out.data() + at, (ad_b << 16) | ad_a);
            for (int k = 0; k < 4; ++k) crc = png_crc_byte(crc, out[at + k]);
            at += 4;
        }
        png_put_be32(out.data() + at, crc);
        at += 4;
    }
    at += (size_t)png_put_end(out.data() + at);
    out.resize(at);
    return out;
}

static bool take(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    char magic[4];
    int32_t cases = 0;
    if (!take(f, magic, 4) || memcmp(magic, "PNGC", 4) || !take(f, &cases, 4)) return 2;
    int bad = 0;
    for (int k = 0; k < cases; ++k) {
        int32_t type;
        if (!take(f, &type, 4)) return 2;
        if (type == 0) {
            int32_t W, H, pal;
            if (!take(f, &W, 4) || !take(f, &H, 4) || !take(f, &pal, 4)) return 2;
            std::vector<unsigned char> palette(pal ? PNG_PLTE_BYTES : 0), pix((size_t)W * H);
            long long n;
            if (!take(f, palette.data(), palette.size()) || !take(f, pix.data(), pix.size()) || !take(f, &n, 8)) return 2;
            std::vector<unsigned char> want((size_t)n);
            if (!take(f, want.data(), want.size())) return 2;
            const std::vector<unsigned char> got = encode(pix.data(), W, H, pal ? palette.data() : nullptr);
            const bool ok = got == want && (long long)got.size() <= png_file_bound(W, H, pal);
            printf("case %d encode %dx%d %zu bytes -> %s\n", k, W, H, got.size(), ok ? "ok" : "DIFFERS");
            bad += !ok;
        } else if (type == 1) {
            int32_t g[5];
            uint32_t ref_bits;
            std::vector<float> thr(PNG_THRESHOLDS);
            if (!take(f, g, 20) || !take(f, &ref_bits, 4) || !take(f, thr.data(), 4 * PNG_THRESHOLDS)) return 2;
            const int T = g[0], ldf = g[1], F = g[2], W = g[3], H = g[4];
            std::vector<float> mag((size_t)T * ldf);
            std::vector<int32_t> tab((size_t)2 * H + 2 * W);
            std::vector<unsigned char> want((size_t)W * H), got((size_t)W * H, 0);
            if (!take(f, mag.data(), 4 * mag.size()) || !take(f, tab.data(), 4 * tab.size()) || !take(f, want.data(), want.size())) return 2;
            const png_i64 row[PNG_LEVEL_META] = {0, T, ldf, F, W, H, 0, 2 * H, 0, 0};
            float ref;
            memcpy(&ref, &ref_bits, 4);
            if (png_levels_row_ok(row, (png_i64)mag.size() - (ldf - F), (png_i64)tab.size(), (png_i64)got.size()) && png_ref_ok(ref)) {
                float prod[PNG_THRESHOLDS];
                for (int i = 0; i < PNG_THRESHOLDS; ++i) prod[i] = png_fmul(thr[i], ref);
                for (int j = 0; j < H; ++j)
                    for (int i = 0; i < W; ++i) {
                        const int f_lo = png_clamp(tab[2 * j], 0, F), f_hi = png_clamp(tab[2 * j + 1], f_lo, F);
                        const int t_lo = png_clamp(tab[2 * H + 2 * i], 0, T), t_hi = png_clamp(tab[2 * H + 2 * i + 1], t_lo, T);
                        float v = 0.f;
                        for (int t = t_lo; t < t_hi; ++t)
                            for (int b = f_lo; b < f_hi; ++b) v = png_cell_max(v, mag[(size_t)t * ldf + b]);
                        got[(size_t)j * W + i] = (unsigned char)png_level(v, prod);
                    }
            }
            const bool ok = got == want;
            printf("case %d levels %dx%d -> %s\n", k, W, H, ok ? "ok" : "DIFFERS");
            bad += !ok;
        } else {
            return 2;
        }
    }
    fclose(f);
    return bad ? 1 : 0;
}
