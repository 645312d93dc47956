// amt_roll_core.h on the host, alone: built by tests/test_roll_cpu.py with the address and undefined-behaviour
// sanitizers and run directly.  Reads packed cases, draws each the way the kernel does -- pitch by pitch, the running
// maxima of both sides into arrays of exactly the lists' sizes (roll_prefix_max), per column two edges, roll_side per
// side, roll_pixel, the pitch's row_px rows -- and writes the images' bytes to stdout, one after the other.
//
// File: "ROLL", int32 n; per case: int64 meta[10] (W, row_px, pitch_lo, pitch_hi, t0, t1, tick, pair, 0, 0), int32
// group[128], int32 n_est, n_gold; then per side pitch int32[n], program int32[n], on int64[n], off int64[n] (little
// endian, sorted by (pitch, on, off, program)).
#include <stdio.h>
#include <string.h>
#include <vector>
#include "amt_roll_core.h"

struct side {
    std::vector<int32_t> pitch, program;
    std::vector<score_i64> on, off, pmax;
    std::vector<int> parg;
    score_notes view() const { return score_notes{pitch.data(), program.data(), on.data(), off.data()}; }
};

static bool read_exact(FILE *f, void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

static bool read_side(FILE *f, int n, side *s) {
    s->pitch.resize(n); s->program.resize(n); s->on.resize(n); s->off.resize(n); s->pmax.resize(n); s->parg.resize(n);
    return read_exact(f, s->pitch.data(), 4u * n) && read_exact(f, s->program.data(), 4u * n) &&
           read_exact(f, s->on.data(), 8u * n) && read_exact(f, s->off.data(), 8u * n);
}

static void draw(const score_i64 *m, side &es, side &gs, const int32_t *group, std::vector<unsigned char> *image) {
    const score_notes E = es.view(), G = gs.view();
    const score_i64 W = m[ROLL_M_W], px = m[ROLL_M_ROW_PX], t0 = m[ROLL_M_T0], span = m[ROLL_M_T1] - m[ROLL_M_T0];
    const int pair = (int)m[ROLL_M_PAIR];
    image->assign((size_t)(W * roll_height(m)), 0xEE);
    std::vector<unsigned char> row((size_t)W);
    for (int pitch = (int)m[ROLL_M_PITCH_LO]; pitch <= (int)m[ROLL_M_PITCH_HI]; ++pitch) {
        score_i64 e0, e1, g0 = 0, g1 = 0;
        score_pitch_range(E.pitch, 0, (score_i64)es.pitch.size(), pitch, &e0, &e1);
        roll_prefix_max(E, e0, e1, es.pmax.data(), es.parg.data());
        if (pair) {
            score_pitch_range(G.pitch, 0, (score_i64)gs.pitch.size(), pitch, &g0, &g1);
            roll_prefix_max(G, g0, g1, gs.pmax.data(), gs.parg.data());
        }
        for (score_i64 x = 0; x < W; ++x) {
            const score_i64 c0 = roll_edge(t0, span, W, x), c1 = roll_edge(t0, span, W, x + 1);
            const roll_hit est = roll_side(E, es.pmax.data(), es.parg.data(), e0, e1, c0, c1);
            roll_hit gold = {0, 0, 0};
            if (pair) gold = roll_side(G, gs.pmax.data(), gs.parg.data(), g0, g1, c0, c1);
            const int32_t g = (est.covered && !pair) ? group[E.program[est.drawn] & (SCORE_PROGRAMS - 1)] : 0;
            row[(size_t)x] = roll_pixel(pitch, roll_tick_hit(c0, c1, m[ROLL_M_TICK]), pair, est, gold, g);
        }
        for (score_i64 r = 0; r < px; ++r)
            memcpy(image->data() + ((m[ROLL_M_PITCH_HI] - pitch) * px + r) * W, row.data(), (size_t)W);
    }
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: roll_host_main cases.bin > images\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char magic[4];
    int32_t n = 0;
    if (!read_exact(f, magic, 4) || memcmp(magic, "ROLL", 4) != 0 || !read_exact(f, &n, 4) || n < 0) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    for (int c = 0; c < n; ++c) {
        score_i64 meta[ROLL_META];
        int32_t head[2];
        std::vector<int32_t> group(SCORE_PROGRAMS);
        side es, gs;
        if (!read_exact(f, meta, sizeof meta) || !read_exact(f, group.data(), 4 * SCORE_PROGRAMS) || !read_exact(f, head, 8) ||
            head[0] < 0 || head[1] < 0 || !read_side(f, head[0], &es) || !read_side(f, head[1], &gs)) {
            fprintf(stderr, "case %d: short file\n", c);
            return 2;
        }
        if (!roll_geometry_ok(meta)) { fprintf(stderr, "case %d: geometry outside the limits\n", c); return 3; }
        for (int i = 0; i < head[0]; ++i)
            if (!score_note_ok(es.pitch[i], es.program[i])) { fprintf(stderr, "case %d: bad estimate %d\n", c, i); return 3; }
        for (int i = 0; i < head[1]; ++i)
            if (!score_note_ok(gs.pitch[i], gs.program[i])) { fprintf(stderr, "case %d: bad gold note %d\n", c, i); return 3; }
        std::vector<unsigned char> image;
        draw(meta, es, gs, group.data(), &image);
        if (fwrite(image.data(), 1, image.size(), stdout) != image.size()) { fprintf(stderr, "case %d: short write\n", c); return 2; }
    }
    fclose(f);
    return 0;
}
