// amt_score_core.h on the host, alone: built by tests/test_score_cpu.py with the address and undefined-behaviour
// sanitizers and run directly.  Reads packed pairs, scores each the way the kernel does -- pitch by pitch, candidate
// ranges, score_max_matching per variant with arrays of exactly the sizes the rule states, score_frames -- and prints the
// ten counts of every pair, one line each.
//
// File: "SCOR", int32 n; per pair: int32 n_est, n_ref; int32 group[128]; then per side pitch int32[n], program int32[n],
// on int64[n], off int64[n] (little endian, sorted by (pitch, on, off, program)).
#include <stdio.h>
#include <string.h>
#include <vector>
#include "amt_score_core.h"

struct side {
    std::vector<int32_t> pitch, program;
    std::vector<score_i64> on, off;
    score_notes view() const { return score_notes{pitch.data(), program.data(), on.data(), off.data()}; }
};

static bool read_exact(FILE *f, void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

static bool read_side(FILE *f, int n, side *s) {
    s->pitch.resize(n); s->program.resize(n); s->on.resize(n); s->off.resize(n);
    return read_exact(f, s->pitch.data(), 4u * n) && read_exact(f, s->program.data(), 4u * n) &&
           read_exact(f, s->on.data(), 8u * n) && read_exact(f, s->off.data(), 8u * n);
}

// the candidates of r one after the other: what the kernel's wave does 64 at a time
struct serial_scan {
    const score_notes &E, &R;
    const int32_t *group;
    const int *lo, *hi, *owner, *visited;
    score_i64 e0, r0;
    int variant;
    void operator()(int r, int stamp, int *free_e, int *next_e) const {
        for (int e = lo[r]; e < hi[r]; ++e) {
            if (visited[e] == stamp || !score_edge(variant, E, e0 + e, R, r0 + r, group)) continue;
            if (owner[e] < 0) { *free_e = e; return; }
            if (*next_e < 0) *next_e = e;
        }
    }
};

static void score_pair(const side &es, const side &rs, const int32_t *group, score_i64 *out) {
    const score_notes E = es.view(), R = rs.view();
    const score_i64 n_est = (score_i64)es.pitch.size(), n_ref = (score_i64)rs.pitch.size();
    for (int k = 0; k < SCORE_OUT; ++k) out[k] = 0;
    out[0] = n_est;
    out[1] = n_ref;
    score_i64 top = 0;
    for (int pitch = 0; pitch < SCORE_PITCHES; ++pitch) {
        score_i64 e0, e1, r0, r1;
        score_pitch_range(E.pitch, 0, n_est, pitch, &e0, &e1);
        score_pitch_range(R.pitch, 0, n_ref, pitch, &r0, &r1);
        const int ne = (int)(e1 - e0), nr = (int)(r1 - r0);
        if (ne == 0 && nr == 0) continue;
        if (ne > 0 && nr > 0) {
            std::vector<int> lo(nr), hi(nr);
            for (int r = 0; r < nr; ++r) score_candidates(E.on, e0, e1, R.on[r0 + r], &lo[r], &hi[r]);
            for (int v = 0; v < SCORE_VARIANTS; ++v) {
                std::vector<int> owner(ne, -1), visited(ne, 0), stack_ref(nr), stack_via(nr);
                const serial_scan scan = {E, R, group, lo.data(), hi.data(), owner.data(), visited.data(), e0, r0, v};
                out[2 + v] += score_max_matching(nr, owner.data(), visited.data(), stack_ref.data(), stack_via.data(), scan);
            }
        }
        score_i64 count[3], pitch_top;
        score_frames(E, e0, e1, R, r0, r1, count, &pitch_top);
        for (int k = 0; k < 3; ++k) out[6 + k] += count[k];
        if (pitch_top > top) top = pitch_top;
    }
    out[9] = score_frames_below(top);
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: score_host_main cases.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char magic[4];
    int32_t n = 0;
    if (!read_exact(f, magic, 4) || memcmp(magic, "SCOR", 4) != 0 || !read_exact(f, &n, 4) || n < 0) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    for (int c = 0; c < n; ++c) {
        int32_t head[2];
        std::vector<int32_t> group(SCORE_PROGRAMS);
        side es, rs;
        if (!read_exact(f, head, 8) || head[0] < 0 || head[1] < 0 || !read_exact(f, group.data(), 4 * SCORE_PROGRAMS) ||
            !read_side(f, head[0], &es) || !read_side(f, head[1], &rs)) {
            fprintf(stderr, "case %d: short file\n", c);
            return 2;
        }
        for (int i = 0; i < head[0]; ++i)
            if (!score_note_ok(es.pitch[i], es.program[i])) { fprintf(stderr, "case %d: bad estimate %d\n", c, i); return 3; }
        for (int i = 0; i < head[1]; ++i)
            if (!score_note_ok(rs.pitch[i], rs.program[i])) { fprintf(stderr, "case %d: bad reference %d\n", c, i); return 3; }
        score_i64 out[SCORE_OUT];
        score_pair(es, rs, group.data(), out);
        printf("case %d:", c);
        for (int k = 0; k < SCORE_OUT; ++k) printf(" %lld", out[k]);
        printf("\n");
    }
    fclose(f);
    return 0;
}
