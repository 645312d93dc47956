// The scratch layouts on the host, alone: built by tests/test_scratch_cpu.py with the address and undefined-behaviour
// sanitizers and run directly.  For every case of every module the layout function counts with a null base, exactly that
// many bytes come from malloc, the same function carves them, and every region is filled with its own tag: a region that
// reaches past the count is the address sanitizer's report, a region that is misaligned or meets another is this
// program's.  Prints one line per case, "<module> <arguments ...> -> <bytes>", for the test to hold against the closed
// formulas and the library.  The carver's refusals come first.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "amt_flacdec_core.h"
#include "amt_png_core.h"
#include "amt_score_core.h"

struct region { const void *p; long long bytes, align; };

#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); exit(1); } } while (0)

// make(base) runs the module's layout function on `base`, lists the regions and returns the bytes
template <class Make>
static long long carve(Make make) {
    std::vector<region> none, regions;
    const long long total = make(nullptr, &none);
    REQUIRE(total >= 0);
    for (const region &r : none) REQUIRE(r.p == nullptr);
    unsigned char *base = (unsigned char *)malloc((size_t)total);      // exactly the count: one byte more is a report
    REQUIRE(base || total == 0);
    REQUIRE(make(base, &regions) == total && regions.size() == none.size());
    for (size_t k = 0; k < regions.size(); ++k) {
        const region &r = regions[k];
        REQUIRE(r.bytes == none[k].bytes && r.bytes >= 0);
        const long long at = (const unsigned char *)r.p - base;
        REQUIRE(at >= 0 && at % r.align == 0 && at + r.bytes <= total);
        if (r.bytes) memset(base + at, (int)(k + 1), (size_t)r.bytes);
    }
    for (size_t k = 0; k < regions.size(); ++k) {                      // disjoint: every region still holds its tag
        const unsigned char *p = (const unsigned char *)regions[k].p;
        for (long long i = 0; i < regions[k].bytes; ++i) REQUIRE(p[i] == (unsigned char)(k + 1));
    }
    free(base);
    return total;
}

static void carver_refusals() {
    long long word[4];
    amt_carver a(word);
    REQUIRE(a.take<int>(1) == (int *)word && a.take<long long>(1) == word + 1 && a.at == 16 && !a.failed);
    REQUIRE(a.take<int>(-1) == nullptr && a.failed && a.at == 16);                     // a negative count
    REQUIRE(a.take<int>(1) == nullptr && a.failed && a.at == 16);                      // ... and it sticks
    amt_carver b(nullptr);
    REQUIRE(b.take<long long>(LLONG_MAX / 4) == nullptr && b.failed && b.at == 0);     // count * size leaves int64
    amt_carver c(nullptr);
    REQUIRE(c.take<unsigned char>(LLONG_MAX - 8) == nullptr && !c.failed && c.at == LLONG_MAX - 8);   // (counting only)
    REQUIRE(c.take<unsigned char>(16) == nullptr && c.failed && c.at == LLONG_MAX - 8);                 // the end does
    amt_carver d(nullptr);
    d.take<unsigned char>(LLONG_MAX - 8);
    REQUIRE(d.take<unsigned char>(0, 16) == nullptr && d.failed);                      // the round-up does
    amt_carver e(nullptr);
    REQUIRE(e.take<int>(1, 0) == nullptr && e.failed);
    amt_flac_layout F;
    REQUIRE(amt_flac_make_layout(nullptr, -1, 1, 48, &F) < 0 && amt_flac_make_layout(nullptr, 1, -1, 48, &F) < 0);
    REQUIRE(amt_flac_make_layout(nullptr, 1LL << 31, 1LL << 31, 12304, &F) < 0);
    REQUIRE(amt_flac_make_layout(nullptr, 1LL << 40, 1LL << 30, 1, &F) < 0);
    fd_layout D;
    REQUIRE(fd_make_layout(nullptr, -1, 0, &D) < 0 && fd_make_layout(nullptr, 0, -1, &D) < 0);
    REQUIRE(fd_make_layout(nullptr, (1LL << 40) + 1, 0, &D) < 0 && fd_make_layout(nullptr, 0, (1LL << 56) + 1, &D) < 0);
    score_scratch S;
    REQUIRE(score_make_layout(nullptr, -1, 0, &S) < 0 && score_make_layout(nullptr, 0, SCORE_MAX_NOTES + 1, &S) < 0);
    REQUIRE(score_make_layout(nullptr, SCORE_MAX_NOTES, SCORE_MAX_NOTES, &S) > 0);
    png_layout P;
    const long long wide[3] = {0, PNG_MAX_DIM + 1, 1}, none[3] = {0, 0, 1}, before[3] = {-1, 1, 1};
    REQUIRE(png_make_layout(nullptr, wide, 1, 0, &P, nullptr) < 0 && png_make_layout(nullptr, none, 1, 0, &P, nullptr) < 0);
    REQUIRE(png_make_layout(nullptr, before, 1, 0, &P, nullptr) < 0 && png_make_layout(nullptr, wide, 0, 0, &P, nullptr) < 0);
    printf("carver ok\n");
}

int main() {
    carver_refusals();

    // FLAC encoder: no signal, no frame, one; the two ends of block size and sample size; block size 17 at 24 bits is a
    // 67-byte slot, so 1 .. 9 slots end one below, on and one above the 8-byte step
    const int flac[][4] = {{0, 100, 16, 16}, {1, 0, 16, 16}, {1, 1, 16, 16}, {1, 16, 16, 24}, {3, 17, 16, 24},
                           {1, 4096, 4096, 16}, {2, 4097, 4096, 24}, {5, 40000, 4096, 24}, {3, 100, 4096, 16},
                           {1, 17, 17, 24}, {2, 17, 17, 24}, {3, 17, 17, 24}, {4, 17, 17, 24}, {5, 17, 17, 24},
                           {6, 17, 17, 24}, {7, 17, 17, 24}, {8, 17, 17, 24}, {9, 17, 17, 24}, {3, 35, 17, 24}};
    for (const auto &c : flac) {
        const long long n = c[0], frames = (c[1] + c[2] - 1) / c[2], bound = 13 + (8 + (long long)c[2] * c[3] + 7) / 8 + 2;
        const long long total = carve([&](void *base, std::vector<region> *r) {
            amt_flac_layout L;
            const long long t = amt_flac_make_layout(base, n, frames, bound, &L);
            *r = {{L.slots, n * frames * bound, 1}, {L.frame_off, 8 * n * frames, 8}};
            return t;
        });
        printf("flac %d %d %d %d -> %lld\n", c[0], c[1], c[2], c[3], total);
    }

    // FLAC decoder: 4 * slot_ints below, on and above the 8-byte step; no candidate, one, several
    const long long dec[][2] = {{0, 0}, {0, 5}, {1, 0}, {1, 1}, {1, 2}, {1, 3}, {5, 4}, {5, 4095}, {5, 4096}, {5, 4097},
                                {64, 65536}, {65, 65537}};
    for (const auto &c : dec) {
        const long long total = carve([&](void *base, std::vector<region> *r) {
            fd_layout L;
            const long long t = fd_make_layout(base, c[0], c[1], &L);
            *r = {{L.slots, 4 * c[1], 4}, {L.next, 8 * c[0], 8}, {L.first, 8 * c[0], 8}};
            return t;
        });
        printf("flacdec %lld %lld -> %lld\n", c[0], c[1], total);
    }

    // scoring: 4 n below, on and above the 16-byte step, on either side
    const long long counts[] = {0, 1, 3, 4, 5, 7, 8, 9, 1000, 1001};
    for (long long ne : counts)
        for (long long nr : counts) {
            const long long total = carve([&](void *base, std::vector<region> *r) {
                score_scratch S;
                const long long t = score_make_layout(base, ne, nr, &S);
                *r = {{S.lo, 4 * nr, 16}, {S.hi, 4 * nr, 16}};
                for (int v = 0; v < SCORE_VARIANTS; ++v) {
                    r->push_back({S.owner[v], 4 * ne, 16});
                    r->push_back({S.visited[v], 4 * ne, 16});
                    r->push_back({S.stack_ref[v], 4 * nr, 16});
                    r->push_back({S.stack_via[v], 4 * nr, 16});
                }
                return t;
            });
            printf("score %lld %lld -> %lld\n", ne, nr, total);
        }

    // PNG: 1 x 1, 3 x 2, the widest accepted row, an image of several pieces; one, two and three images (8 n bytes of
    // sizes below and on the 16-byte step); lists are W, H pairs
    const std::vector<std::vector<long long>> png = {
        {1, 1}, {3, 2}, {PNG_MAX_DIM, 1}, {PNG_MAX_DIM, 3}, {1, PNG_MAX_DIM}, {300, 250}, {1, 1, 3, 2}, {3, 2, 1, 1, 3, 2},
        {PNG_MAX_DIM, 2, 1, 1, 129, 300}, {5, 7, 6, 7, 7, 7, 8, 7, 9, 7}};
    for (const auto &c : png) {
        const int n = (int)c.size() / 2;
        std::vector<long long> meta;
        long long at = 3;
        for (int i = 0; i < n; ++i) {
            meta.insert(meta.end(), {at, c[2 * i], c[2 * i + 1]});
            at += c[2 * i] * c[2 * i + 1];
        }
        const long long total = carve([&](void *base, std::vector<region> *r) {
            png_layout L;
            std::vector<png_i64> tables;
            const long long t = png_make_layout(base, meta.data(), n, 1, &L, &tables);
            REQUIRE((long long)tables.size() == 4 * (n + L.P) && L.cap % 16 == 0);
            REQUIRE(!base || L.pieces == L.meta + 4 * n);                              // one upload fills both tables
            *r = {{L.meta, 32LL * n, 16}, {L.pieces, 32 * L.P, 8}, {L.res, 4 * PNG_RES * L.P, 16}, {L.sizes, 8LL * n, 16},
                  {L.piece_off, 8 * L.P, 16}, {L.slots, L.slot_bytes, 16}};
            return t;
        });
        printf("png");
        for (long long v : c) printf(" %lld", v);
        printf(" -> %lld\n", total);
    }
    return 0;
}
