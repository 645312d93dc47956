// Stand-alone CPU program over csrc/amt_flacdec_core.h, the decoder core the kernels compile.  Built by
// tests/test_flac_decode_cpu.py with the address and undefined-behaviour sanitizers and run directly.
//
//   flacdec_host_main CORPUS
//
// CORPUS (little-endian): "FDC1", int32 streams; per stream: int32 expect (0: must decode to the PCM given, 1: must be
// refused), int32 channels, int32 bps, int64 total, int64 first frame byte, int64 file bytes, the bytes, int32
// candidates, per candidate int64 position and int32 header bytes / block size / assignment / bps, then for expect 0
// int32 PCM [total][channels].  Every stream's bytes are copied into an allocation of exactly their size, so a read
// past the end is a sanitizer report.  Exit 0: every stream did what was expected.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "amt_flacdec_core.h"

static bool get(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    char magic[4];
    int32_t streams = 0;
    if (!get(f, magic, 4) || memcmp(magic, "FDC1", 4) || !get(f, &streams, 4)) return 2;
    int bad = 0;
    for (int s = 0; s < streams; ++s) {
        int32_t expect, channels, bps, ncand;
        int64_t total, first_byte, bytes;
        if (!get(f, &expect, 4) || !get(f, &channels, 4) || !get(f, &bps, 4) || !get(f, &total, 8) ||
            !get(f, &first_byte, 8) || !get(f, &bytes, 8))
            return 2;
        unsigned char *data = (unsigned char *)malloc(bytes ? (size_t)bytes : 1);
        if (!get(f, data, (size_t)bytes) || !get(f, &ncand, 4)) return 2;
        std::vector<fd_i64> cm(5 * (size_t)ncand + 1), next(ncand + 1), first(ncand + 1), cand_out(3 * (size_t)ncand + 1);
        std::vector<std::vector<int32_t>> slots(ncand);
        for (int c = 0; c < ncand; ++c) {
            int64_t pos;
            int32_t v[4];
            if (!get(f, &pos, 8) || !get(f, v, 16)) return 2;
            cm[5 * c] = pos;
            for (int j = 0; j < 4; ++j) cm[5 * c + 1 + j] = v[j];
        }
        std::vector<int32_t> want;
        if (expect == 0) {
            want.resize((size_t)(total * channels));
            if (!get(f, want.data(), want.size() * 4)) return 2;
        }
        // every candidate, speculatively
        int32_t hist[FD_HIST], coef[FD_HIST];
        for (int c = 0; c < ncand; ++c) {
            const int bs = (int)cm[5 * c + 2];
            uint64_t end = 0;
            int err = FD_E_TABLE;
            if (bs >= 1 && bs <= FD_MAX_BLOCK && channels >= 1 && channels <= FD_MAX_CHANNELS) {
                slots[c].assign((size_t)bs * channels, 0);
                err = fd_frame(data, (uint64_t)bytes, (uint64_t)cm[5 * c], (int)cm[5 * c + 1], bs, (int)cm[5 * c + 3],
                               (int)cm[5 * c + 4], channels, slots[c].data(), hist, coef, 1, &end);
            }
            cand_out[3 * c] = (fd_i64)end;
            cand_out[3 * c + 1] = err;
            cand_out[3 * c + 2] = 0;
        }
        for (int c = 0; c < ncand; ++c)
            next[c] = cand_out[3 * c + 1] == FD_OK ? fd_find(cm.data(), 5, 0, ncand, cand_out[3 * c]) : -1;
        fd_i64 at = first_byte;
        int code = fd_walk(cm.data(), 5, cm.data() + 2, 0, ncand, first_byte, total, next.data(), cand_out.data(),
                           first.data(), &at);
        // CRC-16 and placement of the on-chain frames
        std::vector<int32_t> got((size_t)(total * channels), 0);
        bool crc_bad = false;
        for (int c = 0; c < ncand && code == FD_S_OK; ++c) {
            if (cand_out[3 * c + 2] != 1) continue;
            const fd_i64 pos = cm[5 * c], end = cand_out[3 * c];
            const int bs = (int)cm[5 * c + 2], ca = (int)cm[5 * c + 3];
            if (fd_crc16(data + pos, (uint64_t)(end - 2 - pos)) != (((unsigned)data[end - 2] << 8) | data[end - 1]))
                crc_bad = true;
            for (int i = 0; i < bs && first[c] + i < total; ++i)
                for (int k = 0; k < channels; ++k) {
                    const int32_t *sl = slots[c].data();
                    got[(size_t)((first[c] + i) * channels + k)] =
                        ca < 8 ? sl[(size_t)k * bs + i] : fd_stereo(ca, k, sl[i], sl[bs + i]);
                }
        }
        const bool refused = code != FD_S_OK || crc_bad;
        bool ok;
        if (expect == 0) ok = !refused && got == want;
        else ok = refused;
        int frame_err = 0;                                                         // of the candidate the walk stopped at
        for (int c = 0; c < ncand; ++c)
            if (code != FD_S_OK && cm[5 * c] == at) frame_err = (int)cand_out[3 * c + 1];
        printf("stream %d: expect %d status %d at %lld frame_err %d crc_bad %d -> %s\n", s, expect, code, (long long)at,
               frame_err, (int)crc_bad, ok ? "ok" : "WRONG");
        bad += !ok;
        free(data);
    }
    fclose(f);
    return bad ? 1 : 0;
}
