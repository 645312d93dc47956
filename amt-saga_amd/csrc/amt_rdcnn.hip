// RDCNN forward (res_net.predict) for gfx950, host side: weight folding and pre-arrangement over the topology
// (amt_rdcnn_topology.h), the per-layer launch plan, and the forward walk.  The convolutions are implicit GEMMs on the matrix pipe with fused
// BN + sigmoid (+ shortcut add + BN) epilogues, in three f32-equivalent arithmetics:
//   mode 2 (default) split-fp16, amt_conv_f16x3.h;  mode 1 split-bf16, amt_conv_bf16x6.h;  mode 0 f32 MFMA,
//   amt_conv_f32.h;  mode 3 = mode 2 with the large 4 x 16 layers in the FFT domain (amt_fftconv.h).
// The first layer, shortcut projection, max-pool, Dense and output kernels are in amt_rdcnn_small.h.
//
// Replaces keras Model.predict for the graph built in RDCNN.py:176-233 of the reference (+ _add_shortcut :312-335,
// output scaling :304-310, :591-597) -- see oracle/rdcnn.py for the CPU restatement.
//
// All kernels stay in THIS translation unit: the build gives it per-file code generation flags (build.py).
#include "amt_common.h"
#include "amt_launch.h"
#include "amt_fftconv.h"
#include "amt_convh.h"
#include "amt_rdcnn_topology.h"
#include <vector>
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "amt_conv_f32.h"
#include "amt_conv_bf16x6.h"
#include "amt_conv_f16x3.h"
#include "amt_rdcnn_small.h"

#define RD_BN_EPS 1e-3f

// =====================================================================================
// Host side: weight folding / pre-arrangement, launch plan
// =====================================================================================
// Launch plan of one convolution variant: workgroup tile, LDS bytes, N-slicing and the weights in the variant's layout
struct ConvPlan {
    int TH = 0, TW = 0, NWIN = 1;  // tile of NWIN windows x TH x TW positions (TH == 0: no tile fits)
    size_t lds = 0;
    int nslice = 1, cw = 0;    // output channels are computed in nslice slices (blockIdx.y) of cw channels
    bool masked = false;       // small-image form: whole images per workgroup, no halo
    int wm_ms = 0;             // split-fp16 only, > 0: the window-major small-image form (conv_f16x3w_kernel) runs instead of
    size_t wm_lds = 0;         //   the masked one, with wm_ms positions per wave and wm_lds bytes of LDS
    double eff = 0;            // useful fraction of the tile's positions
    void *w = nullptr;         // device weights (null: the variant is not built for this layer)
};
struct ConvOp {
    int cin, cout, H, W, kh, kw;
    float *s1 = nullptr, *t1 = nullptr, *s2 = nullptr, *t2 = nullptr;
    bool residual = false;
    int sc_proj = -1;          // index into projs, -1 => identity shortcut
    int pool_after = 0;        // 1 => maxpool (ph, pw) follows
    ConvPlan f32;              // f32 MFMA (always built; for the first layer only w: the [tap][cout] kernel as is)
    int MT = 2;                //   its M-tiles per wave
    ConvPlan bf16;             // split-bf16: 128 couts run as two 64-wide slices
    ConvPlan f16;              // split-fp16: 32-wide N-slices, 16x16x32 fragments of tap pairs (conv_f16x3s_kernel)
    int sw = 0;                //   its weights are scaled by 2^sw
    // FFT-domain forms (conv mode 3), built on the first amt_rdcnn_set_mode(net, 3): the row form for the 32 -> 32
    // (4 x 16) layers on images of at most 561 columns (amt_fftconv.hip), the packed-image form for the 64 -> 64
    // (4 x 16) layers on 10 x 64 images (amt_fftpk.hip); k_host keeps the Keras-layout kernel for that
    std::vector<float> k_host;
    FcLayer fc;
};
struct ProjOp {
    int cin, cout, H, W, ph, pw, HO, WO;
    float *w = nullptr, *s = nullptr, *t = nullptr;
};
struct Tower {
    int in_h, in_w, ph, pw;
    std::vector<ConvOp> convs;
    std::vector<ProjOp> projs;
    size_t max_act = 0;        // floats per window of the largest activation
    int out_h, out_w, out_c;
};
struct ProfPending { hipEvent_t e0, e1; int tower, layer, windows; };
struct ProfAcc { double ms = 0, windows = 0; long launches = 0; };
struct amt_rdcnn {
    // optional per-conv-launch timing (HIP events on the caller's stream)
    mutable bool prof_on = false;
    mutable std::vector<ProfPending> prof_pending;
    mutable std::vector<hipEvent_t> prof_free;
    mutable std::vector<std::vector<ProfAcc>> prof_acc;   // [tower][layer]
    // optional layer taps (amt_rdcnn_layer_tap): [tower][layer] device pointers, empty until the first one is set
    mutable std::vector<std::vector<float *>> taps;
    amt_rdcnn_desc d;
    std::vector<Tower> towers;
    std::vector<void *> allocs;
    float *d1w = nullptr, *d1b = nullptr, *d2w = nullptr, *d2b = nullptr;
    int flat = 0;
    double flops = 0;
    mutable int mode = 0;      // 0: f32 MFMA, 1: split-bf16 where built, 2: split-fp16 where built, 3: 2 + FFT-domain forms
    bool fc_pooled = true;     // mode 3: the last FFT-domain layer in front of a max pool (ph, 8) leaves its output W-pooled
                               // (fc_wpooled_ok); AMT_FC_POOLED=0, read when the net is created, keeps the full-size output
};

// host bytes -> a new device allocation owned by the net
template <class T>
static int upload(amt_rdcnn *n, const void *h, size_t bytes, T **out) {
    void *d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) return AMT_E_NOMEM;
    n->allocs.push_back(d);
    if (hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) != hipSuccess) return AMT_E_HIP;
    *out = static_cast<T *>(d);
    return AMT_OK;
}
// BatchNormalization (bn: gamma, beta, mean, variance, c floats each) behind an optional bias, folded to y = s x + t
static int upload_folded_bn(amt_rdcnn *n, const float *bn, int c, const float *bias, float **s_out, float **t_out) {
    const float *g = bn, *b = bn + c, *m = bn + 2 * c, *v = bn + 3 * c;
    std::vector<float> s(c), t(c);
    for (int i = 0; i < c; ++i) {
        const float sc = g[i] / sqrtf(v[i] + RD_BN_EPS);
        s[i] = sc;
        t[i] = b[i] + ((bias ? bias[i] : 0.f) - m[i]) * sc;
    }
    const int rc = upload(n, s.data(), c * sizeof(float), s_out);
    return rc != AMT_OK ? rc : upload(n, t.data(), c * sizeof(float), t_out);
}

// Candidate tiles of at most pcap positions, in the order the choosers try them (a tie keeps the earlier one): whole
// images of several windows, then for every tile height the widest tile and the narrowest one with as many column tiles
template <class F>
static void for_each_tile(int H, int W, int pcap, int max_win, F consider) {
    if (H * W <= pcap)
        for (int nw = std::min(pcap / (H * W), max_win); nw >= 1; --nw) consider(H, W, nw);
    for (int TH = 1; TH <= H && TH <= pcap; ++TH) {
        int TW = pcap / TH;
        if (TW > W) TW = W;
        if (TW >= 1) consider(TH, TW, 1);
        const int nct = (W + TW - 1) / TW;
        const int TW2 = (W + nct - 1) / nct;
        if (TW2 >= 1 && TW2 <= TW) consider(TH, TW2, 1);
    }
}

static void choose_tile(ConvOp &c) {
    ConvPlan &p = c.f32;
    double best = -1;
    for (int MT = 2; MT >= 1; --MT) {
        const int pcap = 128 * MT;
        for_each_tile(c.H, c.W, pcap, pcap, [&](int TH, int TW, int NWIN) {
            const size_t posin = (size_t)NWIN * (TH + c.kh - 1) * (TW + c.kw - 1);
            const size_t lds = posin * RD_CSTRIDE * 4 + 2 * (size_t)RD_CC * p.cw * 4 + (size_t)pcap * 8;
            if (lds > 150 * 1024) return;
            const double tiles = (double)((c.H + TH - 1) / TH) * ((c.W + TW - 1) / TW) / NWIN;
            double eff = (double)c.H * c.W / (tiles * pcap);
            if (lds > 78 * 1024) eff *= 0.93;          // prefer two workgroups per CU
            if (eff > best + 1e-9) { best = eff; p.TH = TH; p.TW = TW; p.NWIN = NWIN; c.MT = MT; p.lds = lds; p.eff = eff; }
        });
    }
}

// Tile of the split-bf16 / split-fp16 kernels: 256 positions, at most max_win windows, LDS for two workgroups per CU.
// lds_of(staged positions) = the kernel's dynamic LDS bytes.
template <class F>
static void choose_tile_split(const ConvOp &c, ConvPlan &p, int max_win, F lds_of) {
    double best = -1;
    const int pcap = 256;
    p.masked = false; p.TH = 0;
    if (c.H * c.W <= 64) {
        // small image: halo-free (masked) tile of whole images, plus one all-zero position
        const int nw = std::min(pcap / (c.H * c.W), max_win);
        const size_t lds = lds_of((size_t)nw * c.H * c.W + 1);
        if (lds <= 79 * 1024) {
            p.masked = true; p.TH = c.H; p.TW = c.W; p.NWIN = nw; p.lds = lds;
            p.eff = (double)nw * c.H * c.W / pcap;
            return;
        }
    }
    for_each_tile(c.H, c.W, pcap, max_win, [&](int TH, int TW, int NWIN) {
        const size_t lds = lds_of((size_t)NWIN * (TH + c.kh - 1) * bx_row_pitch(TW, TW + c.kw - 1));
        if (lds > 79 * 1024) return;                    // two workgroups per CU
        const double tiles = (double)((c.H + TH - 1) / TH) * ((c.W + TW - 1) / TW) / NWIN;
        const double eff = (double)c.H * c.W / (tiles * pcap);
        if (eff > best + 1e-9) { best = eff; p.TH = TH; p.TW = TW; p.NWIN = NWIN; p.lds = lds; p.eff = eff; }
    });
}
static void choose_tile16(ConvOp &c) {
    const int NT = c.bf16.cw / 32, ntaps = c.kh * c.kw;
    const int tps = (NT == 1 && ntaps % 2 == 0) ? 2 : 1;
    const size_t slab = (size_t)tps * 3 * NT * 64 * 16;  // bytes of one weight slab, three buffers
    choose_tile_split(c, c.bf16, 256, [&](size_t npos) { return npos * BX_PSTRIDE + 3 * slab + (size_t)256 * 8; });
}

// ---- the supported shapes, each stated once: what the kernels are instantiated for (amt_dispatch, amt_common.h) ------
// kernel sizes (kh, kw), every family
using ConvKernelSizes = amt_cases<amt_case<4, 16>, amt_case<4, 2>, amt_case<2, 2>>;
// f32 MFMA (cin, slice width)
using F32Shapes = amt_cases<amt_case<32, 32>, amt_case<32, 64>, amt_case<64, 64>, amt_case<64, 128>, amt_case<128, 128>,
                            amt_case<64, 32>, amt_case<128, 32>>;
// split-bf16 (cin, slice width)
using Bf16Shapes = amt_cases<amt_case<32, 32>, amt_case<32, 64>, amt_case<64, 64>, amt_case<128, 64>>;
// split-fp16 cin (32-wide slices), inference and trainer forms
using F16Cins = amt_values<32, 64, 128>;
// split-fp16 window-major (cin, positions per wave), 4 x 16 kernels only
using WmajorShapes = amt_cases<amt_case<32, 3>, amt_case<32, 5>, amt_case<32, 8>, amt_case<64, 3>, amt_case<64, 5>,
                               amt_case<64, 8>, amt_case<128, 3>, amt_case<128, 5>, amt_case<128, 8>>;
using Flag = amt_values<0, 1>;      // a bool template argument
template <class List, class... V>
static bool in_list(List l, V... v) { return amt_dispatch(l, v..., [](auto...) { return (int)AMT_OK; }) == AMT_OK; }
static bool conv_supported(int kh, int kw) { return in_list(ConvKernelSizes{}, kh, kw); }
// channel pairs (cin, cout) of the LAYERS the matrix-pipe convolutions run (all three arithmetics, in the slices above)
static bool conv_channels_supported(int cin, int cout) {
    return (cin == 32 && cout == 32) || (cin == 32 && cout == 64) || (cin == 64 && cout == 64) ||
           (cin == 64 && cout == 128) || (cin == 128 && cout == 128);
}

// ---- the tile of a tiled kernel (its launch: amt_launch.h) -----------------------------------------------------------
// the workgroup tile into the launch parameters; returns the number of position tiles (gridDim.x)
static unsigned apply_tile(ConvParams &p, int TH, int TW, int NWIN) {
    p.TH = TH; p.TW = TW; p.NWIN = NWIN;
    p.tiles_h = (p.H + p.TH - 1) / p.TH; p.tiles_w = (p.W + p.TW - 1) / p.TW;
    const int groups = (p.B + p.NWIN - 1) / p.NWIN;
    return (unsigned)((size_t)groups * p.tiles_h * p.tiles_w);
}
static unsigned apply_plan(ConvParams &p, const ConvPlan &pl) { return apply_tile(p, pl.TH, pl.TW, pl.NWIN); }
static int launch_conv16(const ConvOp &c, ConvParams p, hipStream_t st) {
    const dim3 grid(apply_plan(p, c.bf16), c.bf16.nslice);
    return amt_dispatch(ConvKernelSizes{}, c.kh, c.kw, [&](auto KH, auto KW) {
        return amt_dispatch(Bf16Shapes{}, c.cin, c.bf16.cw, [&](auto CI, auto CW) {
            return amt_dispatch(Flag{}, c.bf16.masked, [&](auto MASKED) {
                return amt_launch<conv_bf16x6_kernel<KH(), KW(), CI(), CW(), MASKED() != 0>>(
                    AMT_LDS_CONV, grid, 512, c.bf16.lds, st, p, static_cast<const uint4 *>(c.bf16.w));
            });
        });
    });
}

// ---- split-fp16 variant: tile choice and launch ---------------------------------------------
#define HX_SLAB_BYTES 4096
#define HX_XCHG_BYTES (8 * 32 * HX_TPITCH * 4)  // epilogue transposition patches (>= the K-split exchange, 8 x 4 KB)
static void choose_tile_h(ConvOp &c) {
    // two weight-group buffers (a group = min(4, steps per chunk) steps of 4 KB)
    const int NTh = c.f16.cw / 32;
    const int nsteps = c.kh * c.kw / (NTh == 1 ? 2 : 1);
    const size_t wbytes = 2 * (size_t)std::min(4, nsteps) * HX_SLAB_BYTES;
    choose_tile_split(c, c.f16, HX_MAXWIN, [&](size_t npos) {
        return std::max(npos * HX_PSTRIDE, (size_t)HX_XCHG_BYTES) + wbytes + (size_t)256 * 12 + (size_t)HX_MAXWIN * 8 + 512;      // + the slice's folded BN parameters
    });
}

// AMT_CONV_TS diagnostic: phase split of a workgroup's life, four 100-MHz timestamps per workgroup of a split-fp16 launch
static bool conv_ts_wanted() { static const bool want = amt_env_switch("AMT_CONV_TS", false); return want; }
static int conv_ts_buffer(size_t nwg, unsigned long long **out) {
    static unsigned long long *ts_dev = nullptr;
    static size_t ts_cap = 0;
    if (nwg > ts_cap) {
        if (ts_dev) (void)hipFree(ts_dev);
        ts_dev = nullptr; ts_cap = 0;
        AMT_HIP_CHECK(hipMalloc(&ts_dev, nwg * 4 * sizeof(unsigned long long)));
        ts_cap = nwg;
    }
    *out = ts_dev;
    return AMT_OK;
}
// form: "masked0", "masked1" or "wmajor"; slots = workgroups the chip holds at once
static int conv_ts_report(const ConvOp &c, const char *form, const unsigned long long *ts_dev, size_t nwg, int slots, hipStream_t st) {
    AMT_HIP_CHECK(hipStreamSynchronize(st));
    std::vector<unsigned long long> h(nwg * 4);
    AMT_HIP_CHECK(hipMemcpy(h.data(), ts_dev, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    double a = 0, b = 0, e = 0;
    unsigned long long t0 = ~0ull, t1 = 0;
    for (size_t i = 0; i < nwg; ++i) {
        a += (double)(h[4 * i + 1] - h[4 * i]); b += (double)(h[4 * i + 2] - h[4 * i + 1]);
        e += (double)(h[4 * i + 3] - h[4 * i + 2]);
        t0 = std::min(t0, h[4 * i]); t1 = std::max(t1, h[4 * i + 3]);
    }
    fprintf(stderr, "conv_ts k%dx%d cin%d %dx%d %s wgs %zu: start->first MFMA %.2f us, MFMA loop %.2f us, epilogue %.2f us; "
                    "kernel %.1f us = %.2f workgroup lives per slot of %d\n",
            c.kh, c.kw, c.cin, c.H, c.W, form, nwg, a / nwg / 100.0, b / nwg / 100.0, e / nwg / 100.0,
            (double)(t1 - t0) / 100.0, (double)(t1 - t0) * slots / ((a + b + e)), slots);
    return AMT_OK;
}
// The inference net's 4 x 16 layers on small images (the masked plan of choose_tile_h) take the window-major form
// instead (amt_conv_f16x3.h): 3, 5 or 8 positions per wave.  AMT_CONV_WMAJOR=0, read here = when a net is created,
// keeps them on the masked form (A/B measurements, tests/test_gpu_small_conv.py).
static void choose_tile_w(ConvOp &c) {
    ConvPlan &p = c.f16;
    p.wm_ms = 0;
    if (!amt_env_switch("AMT_CONV_WMAJOR", true)) return;
    if (!p.masked || c.kh != 4 || c.kw != 16 || !in_list(F16Cins{}, c.cin)) return;
    const int npos = c.H * c.W, ms = (npos + HXW_NWAVE - 1) / HXW_NWAVE;
    p.wm_ms = ms <= 3 ? 3 : ms <= 5 ? 5 : 8;
    p.wm_lds = hxw_lds_bytes<16>(npos);
}

// split-fp16 single-tile kernel on the plan's tile: 32-wide N-slices in blockIdx.y, small images its masked form;
// TRAIN: the trainer's form (amt_convh_run)
template <bool TRAIN>
static int launch_convs(int kh, int kw, int cin, bool masked, dim3 grid, size_t lds, const ConvParams &p, const void *w,
                        const HxScale &hs, hipStream_t st) {
    return amt_dispatch(ConvKernelSizes{}, kh, kw, [&](auto KH, auto KW) {
        return amt_dispatch(F16Cins{}, cin, [&](auto CI) {
            return amt_dispatch(Flag{}, masked, [&](auto MASKED) {
                return amt_launch<conv_f16x3s_kernel<KH(), KW(), CI(), MASKED() != 0, 2, TRAIN>>(
                    AMT_LDS_CONV, grid, 512, lds, st, p, static_cast<const uint4 *>(w), hs);
            });
        });
    });
}
// The inference forms.  Window-major (wm_ms > 0): 16 windows x all positions x 32 output channels per workgroup, the
// N-slice in the low bits of the 1-D workgroup id; one workgroup per CU
static int launch_convh(const ConvOp &c, ConvParams p, const float *amax_in, float *amax_out, hipStream_t st) {
    const ConvPlan &pl = c.f16;
    const bool wmajor = pl.wm_ms > 0;
    if (!pl.w || pl.cw != 32) return AMT_E_UNSUPPORTED;
    if (wmajor && (c.kh != 4 || c.kw != 16 || c.H * c.W > 8 * pl.wm_ms)) return AMT_E_UNSUPPORTED;
    const unsigned grid = wmajor ? apply_tile(p, p.H, p.W, HXW_WIN) : apply_plan(p, pl);
    const size_t nwg = (size_t)grid * pl.nslice;
    HxScale hs{amax_in, amax_out, c.sw, nullptr};
    if (conv_ts_wanted()) { const int rc = conv_ts_buffer(nwg, &hs.ts); if (rc != AMT_OK) return rc; }
    const int rc = !wmajor ? launch_convs<false>(c.kh, c.kw, c.cin, pl.masked, dim3(grid, pl.nslice), pl.lds, p, pl.w, hs, st)
                           : amt_dispatch(WmajorShapes{}, c.cin, pl.wm_ms, [&](auto CI, auto MS) {
                                 return amt_launch<conv_f16x3w_kernel<4, 16, CI(), MS()>>(
                                     160 * 1024, dim3((unsigned)nwg), 64 * HXW_NWAVE, pl.wm_lds, st, p,
                                     static_cast<const uint4 *>(pl.w), hs, pl.nslice);
                             });
    if (rc != AMT_OK || !hs.ts) return rc;
    return conv_ts_report(c, wmajor ? "wmajor" : pl.masked ? "masked1" : "masked0", hs.ts, nwg, wmajor ? 256 : 512, st);
}

static int launch_conv(const ConvOp &c, ConvParams p, hipStream_t st) {
    const dim3 grid(apply_plan(p, c.f32), c.f32.nslice);
    return amt_dispatch(ConvKernelSizes{}, c.kh, c.kw, [&](auto KH, auto KW) {
        return amt_dispatch(F32Shapes{}, c.cin, c.f32.cw, [&](auto CI, auto CW) {
            return amt_dispatch(amt_values<2, 1>{}, c.MT, [&](auto MT) {
                return amt_launch<conv_mfma_kernel<KH(), KW(), CI(), CW(), MT()>>(152 * 1024, grid, 256, c.f32.lds, st, p);
            });
        });
    });
}

static void choose_tile1(int H, int W, int *TH_, int *TW_) {
    long best = -1;
    for (int TH = 1; TH <= H && TH <= C1M_PCAP; ++TH) {
        int TWmax = std::min(W, C1M_PCAP / TH);
        for (int TW = std::max(1, TWmax - 40); TW <= TWmax; ++TW) {
            const long tiles = (long)((H + TH - 1) / TH) * ((W + TW - 1) / TW);
            const long cost = tiles * ((TH * TW + 31) / 32);
            if (best < 0 || cost < best) { best = cost; *TH_ = TH; *TW_ = TW; }
        }
    }
}

static int launch_conv1_mfma(const ConvOp &c, const Conv1Params &cp, hipStream_t st) {
    int TH1 = 1, TW1 = 1;
    choose_tile1(cp.H, cp.W, &TH1, &TW1);
    const int th = (cp.H + TH1 - 1) / TH1, twn = (cp.W + TW1 - 1) / TW1;
    const size_t lds = (size_t)2 * C1M_PCAP * 4 + (size_t)4 * 32 * HX_TPITCH * 4 +
                       (size_t)(TH1 + c.kh - 1) * (TW1 + c.kw - 1) * 4;
    const unsigned grid = (unsigned)std::min<size_t>((size_t)cp.B * th * twn, 256 * 8);
    return amt_dispatch(ConvKernelSizes{}, c.kh, c.kw, [&](auto KH, auto KW) {
        return amt_launch<conv1_mfma_kernel<KH(), KW()>>(0, grid, 256, lds, st, cp, TH1, TW1, th, twn);
    });
}
static int launch_conv1(const ConvOp &c, const Conv1Params &cp, hipStream_t st) {
    const int groups = 256 / c.cout;
    const size_t lds = ((size_t)c.kh * c.kw * c.cout +
                        (size_t)c.kh * (groups * C1_PPT + c.kw - 1)) * 4;
    const size_t tiles = (size_t)cp.B * cp.H * ((cp.W + groups * C1_PPT - 1) / (groups * C1_PPT));
    conv1_kernel<<<(unsigned)std::min<size_t>(tiles, 8192), 256, lds, st>>>(cp);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

// ---- which implementation runs a layer ------------------------------------------------------------------------------
// THE decision: the forward walk switches on it, and what else depends on the implementation (who forms a rank-1
// shortcut, who measures its output, who needs frequency tensors in the workspace) is derived from it below.
// Fall-backs: a variant that is not built for the layer (null weights / no FFT-domain layer) hands down to the next.
enum ConvImpl {
    IMPL_FIRST_MFMA,           // first layer (Cin = 1) on the matrix pipe, 32 filters
    IMPL_FIRST_VALU,           // first layer, any other filter count or kernel size
    IMPL_FFT_ROW,              // mode 3: 576-point row form
    IMPL_FFT_PACKED,           // mode 3: 1152-point packed-image form
    IMPL_F16X3,                // mode >= 2: split-fp16
    IMPL_BF16X6,               // mode >= 1: split-bf16
    IMPL_F32                   // f32 MFMA
};
static ConvImpl conv_impl(const ConvOp &c, int mode) {
    if (c.cin == 1) return (c.cout == 32 && conv_supported(c.kh, c.kw)) ? IMPL_FIRST_MFMA : IMPL_FIRST_VALU;
    if (mode == 3 && c.fc.row) return IMPL_FFT_ROW;
    if (mode == 3 && c.fc.pk) return IMPL_FFT_PACKED;
    if (mode >= 2 && c.f16.w) return IMPL_F16X3;
    if (mode >= 1 && c.bf16.w) return IMPL_BF16X6;
    return IMPL_F32;
}
static bool impl_is_fft(ConvImpl impl) { return impl == IMPL_FFT_ROW || impl == IMPL_FFT_PACKED; }
// the epilogue can form a 1 x 1 projection of the one-channel network input itself (ConvParams::sc1, FcEpilogue::sc1)
static bool impl_forms_rank1_shortcut(ConvImpl impl, const ConvOp &c) {
    return impl == IMPL_FFT_ROW || (impl == IMPL_F16X3 && (!c.f16.masked || c.f16.wm_ms > 0));
}
// ... and does so for this projection: 1 x 1 kernel on the unpooled one-channel input
static bool shortcut_is_rank1(ConvImpl impl, const ConvOp &c, const ProjOp &pr) {
    return impl_forms_rank1_shortcut(impl, c) && pr.cin == 1 && pr.ph == 1 && pr.pw == 1 && pr.w;
}
// the kernel leaves max |output| per window for the split-fp16 scaling of its consumer
static bool impl_writes_amax(ConvImpl impl) {
    return impl == IMPL_FIRST_MFMA || impl_is_fft(impl) || impl == IMPL_F16X3;
}

// ---- weight packers: Keras-layout kernel [tap][cin][cout] -> the variant's layout, on the host ----------------------
// f32 MFMA: [slice][cchunk][tap][c][j][ntw], cout = slice*cw + 32*ntw + j
static std::vector<float> pack_f32(const float *kern, int ntap, int C, int fo, int nslice) {
    const int nch = C / 32, cw = fo / nslice, NTW = cw / 32;
    std::vector<float> wa((size_t)ntap * C * fo);
    for (int sl = 0; sl < nslice; ++sl)
        for (int ch = 0; ch < nch; ++ch)
            for (int tap = 0; tap < ntap; ++tap)
                for (int cc = 0; cc < 32; ++cc)
                    for (int j = 0; j < 32; ++j)
                        for (int nt = 0; nt < NTW; ++nt)
                            wa[(((((size_t)sl * nch + ch) * ntap + tap) * 32 + cc) * 32 + j) * NTW + nt] =
                                kern[((size_t)tap * C + ch * 32 + cc) * fo + sl * cw + nt * 32 + j];
    return wa;
}
// split-bf16: [slice][chunk16][slab][tt][plane][nt][h][col][8] bf16
static std::vector<unsigned short> pack_bf16x6(const float *kern, int ntap, int C, int fo, int nslice16) {
    const int NT = fo / 32, cw16 = fo / nslice16, NT16 = cw16 / 32;
    const int tps = (NT16 == 1 && ntap % 2 == 0) ? 2 : 1;
    const int nslab = ntap / tps;
    const int nch16 = C / BX_CC;
    std::vector<unsigned short> w16((size_t)nch16 * ntap * 3 * NT * 2 * 32 * 8);
    for (int sl = 0; sl < nslice16; ++sl)
        for (int ch = 0; ch < nch16; ++ch)
            for (int sb = 0; sb < nslab; ++sb)
                for (int tt = 0; tt < tps; ++tt)
                    for (int nt = 0; nt < NT16; ++nt)
                        for (int h = 0; h < 2; ++h)
                            for (int col = 0; col < 32; ++col)
                                for (int jj = 0; jj < 8; ++jj) {
                                    const int tap = sb * tps + tt;
                                    const int cin_i = ch * BX_CC + 8 * h + jj;
                                    const float wv = kern[((size_t)tap * C + cin_i) * fo + sl * cw16 + nt * 32 + col];
                                    unsigned short hh[3];
                                    amt_split3(wv, hh[0], hh[1], hh[2]);
                                    for (int pl = 0; pl < 3; ++pl) {
                                        const size_t idx =
                                            ((((((((size_t)sl * nch16 + ch) * nslab + sb) * tps + tt) * 3 + pl) * NT16 + nt) * 2 + h) * 32 + col) * 8 + jj;
                                        w16[idx] = hh[pl];
                                    }
                                }
    return w16;
}
// split-fp16, weights scaled by wscale: the layout of hx_weight_at (amt_conv_f16x3.h)
static std::vector<unsigned short> pack_f16x3(const float *kern, int ntap, int C, int fo, float wscale) {
    const int nsliceh = fo / 32, nch16 = C / BX_CC, ntp = ntap / 2;
    std::vector<unsigned short> ws((size_t)ntap * C * fo * 2);
    for (int sl = 0; sl < nsliceh; ++sl)
        for (int ch = 0; ch < nch16; ++ch)
            for (int tp = 0; tp < ntp; ++tp)
                for (int ns = 0; ns < 2; ++ns)
                    for (int ln = 0; ln < 64; ++ln)
                        for (int jj = 0; jj < 8; ++jj) {
                            const HxWeightAt at = hx_weight_at(nch16, ntp, sl, ch, tp, 0, ns, ln, jj);
                            unsigned short hh[2];
                            amt_split_f16<true>(kern[((size_t)at.tap * C + at.cin) * fo + at.cout] * wscale, hh[0], hh[1]);
                            for (int pl = 0; pl < 2; ++pl) ws[hx_weight_at(nch16, ntp, sl, ch, tp, pl, ns, ln, jj).idx] = hh[pl];
                        }
    return ws;
}

// The matrix-pipe variants of one layer (Cin >= 32): plan and weights of the f32 MFMA kernel (always), of the split-bf16
// kernel (where its tile efficiency pays) and of the split-fp16 kernel (where a tile fits and the weights are finite)
static int build_conv_variants(amt_rdcnn *n, ConvOp &c, const float *kern) {
    const int C = c.cin, fo = c.cout, H = c.H, W = c.W, kh = c.kh, kw = c.kw, ntap = kh * kw;
    if (C % 32 || fo % 32 || !conv_supported(kh, kw) || !conv_channels_supported(C, fo)) return AMT_E_UNSUPPORTED;
    if ((kh == 4 && kw == 16 && C == 32 && fo == 32 && W + 15 <= 576 && H <= 20) ||
        (kh == 4 && kw == 16 && C == 64 && fo == 64 && W == 64 && H == 10))
        c.k_host.assign(kern, kern + (size_t)ntap * C * fo);      // FFT-domain forms, built on demand (mode 3)
    int rc;
    // small late-stage layers (few output positions per window) cannot fill 256 CUs with
    // position tiles alone: compute them in 32-channel output slices (blockIdx.y)
    c.f32.nslice = (fo >= 128 && H * W <= 128) ? fo / 32 : 1;
    c.f32.cw = fo / c.f32.nslice;
    const std::vector<float> wa = pack_f32(kern, ntap, C, fo, c.f32.nslice);
    if ((rc = upload(n, wa.data(), wa.size() * sizeof(float), &c.f32.w)) != AMT_OK) return rc;
    choose_tile(c);
    if (c.f32.TH == 0) return AMT_E_UNSUPPORTED;

    c.bf16.nslice = fo > 64 ? fo / 64 : 1;                // 128 couts run as two 64-wide slices
    c.bf16.cw = fo / c.bf16.nslice;
    choose_tile16(c);
    // worth it only if 2.67x fewer matrix cycles survive the tile efficiency
    if (c.bf16.TH > 0 && c.bf16.eff * 2.67 > c.f32.eff * 1.15) {
        const std::vector<unsigned short> w16 = pack_bf16x6(kern, ntap, C, fo, c.bf16.nslice);
        if ((rc = upload(n, w16.data(), w16.size() * 2, &c.bf16.w)) != AMT_OK) return rc;
    }

    c.f16.cw = 32; c.f16.nslice = fo / 32;                // 32-wide N-slices
    choose_tile_h(c);
    choose_tile_w(c);
    float wmax = 0.f;
    bool finite = true;
    for (size_t q = 0; q < (size_t)ntap * C * fo; ++q) {
        if (!std::isfinite(kern[q])) finite = false;
        wmax = std::max(wmax, fabsf(kern[q]));
    }
    if (c.f16.TH > 0 && finite && wmax > 0.f) {
        c.sw = hx_weight_shift(wmax);
        const std::vector<unsigned short> ws = pack_f16x3(kern, ntap, C, fo, ldexpf(1.0f, c.sw));
        if ((rc = upload(n, ws.data(), ws.size() * 2, &c.f16.w)) != AMT_OK) return rc;
    }
    return AMT_OK;
}

// layer tap (amt_rdcnn_layer_tap): n floats per window from src (window stride `stride`) into the dense dst
__global__ __launch_bounds__(256) void tap_copy_kernel(const float *__restrict__ src, size_t stride, float *__restrict__ dst,
                                                       size_t n) {
    const float *s = src + (size_t)blockIdx.y * stride;
    float *o = dst + (size_t)blockIdx.y * n;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) o[i] = s[i];
}

extern "C" {

size_t amt_rdcnn_param_count(const amt_rdcnn_desc *desc) {
    RdTopology tp;
    return desc && amt_rdcnn_topology(*desc, &tp) == AMT_OK ? tp.total : 0;
}

int amt_rdcnn_destroy(amt_rdcnn *net) {
    if (!net) return AMT_OK;
    for (const ProfPending &pp : net->prof_pending) { (void)hipEventDestroy(pp.e0); (void)hipEventDestroy(pp.e1); }
    for (hipEvent_t e : net->prof_free) (void)hipEventDestroy(e);
    for (void *p : net->allocs) (void)hipFree(p);
    for (Tower &t : net->towers)
        for (ConvOp &c : t.convs)
        {
            if (c.fc.row) amt_fftconv_layer_destroy_internal(c.fc.row);
            if (c.fc.pk) amt_fftpk_layer_destroy_internal(c.fc.pk);
        }
    delete net;
    return AMT_OK;
}

int amt_rdcnn_create(amt_rdcnn **out, const amt_rdcnn_desc *desc, const float *wh, size_t n_floats) {
    if (!out || !desc || !wh) return AMT_E_INVALID;
    const amt_rdcnn_desc &d = *desc;
    if (d.n_towers < 1 || d.n_towers > 2 || d.conv_layers < 1 || d.dense_units < 1 ||
        d.output_classes < 1)
        return AMT_E_INVALID;
    RdTopology tp;
    if (amt_rdcnn_topology(d, &tp) != AMT_OK) return AMT_E_UNSUPPORTED;
    if (tp.total != n_floats) return AMT_E_SHAPE;
    if (!tp.shortcut_ok) return AMT_E_UNSUPPORTED;
    amt_rdcnn *n = new amt_rdcnn();
    n->d = d;
    n->fc_pooled = amt_env_switch("AMT_FC_POOLED", true);
    n->flat = tp.flat;
    n->towers.resize(d.n_towers);
    for (int t = 0; t < d.n_towers; ++t) {
        Tower &tw = n->towers[t];
        tw.in_h = d.in_h[t]; tw.in_w = d.in_w[t]; tw.ph = d.pool_h[t]; tw.pw = d.pool_w[t];
        tw.max_act = (size_t)tw.in_h * tw.in_w;
        tw.out_h = tp.out_h[t]; tw.out_w = tp.out_w[t]; tw.out_c = tp.out_c[t];
    }
    int rc = AMT_OK;
#define RD_TRY(x) do { rc = (x); if (rc != AMT_OK) { amt_rdcnn_destroy(n); return rc; } } while (0)
    for (const RdLayer &l : tp.layers) {
        Tower &tw = n->towers[l.tower];
        ConvOp c;
        c.cin = l.cin; c.cout = l.cout; c.H = l.H; c.W = l.W; c.kh = l.kh; c.kw = l.kw;
        const float *kern = wh + l.kernel;
        RD_TRY(upload_folded_bn(n, wh + l.bn, l.cout, wh + l.bias, &c.s1, &c.t1));
        if (l.cin == 1) RD_TRY(upload(n, kern, (size_t)l.kh * l.kw * l.cout * sizeof(float), &c.f32.w));      // [tap][cout] as is
        else RD_TRY(build_conv_variants(n, c, kern));
        n->flops += 2.0 * l.H * l.W * (double)l.kh * l.kw * l.cin * l.cout;
        tw.max_act = std::max(tw.max_act, (size_t)l.H * l.W * l.cout);
        c.residual = l.residual;
        if (l.residual && l.sc_bn) {
            ProjOp pr;
            pr.cin = l.sC; pr.cout = l.cout; pr.H = l.sH; pr.W = l.sW;
            pr.ph = l.sc_ph; pr.pw = l.sc_pw; pr.HO = l.H; pr.WO = l.W;      // valid avg-pool output (shortcut_ok)
            RD_TRY(upload_folded_bn(n, wh + l.sc_bnorm, l.cout, l.sc_proj ? wh + l.sc_bias : nullptr, &pr.s, &pr.t));
            if (l.sc_proj) RD_TRY(upload(n, wh + l.sc_kernel, (size_t)l.sC * l.cout * sizeof(float), &pr.w));
            n->flops += 2.0 * l.H * l.W * (double)l.sC * l.cout;
            c.sc_proj = (int)tw.projs.size();
            tw.projs.push_back(pr);
        }
        if (l.residual) RD_TRY(upload_folded_bn(n, wh + l.res_bn, l.cout, nullptr, &c.s2, &c.t2));
        c.pool_after = l.pool_after ? 1 : 0;
        tw.convs.push_back(c);
    }
    RD_TRY(upload(n, wh + tp.d1_kernel, (size_t)tp.flat * d.dense_units * sizeof(float), &n->d1w));
    RD_TRY(upload(n, wh + tp.d1_bias, (size_t)d.dense_units * sizeof(float), &n->d1b));
    RD_TRY(upload(n, wh + tp.d2_kernel, (size_t)d.dense_units * d.output_classes * sizeof(float), &n->d2w));
    RD_TRY(upload(n, wh + tp.d2_bias, (size_t)d.output_classes * sizeof(float), &n->d2b));
    n->flops += 2.0 * tp.flat * d.dense_units + 2.0 * d.dense_units * d.output_classes;
#undef RD_TRY
    *out = n;
    return AMT_OK;
}

double amt_rdcnn_flops_per_window(const amt_rdcnn *net) { return net ? net->flops : 0.0; }

int amt_rdcnn_set_mode(amt_rdcnn *net, int mode) {
    if (!net || mode < 0 || mode > 3) return AMT_E_INVALID;
    if (mode == 3) {
        // FFT-domain form of the 32 -> 32 (4 x 16) layers (every other layer runs the split-fp16 kernels of mode 2):
        // the transformed kernel matrices are computed on the host in float64, once
        for (Tower &t : net->towers)
            for (ConvOp &c : t.convs)
                if (!c.fc && !c.k_host.empty()) {
                    const int rc = c.cin == 64 ? amt_fftpk_layer_create_internal(&c.fc.pk, c.k_host.data())
                                               : amt_fftconv_layer_create_internal(&c.fc.row, c.k_host.data());
                    if (rc != AMT_OK) return rc;
                    c.fc.H = c.H; c.fc.W = c.W;
                }
    }
    net->mode = mode;
    return AMT_OK;
}

// Diagnostic export (not in include/amt_saga.h; tests/test_gpu_pooled_epilogue.py): how many layers of the net take the
// W-pooled epilogue in its current mode (fc_wpooled_ok, below)
static bool fc_wpooled_ok(const amt_rdcnn *net, const Tower &tw, int i, ConvImpl impl, int H, int W);
int amt_rdcnn_fc_pooled_layers(const amt_rdcnn *net) {
    if (!net) return AMT_E_INVALID;
    int n = 0;
    for (const Tower &tw : net->towers)
        for (size_t i = 0; i < tw.convs.size(); ++i)
            n += fc_wpooled_ok(net, tw, (int)i, conv_impl(tw.convs[i], net->mode), tw.convs[i].H, tw.convs[i].W) ? 1 : 0;
    return n;
}

int amt_rdcnn_profile(amt_rdcnn *net, int enable) {
    if (!net) return AMT_E_INVALID;
    net->prof_on = enable != 0;
    if (net->prof_acc.empty()) {
        net->prof_acc.resize(net->towers.size());
        for (size_t t = 0; t < net->towers.size(); ++t) net->prof_acc[t].resize(net->towers[t].convs.size());
    }
    return AMT_OK;
}

int amt_rdcnn_profile_read(amt_rdcnn *net, int32_t *desc, double *ms, double *windows,
                           double *flops_per_window, int cap, int *n_rows, int reset) {
    if (!net || !n_rows) return AMT_E_INVALID;
    for (const ProfPending &pp : net->prof_pending) {
        AMT_HIP_CHECK(hipEventSynchronize(pp.e1));
        float e = 0.f;
        AMT_HIP_CHECK(hipEventElapsedTime(&e, pp.e0, pp.e1));
        ProfAcc &a = net->prof_acc[pp.tower][pp.layer];
        a.ms += e; a.windows += pp.windows; a.launches += 1;
        net->prof_free.push_back(pp.e0);
        net->prof_free.push_back(pp.e1);
    }
    net->prof_pending.clear();
    int r = 0;
    for (size_t t = 0; t < net->prof_acc.size(); ++t)
        for (size_t i = 0; i < net->prof_acc[t].size(); ++i) {
            if (r < cap && desc && ms && windows && flops_per_window) {
                const ConvOp &c = net->towers[t].convs[i];
                int32_t *d = desc + (size_t)r * 8;
                d[0] = (int)t; d[1] = (int)i + 1; d[2] = c.kh; d[3] = c.kw; d[4] = c.cin; d[5] = c.cout;
                d[6] = c.H; d[7] = c.W;
                ms[r] = net->prof_acc[t][i].ms;
                windows[r] = net->prof_acc[t][i].windows;
                flops_per_window[r] = 2.0 * c.H * c.W * (double)c.kh * c.kw * c.cin * c.cout;
            }
            ++r;
        }
    *n_rows = r;
    if (reset)
        for (auto &v : net->prof_acc) for (auto &a : v) a = ProfAcc();
    return AMT_OK;
}

// Diagnostic exports (not in include/amt_saga.h; tests/test_gpu_rdcnn_layers.py), bound in rdcnn.py like
// amt_rdcnn_fc_pooled_layers.
//
// The layer tap.  dst: device memory for the block output of conv layer `layer` (0-based) of `tower` -- after BN +
// sigmoid, after the shortcut add and its BN where a shortcut closes, before any max pool -- dense [B][H][W][cout]
// for the B of the forwards that follow; NULL takes the tap away.  While a tap is set amt_rdcnn_forward copies the
// layer's output there on its stream, right behind the layer's launches.  A mode-3 layer that leaves its W-pooled pair
// in place of its output (amt_rdcnn_fc_plan: wpooled) is tapped as that pair: dst is dense [2][B][H][W / 8][cout], the
// 8-column means (wavg) first, then the 8-column maxima (wmax).  A mode-3 layer with neither -- the next layer reads it
// transformed and nothing else reads it (hands_on && !writes_spatial) -- cannot be tapped: the forward answers
// AMT_E_UNSUPPORTED before it launches that layer and computes what it always computes otherwise.  Without taps the
// forward launches exactly what it launches without this export.
int amt_rdcnn_layer_tap(amt_rdcnn *net, int tower, int layer, float *dst) {
    if (!net || tower < 0 || tower >= (int)net->towers.size()) return AMT_E_INVALID;
    if (layer < 0 || layer >= (int)net->towers[tower].convs.size()) return AMT_E_INVALID;
    if (net->taps.empty()) {
        if (!dst) return AMT_OK;
        net->taps.resize(net->towers.size());
        for (size_t t = 0; t < net->towers.size(); ++t) net->taps[t].assign(net->towers[t].convs.size(), nullptr);
    }
    net->taps[tower][layer] = dst;
    return AMT_OK;
}

// The plan report: what amt_rdcnn_forward runs for conv layer `layer` (0-based) of `tower` in `mode`, as
// AMT_RDCNN_PLAN_INTS ints: ConvImpl, kh, kw, cin, cout, H, W, slice width, TH, TW, NWIN, masked, wm_ms, nslice, MT.
// Slice width, tile and slices are the running variant's (the window-major form: whole images of HXW_WIN windows; the
// matrix-pipe first layer: its TH x TW tile; zero where the implementation has none).  MT is the f32 MFMA kernel's
// M-tiles per wave, 0 for every other implementation.  Host only, reads the net and changes nothing.  (Mode 3 reports
// an FFT-domain form only once amt_rdcnn_set_mode(net, 3) has built it.)
#define AMT_RDCNN_PLAN_INTS 15
int amt_rdcnn_layer_plan(const amt_rdcnn *net, int tower, int layer, int mode, int32_t *out) {
    if (!net || !out || mode < 0 || mode > 3 || tower < 0 || tower >= (int)net->towers.size()) return AMT_E_INVALID;
    if (layer < 0 || layer >= (int)net->towers[tower].convs.size()) return AMT_E_INVALID;
    const ConvOp &c = net->towers[tower].convs[layer];
    const ConvImpl impl = conv_impl(c, mode);
    int cw = 0, TH = 0, TW = 0, NWIN = 0, masked = 0, wm_ms = 0, nslice = 0, MT = 0;
    auto from_plan = [&](const ConvPlan &p) {
        cw = p.cw; TH = p.TH; TW = p.TW; NWIN = p.NWIN; masked = p.masked ? 1 : 0; nslice = p.nslice;
    };
    switch (impl) {
    case IMPL_FIRST_MFMA: cw = c.cout; nslice = 1; NWIN = 1; choose_tile1(c.H, c.W, &TH, &TW); break;
    case IMPL_F16X3:
        from_plan(c.f16);
        wm_ms = c.f16.wm_ms;
        if (wm_ms > 0) { TH = c.H; TW = c.W; NWIN = HXW_WIN; }
        break;
    case IMPL_BF16X6: from_plan(c.bf16); break;
    case IMPL_F32: from_plan(c.f32); MT = c.MT; break;
    default: break;
    }
    const int32_t v[AMT_RDCNN_PLAN_INTS] = {(int32_t)impl, c.kh, c.kw, c.cin, c.cout, c.H, c.W, cw, TH, TW, NWIN, masked, wm_ms, nslice, MT};
    std::copy(v, v + AMT_RDCNN_PLAN_INTS, out);
    return AMT_OK;
}

#define RD_CHUNK 1024          // windows per pass through the network

// ---- workspace: THE layout, in floats from the workspace base --------------------------------------------------------
struct WsLayout {
    size_t act;                // floats per window of an activation buffer
    size_t buf[4];             // activation buffers (ping-pong, shortcut source, projected shortcut)
    size_t flat, dense, logits;
    size_t amax;               // [conv_layers + 1][Bc] max |activation| per window: the network input and every conv
                               // layer's output (split-fp16 scaling)
    size_t Xf, Yf, amaxf;      // mode 3: two frequency tensors (16-byte aligned) + per-window max |Xf|
    size_t total;
};
// base: the workspace the offsets will be applied to (only its 16-byte misalignment matters; the total does not
// depend on it -- the 8 floats in front of Xf cover the round-up)
static WsLayout ws_layout(const amt_rdcnn *n, int Bc, const void *base = nullptr) {
    auto up4 = [](size_t v) { return (v + 3) & ~(size_t)3; };
    WsLayout l;
    l.act = 0;
    for (const Tower &t : n->towers) l.act = std::max(l.act, t.max_act);
    l.act = up4(l.act);
    for (int i = 0; i < 4; ++i) l.buf[i] = (size_t)i * Bc * l.act;
    l.flat = (size_t)4 * Bc * l.act;
    l.dense = l.flat + (size_t)Bc * up4(n->flat);
    l.logits = l.dense + (size_t)Bc * up4(n->d.dense_units);
    l.amax = l.logits + (size_t)Bc * up4(n->d.output_classes);
    l.Xf = l.amax + (size_t)(n->d.conv_layers + 1) * Bc + 8;
    l.total = l.Xf;
    l.Xf += ((16 - (reinterpret_cast<uintptr_t>(base) + l.Xf * sizeof(float)) % 16) % 16) / sizeof(float);
    size_t freq = 0;                                     // the largest frequency tensor of the net
    for (const Tower &t : n->towers)
        for (const ConvOp &c : t.convs)
            if (impl_is_fft(conv_impl(c, n->mode))) freq = std::max(freq, fc_freq_floats(c.fc, Bc));
    l.Yf = l.Xf + freq;
    l.amaxf = l.Yf + freq;
    if (freq) l.total += 2 * freq + (size_t)Bc + 8;
    return l;
}

size_t amt_rdcnn_workspace_bytes(const amt_rdcnn *net, int B) {
    if (!net || B <= 0) return 0;
    return ws_layout(net, std::min(B, RD_CHUNK)).total * sizeof(float);
}

static int grid_for(size_t total) {
    size_t g = (total + 255) / 256;
    return (int)std::min<size_t>(g, 65536);
}
static int launch_absmax(const float *x, size_t n, size_t stride, int B, float *amax, hipStream_t st) {
    absmax_kernel<<<dim3((unsigned)std::min<size_t>((n + 1023) / 1024, 64), B), 256, 0, st>>>(x, n, stride, amax);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

// ---- per-layer event profiler (amt_rdcnn_profile): a begin and an end around a layer's launches ----------------------
static int prof_begin(const amt_rdcnn *net, ProfPending &pp, hipStream_t st) {
    if (!net->prof_on) return AMT_OK;
    for (hipEvent_t *pe : {&pp.e0, &pp.e1}) {
        if (!net->prof_free.empty()) { *pe = net->prof_free.back(); net->prof_free.pop_back(); }
        else AMT_HIP_CHECK(hipEventCreate(pe));
    }
    AMT_HIP_CHECK(hipEventRecord(pp.e0, st));
    return AMT_OK;
}
static int prof_end(const amt_rdcnn *net, const ProfPending &pp, hipStream_t st) {
    if (!net->prof_on) return AMT_OK;
    AMT_HIP_CHECK(hipEventRecord(pp.e1, st));
    net->prof_pending.push_back(pp);
    return AMT_OK;
}

// FFT-domain form, either kind: [forward transform of the spatial input, unless the previous layer left its output
// transformed in Xf] -> per-frequency GEMM -> inverse + epilogue [+ forward transform for the next such layer]; the
// spatial output is written only where something reads it (a later shortcut, a pooling, a layer of another kind)
struct FcBufs { float *Xf, *Yf, *amaxf; };
// The W-pooled epilogue (FcEpilogue::wmax / wavg, EPI = 5 of both row kernels) in place of layer i's full-size output.
// THE rule: an FFT-form layer (row or packed) that adds a shortcut TENSOR (the block's input or its projection; not the
// rank-1 form), a max pool (ph, 8) behind it, and no reader of its output that the pooled pair cannot serve.  The
// readers are that max pool -- from wmax, with (ph, 1) -- and at most the next closing layer's projected shortcut, whose
// source is this output: it is served from wavg with (sc_ph, 1) only if its average pool spans the max pool's 8 columns.
// That is not automatic: a 6 x 20 image pooled (2, 8) gives a shortcut pool of (3, 10).  (Rows are not pooled by the
// epilogue, so the shortcut's row count is free: 3 x 17 gives (3, 8) against (2, 8).)
static bool fc_wpooled_ok(const amt_rdcnn *net, const Tower &tw, int i, ConvImpl impl, int H, int W) {
    const ConvOp &c = tw.convs[i];
    if (!net->fc_pooled || !impl_is_fft(impl) || !c.pool_after || tw.pw != 8 || W < 8) return false;
    if (!c.residual || (c.sc_proj >= 0 && shortcut_is_rank1(impl, c, tw.projs[c.sc_proj]))) return false;
    for (size_t j = (size_t)i + 1; j < tw.convs.size(); ++j) {
        const ConvOp &r = tw.convs[j];
        if (!r.residual) continue;
        if (r.sc_proj < 0) return false;
        const ProjOp &pr = tw.projs[r.sc_proj];
        return pr.H == H && pr.W == W && pr.cin == c.cout && pr.pw == 8 && pr.WO == W / 8;
    }
    return true;
}
// THE form of one layer's step: what amt_rdcnn_forward launches for conv layer i of a tower in `mode`, decided here and
// nowhere else (amt_rdcnn_fc_plan reports the same struct).  H x W: the layer's image.
struct LayerForm {
    ConvImpl impl;
    bool last_op;              // the output goes into the tower's part of the dense input (stride: the flat row)
    const ProjOp *rank1;       // shortcut: a 1 x 1 projection of the one-channel input, formed in the epilogue
    const ProjOp *proj;        // shortcut: a tensor made by proj_kernel (neither: the block's input as is, where one closes)
    // FFT-domain forms only (false elsewhere, need_sp true)
    bool have_xf;              // the previous layer left this one's input transformed in Xf: no forward transform
    bool next_fc;              // hands its output on transformed (Xf_next) to a next layer of its kind
    bool wpooled;              // leaves the W-pooled pair in place of its output (fc_wpooled_ok)
    bool need_sp;              // writes its spatial output
};
static bool fc_hands_on(const Tower &tw, int i, int mode) {
    const ConvOp &c = tw.convs[i];
    const ConvImpl impl = conv_impl(c, mode);
    return impl_is_fft(impl) && i + 1 < (int)tw.convs.size() && !c.pool_after && conv_impl(tw.convs[i + 1], mode) == impl;
}
static LayerForm layer_form(const amt_rdcnn *net, const Tower &tw, int i, int mode, int H, int W) {
    const ConvOp &c = tw.convs[i];
    LayerForm f{};
    f.impl = conv_impl(c, mode);
    f.last_op = (i == (int)tw.convs.size() - 1) && !c.pool_after;
    if (c.residual && c.sc_proj >= 0) {
        const ProjOp &pr = tw.projs[c.sc_proj];
        (shortcut_is_rank1(f.impl, c, pr) ? f.rank1 : f.proj) = &pr;
    }
    const bool fft = impl_is_fft(f.impl);
    f.have_xf = fft && i > 0 && fc_hands_on(tw, i - 1, mode);
    f.next_fc = fft && fc_hands_on(tw, i, mode);
    f.wpooled = fc_wpooled_ok(net, tw, i, f.impl, H, W);
    // the spatial output is written only where something reads it: a later shortcut, a pooling, a layer of another kind
    f.need_sp = !fft || (!f.wpooled && (!f.next_fc || c.residual));
    return f;
}

// Diagnostic export (not in include/amt_saga.h; tests/test_gpu_rdcnn_fft_layers.py), bound in rdcnn.py next to
// amt_rdcnn_layer_plan: the FFT-domain form of conv layer `layer` (0-based) of `tower` in `mode`, from layer_form -- the
// function the forward itself asks -- as 8 ints: form (0 none, 1 row, 2 packed), have_xf, hands_on (writes Xf_next),
// writes_spatial, shortcut kind (0 none, 1 tensor as is, 2 tensor through proj_kernel, 3 rank-1), wpooled,
// out_is_flat_row, GEMM chunks per workgroup for a forward of B windows (amt_fftconv_gemm; 1 for the packed form, whose
// persistent grid has no such figure; B <= 0: a full pass of RD_CHUNK windows).  Host only, reads the net.  A layer that
// is no FFT-domain form reports form 0 and its shortcut kind, spatial output and flat row all the same.  (Like
// amt_rdcnn_layer_plan, mode 3 reports an FFT-domain form only once amt_rdcnn_set_mode(net, 3) has built it.)
int amt_rdcnn_fc_plan(const amt_rdcnn *net, int tower, int layer, int mode, int B, int32_t *out) {
    if (!net || !out || mode < 0 || mode > 3 || tower < 0 || tower >= (int)net->towers.size()) return AMT_E_INVALID;
    if (layer < 0 || layer >= (int)net->towers[tower].convs.size()) return AMT_E_INVALID;
    const Tower &tw = net->towers[tower];
    const ConvOp &c = tw.convs[layer];
    const LayerForm f = layer_form(net, tw, layer, mode, c.H, c.W);
    const int form = f.impl == IMPL_FFT_ROW ? 1 : f.impl == IMPL_FFT_PACKED ? 2 : 0;
    const int Bc = B <= 0 ? RD_CHUNK : std::min(B, RD_CHUNK);
    out[0] = form;
    out[1] = f.have_xf;
    out[2] = f.next_fc;
    out[3] = f.need_sp;
    out[4] = !c.residual ? 0 : f.rank1 ? 3 : f.proj ? 2 : 1;
    out[5] = f.wpooled;
    out[6] = f.last_op;
    out[7] = form == 1 ? amt_fftconv_gemm_chunks_per_wg(Bc) : form == 2 ? 1 : 0;
    return AMT_OK;
}

static int run_fc(const ConvOp &c, const float *in, size_t in_stride, const LayerForm &f, int Bc, const FcEpilogue &ep,
                  const FcBufs &b, float *o, size_t o_stride, float *amax_o, hipStream_t st) {
    int rc = AMT_OK;
    if (!f.have_xf) rc = fc_forward_fft(c.fc, in, in_stride, Bc, b.Xf, b.amaxf, st);
    if (rc == AMT_OK) rc = fc_gemm(c.fc, b.Xf, b.amaxf, Bc, b.Yf, st);
    if (rc != AMT_OK) return rc;
    return fc_inverse_epilogue(c.fc, b.Yf, ep, Bc, f.need_sp ? o : nullptr, o_stride, f.next_fc ? b.Xf : nullptr, b.amaxf,
                               f.next_fc ? nullptr : amax_o, st);
}

int amt_rdcnn_forward(const amt_rdcnn *net, const float *const *x, int B, float *y, float *logits,
                      void *workspace, size_t workspace_bytes, void *stream) {
    if (!net || !x || !y || !workspace || B <= 0) return AMT_E_INVALID;
    const amt_rdcnn_desc &d = net->d;
    for (int t = 0; t < d.n_towers; ++t) if (!x[t]) return AMT_E_INVALID;
    if (workspace_bytes < amt_rdcnn_workspace_bytes(net, B)) return AMT_E_NOMEM;
    hipStream_t st = (hipStream_t)stream;
    const int K = d.output_classes, DU = d.dense_units, flat = net->flat, mode = net->mode;
#define RD_TRY(x) do { const int rc_ = (x); if (rc_ != AMT_OK) return rc_; } while (0)

    for (int b0 = 0; b0 < B; b0 += RD_CHUNK) {
        const int Bc = std::min(RD_CHUNK, B - b0);
        float *ws = static_cast<float *>(workspace);
        const WsLayout lay = ws_layout(net, Bc, workspace);
        float *buf[4];
        for (int i = 0; i < 4; ++i) buf[i] = ws + lay.buf[i];
        float *flatbuf = ws + lay.flat, *d1 = ws + lay.dense, *lg = ws + lay.logits;
        // split-fp16 scaling: layer i reads amax row i (its input) and leaves row i + 1 (its output)
        auto amax_row = [&](int i) { return ws + lay.amax + (size_t)i * Bc; };
        const FcBufs fcb{ws + lay.Xf, ws + lay.Yf, ws + lay.amaxf};
        int flat_off = 0;
        for (int t = 0; t < d.n_towers; ++t) {
            const Tower &tw = net->towers[t];
            const float *cur = x[t] + (size_t)b0 * tw.in_h * tw.in_w;
            size_t cur_stride = (size_t)tw.in_h * tw.in_w;
            if (mode >= 2) {
                AMT_HIP_CHECK(hipMemsetAsync(amax_row(0), 0, (size_t)(d.conv_layers + 1) * Bc * sizeof(float), st));
                RD_TRY(launch_absmax(cur, cur_stride, cur_stride, Bc, amax_row(0), st));
            }
            const float *p0 = cur; size_t p0_stride = cur_stride;
            bool p0_wpooled = false;                     // p0 is the W-pooled average of a layer's output (fc_wpooled_ok)
            int H = tw.in_h, W = tw.in_w;
            const int L = (int)tw.convs.size();
            auto pick = [&](const float *a, const float *b_, const float *c_) -> float * {
                for (int i = 0; i < 4; ++i)
                    if (buf[i] != a && buf[i] != b_ && buf[i] != c_) return buf[i];
                return nullptr;
            };
            for (int i = 0; i < L; ++i) {
                const ConvOp &c = tw.convs[i];
                const LayerForm form = layer_form(net, tw, i, mode, H, W);
                const ConvImpl impl = form.impl;
                const bool last_op = form.last_op, wpooled = form.wpooled;
                float *o = last_op ? flatbuf + flat_off : pick(cur, p0, nullptr);
                const size_t o_stride = last_op ? (size_t)flat : (size_t)H * W * c.cout;
                // shortcut: the block's input as is, its projection (a kernel of its own), or -- a 1 x 1 projection of
                // the one-channel network input -- formed in the consumer's epilogue (rank1)
                const float *sc = nullptr; size_t sc_stride = 0;
                const ProjOp *rank1 = form.rank1;
                if (form.proj) {
                    const ProjOp &pr = *form.proj;
                    float *sb = pick(cur, p0, o);
                    ProjParams pp{p0, p0_stride, sb, (size_t)pr.HO * pr.WO * pr.cout, pr.w, pr.s, pr.t,
                                  Bc, pr.H, pr.W, pr.cin, pr.cout, pr.ph, pr.pw, pr.HO, pr.WO};
                    if (p0_wpooled) { pp.W = pr.W / 8; pp.PW = 1; }      // 1 / (sc_ph * 1) x the epilogue's 0.125 = 1 / (sc_ph * 8)
                    proj_kernel<<<dim3((pr.WO + PJ_TW - 1) / PJ_TW, pr.HO, Bc), 256,
                                  (size_t)PJ_TW * pr.cin * sizeof(float), st>>>(pp);
                    sc = sb; sc_stride = (size_t)pr.HO * pr.WO * pr.cout;
                } else if (c.residual && !rank1) {
                    sc = p0; sc_stride = p0_stride;
                }
                const float *s2 = c.residual ? c.s2 : nullptr, *t2 = c.residual ? c.t2 : nullptr;
                float *amax_o = mode >= 2 ? amax_row(i + 1) : nullptr;
                // the pooled pair shares the layer's output buffer: [Bc] wavg, then [Bc] wmax (a quarter of it together)
                const size_t wp_stride = (size_t)H * (W / 8) * c.cout;
                float *const tap = net->taps.empty() ? nullptr : net->taps[t][i];
                if (tap && !form.need_sp && !wpooled) return AMT_E_UNSUPPORTED;      // handed on transformed only: nothing to copy
                ProfPending prof{nullptr, nullptr, t, i, Bc};
                RD_TRY(prof_begin(net, prof, st));
                switch (impl) {
                case IMPL_FIRST_MFMA:
                    RD_TRY(launch_conv1_mfma(c, Conv1Params{cur, cur_stride, o, o_stride, sc, sc_stride, static_cast<const float *>(c.f32.w),
                                                            c.s1, c.t1, s2, t2, Bc, H, W, c.kh, c.kw, c.cout, amax_o}, st));
                    break;
                case IMPL_FIRST_VALU:
                    RD_TRY(launch_conv1(c, Conv1Params{cur, cur_stride, o, o_stride, sc, sc_stride, static_cast<const float *>(c.f32.w),
                                                       c.s1, c.t1, s2, t2, Bc, H, W, c.kh, c.kw, c.cout}, st));
                    break;
                case IMPL_FFT_ROW:
                case IMPL_FFT_PACKED: {
                    FcEpilogue ep;
                    ep.s1 = c.s1; ep.t1 = c.t1; ep.s2 = s2; ep.t2 = t2;
                    if (rank1) { ep.sc1 = p0; ep.sc1_stride = p0_stride; ep.sc1_w = rank1->w; ep.sc1_s = rank1->s; ep.sc1_t = rank1->t; }
                    else { ep.sc = sc; ep.sc_stride = sc_stride; }
                    if (wpooled) { ep.wavg = o; ep.wmax = o + (size_t)Bc * wp_stride; ep.wp_stride = wp_stride; }
                    RD_TRY(run_fc(c, cur, cur_stride, form, Bc, ep, fcb, o, o_stride, amax_o, st));
                    break;
                }
                default: {
                    ConvParams cp{cur, cur_stride, o, o_stride, sc, sc_stride, static_cast<const float *>(c.f32.w), c.s1, c.t1, s2, t2,
                                  Bc, H, W, 0, 0, 1, 0, 0, c.cout};          // the launcher fills in its variant's tile
                    if (rank1) {
                        cp.sc1 = p0; cp.sc1_win_stride = p0_stride;
                        cp.sc1_w = rank1->w; cp.sc1_s = rank1->s; cp.sc1_t = rank1->t;
                    }
                    RD_TRY(impl == IMPL_F16X3    ? launch_convh(c, cp, amax_row(i), amax_o, st)
                           : impl == IMPL_BF16X6 ? launch_conv16(c, cp, st) : launch_conv(c, cp, st));
                }
                }
                if (amax_o && !impl_writes_amax(impl) && i + 1 < L)
                    // the producing kernel does not measure its output: one extra pass (layers the split-fp16
                    // kernel is not built for; none of the reference's head topologies)
                    RD_TRY(launch_absmax(o, (size_t)H * W * c.cout, o_stride, Bc, amax_o, st));
                RD_TRY(prof_end(net, prof, st));
                if (tap && wpooled) {
                    // the pair as the epilogue left it: dense [2][B][H][W / 8][cout], wavg then wmax, B the forward's
                    const size_t n = wp_stride;
                    for (int half = 0; half < 2; ++half)
                        tap_copy_kernel<<<dim3((unsigned)std::min<size_t>((n + 255) / 256, 64), Bc), 256, 0, st>>>(
                            o + (size_t)half * Bc * wp_stride, wp_stride, tap + ((size_t)half * B + b0) * n, n);
                    AMT_LAUNCH_CHECK();
                } else if (tap) {
                    const size_t n = (size_t)H * W * c.cout;      // o_stride is the flat row where this is the last layer
                    tap_copy_kernel<<<dim3((unsigned)std::min<size_t>((n + 255) / 256, 64), Bc), 256, 0, st>>>(
                        o, o_stride, tap + (size_t)b0 * n, n);
                    AMT_LAUNCH_CHECK();
                }
                if (c.residual) { p0 = o; p0_stride = wpooled ? wp_stride : o_stride; p0_wpooled = wpooled; }
                cur = o; cur_stride = o_stride;
                if (wpooled) { cur = o + (size_t)Bc * wp_stride; cur_stride = wp_stride; }
                if (c.pool_after) {
                    const int HO = H / tw.ph, WO = W / tw.pw;
                    const bool last = (i == L - 1);
                    float *po = last ? flatbuf + flat_off : pick(cur, p0, nullptr);
                    const size_t po_stride = last ? (size_t)flat : (size_t)HO * WO * c.cout;
                    maxpool_kernel<<<grid_for((size_t)Bc * HO * WO * c.cout / 4), 256, 0, st>>>(
                        cur, cur_stride, po, po_stride, Bc, H, wpooled ? W / 8 : W, c.cout, tw.ph, wpooled ? 1 : tw.pw, HO, WO);
                    cur = po; cur_stride = po_stride; H = HO; W = WO;
                }
            }
            flat_off += tw.out_h * tw.out_w * tw.out_c;
        }
        if (flat >= 2048 && lay.act >= (size_t)DN_KSPLIT * DU) {
            float *dpart = buf[0];                         // the activation buffers are dead by now
            dense_kernel<<<dim3((DU + 31) / 32, (Bc + 31) / 32, DN_KSPLIT), 256, 0, st>>>(
                flatbuf, flat, net->d1w, net->d1b, DU, d1, Bc, 1, dpart);
            dense_reduce_kernel<<<(unsigned)(((size_t)Bc * DU + 255) / 256), 256, 0, st>>>(
                dpart, DN_KSPLIT, net->d1b, DU, d1, Bc, 1);
        } else {
            dense_kernel<<<dim3((DU + 31) / 32, (Bc + 31) / 32), 256, 0, st>>>(
                flatbuf, flat, net->d1w, net->d1b, DU, d1, Bc, 1, nullptr);
        }
        dense_kernel<<<dim3((K + 31) / 32, (Bc + 31) / 32), 256, 0, st>>>(
            d1, DU, net->d2w, net->d2b, K, lg, Bc, 0, nullptr);
        head_output_kernel<<<(Bc + 63) / 64, 64, 0, st>>>(lg, y + (size_t)b0 * K, Bc, K, d.out_lo, d.out_hi);
        if (logits)
            AMT_HIP_CHECK(hipMemcpyAsync(logits + (size_t)b0 * K, lg, (size_t)Bc * K * sizeof(float),
                                         hipMemcpyDeviceToDevice, st));
        AMT_LAUNCH_CHECK();
    }
#undef RD_TRY
    return AMT_OK;
}

}  // extern "C"

// ---- trainer form of the split-fp16 kernels (amt_convh.h) --------------------------------------------------------
int amt_convh_plan_init(amt_convh_plan *pl, int kh, int kw, int cin, int cout, int H, int W) {
    if (!pl || !conv_supported(kh, kw)) return AMT_E_UNSUPPORTED;
    if (!in_list(F16Cins{}, cin) || cout < 32 || cout % 32 != 0 || H < 1 || W < 1) return AMT_E_UNSUPPORTED;
    ConvOp c;
    c.cin = cin; c.cout = cout; c.H = H; c.W = W; c.kh = kh; c.kw = kw;
    c.f16.cw = 32; c.f16.nslice = cout / 32;
    choose_tile_h(c);
    if (c.f16.TH <= 0) return AMT_E_UNSUPPORTED;
    pl->kh = kh; pl->kw = kw; pl->cin = cin; pl->cout = cout; pl->H = H; pl->W = W;
    pl->TH = c.f16.TH; pl->TW = c.f16.TW; pl->NWIN = c.f16.NWIN; pl->masked = c.f16.masked ? 1 : 0; pl->lds = c.f16.lds;
    return AMT_OK;
}
size_t amt_convh_packed_bytes(const amt_convh_plan *pl) {
    return (size_t)pl->kh * pl->kw * pl->cin * pl->cout * 2 /* planes */ * 2 /* bytes */;
}

__global__ __launch_bounds__(256) void convh_wmax_kernel(const amt_convh_pack_job *jobs) {
    __shared__ float red[16];
    const amt_convh_pack_job j = jobs[blockIdx.y];
    const size_t n = (size_t)j.ntap * j.Cin * j.Cout;
    float m = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = fmaxf(m, fabsf(j.w[i]));
    m = block_max(m, red);
    if (threadIdx.x == 0) atomicMax(reinterpret_cast<int *>(j.wmax), __float_as_int(m));
}
// one thread per (slice, chunk, tap pair, N-subtile, lane): eight channels x two planes = two 16-byte stores.  The
// layout is hx_weight_at's (amt_conv_f16x3.h; pack_f16x3 is the host's packer), spelled out here in 16-byte units:
// going through that function costs this kernel a register and two instructions
__global__ __launch_bounds__(256) void convh_pack_kernel(const amt_convh_pack_job *jobs) {
    const amt_convh_pack_job j = jobs[blockIdx.y];
    const float wmax = *j.wmax;
    int sw = 0;
    if (wmax > 0.f && wmax < 3.0e38f) sw = hx_weight_shift(wmax);
    if (blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x == 0) *j.sw = sw;
    const float wscale = ldexpf(1.0f, sw);
    const bool bwd = blockIdx.z == 1;
    uint4 *out = static_cast<uint4 *>(bwd ? j.packed_bwd : j.packed_fwd);
    if (!out) return;
    const int C = bwd ? j.Cout : j.Cin, fo = bwd ? j.Cin : j.Cout;          // channels of the convolution that runs
    const int nch16 = C / BX_CC, ntp = j.ntap / 2, nsl = fo / 32;
    const size_t total = (size_t)nsl * nch16 * ntp * 2 * 64;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (size_t)gridDim.x * 256) {
        const int ln = (int)(q & 63);
        size_t r = q >> 6;
        const int ns = (int)(r & 1); r >>= 1;
        const int tp = (int)(r % ntp); r /= ntp;
        const int ch = (int)(r % nch16);
        const int sl = (int)(r / nch16);
        const int col = ln & 15, kg = ln >> 4;
        const int tap = 2 * tp + (kg & 1);
        const int co = sl * 32 + ns * 16 + col;
        unsigned short h[2][8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const int ci = ch * BX_CC + 8 * (kg >> 1) + jj;
            const float wv = bwd ? j.w[((size_t)(j.ntap - 1 - tap) * j.Cin + co) * j.Cout + ci]
                                 : j.w[((size_t)tap * j.Cin + ci) * j.Cout + co];
            amt_split_f16<true>(wv * wscale, h[0][jj], h[1][jj]);
        }
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            uint4 pk;
            pk.x = h[pl][0] | ((unsigned)h[pl][1] << 16);
            pk.y = h[pl][2] | ((unsigned)h[pl][3] << 16);
            pk.z = h[pl][4] | ((unsigned)h[pl][5] << 16);
            pk.w = h[pl][6] | ((unsigned)h[pl][7] << 16);
            out[((((((size_t)sl * nch16 + ch) * ntp + tp) * 2 + pl) * 2 + ns) * 64) + ln] = pk;
        }
    }
}
int amt_convh_pack_all(const amt_convh_pack_job *jobs_dev, int n, int max_elems, hipStream_t st) {
    if (n <= 0) return AMT_OK;
    const unsigned gx = (unsigned)std::min<size_t>(((size_t)max_elems + 256 * 16 - 1) / (256 * 16), 64);
    convh_wmax_kernel<<<dim3(gx, n), 256, 0, st>>>(jobs_dev);
    convh_pack_kernel<<<dim3(gx, n, 2), 256, 0, st>>>(jobs_dev);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}
int amt_convh_absmax(const float *x, size_t n, int B, float *amax, hipStream_t st) {
    return launch_absmax(x, n, n, B, amax, st);
}
int amt_convh_run(const amt_convh_plan *pl, const float *in, float *out, const float *acc, int B, const void *packed,
                  const int *sw_dev, const float *bias, const float *amax_in, int pad_t, int pad_l, hipStream_t st) {
    if (!pl || !in || !out || !packed || !sw_dev || !amax_in || B <= 0) return AMT_E_INVALID;
    if (pad_t < 0 || pad_t >= pl->kh || pad_l < 0 || pad_l >= pl->kw) return AMT_E_INVALID;
    const size_t istr = (size_t)pl->H * pl->W * pl->cin, ostr = (size_t)pl->H * pl->W * pl->cout;
    ConvParams p{in, istr, out, ostr, acc, ostr, nullptr, nullptr, bias, nullptr, nullptr, B, pl->H, pl->W, 0, 0, 1, 0, 0, pl->cout};
    p.pad_t = pad_t; p.pad_l = pad_l;
    const dim3 grid(apply_tile(p, pl->TH, pl->TW, pl->NWIN), pl->cout / 32);
    HxScale hs{amax_in, nullptr, 0, nullptr};
    hs.sw_dev = sw_dev;
    return launch_convs<true>(pl->kh, pl->kw, pl->cin, pl->masked != 0, grid, pl->lds, p, packed, hs, st);
}
