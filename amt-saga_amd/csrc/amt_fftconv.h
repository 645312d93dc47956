// Internal interface of the FFT-domain convolution form (amt_fftconv.hip), used by amt_rdcnn.hip (conv mode 3).
#pragma once
#include "amt_common.h"
#include "amt_launch.h"

struct amt_fftconv_layer;

struct FcEpilogue {
    const float *s1 = nullptr, *t1 = nullptr, *s2 = nullptr, *t2 = nullptr;   // device [32]
    const float *sc = nullptr; size_t sc_stride = 0;                          // identity shortcut [B][H][W][32]
    const float *sc1 = nullptr; size_t sc1_stride = 0;                        // rank-1 shortcut input [B][H][W]
    const float *sc1_w = nullptr, *sc1_s = nullptr, *sc1_t = nullptr;         // device [32]
    // W-pooled pair in place of the spatial output (either form; identity shortcut, no next transform): wmax / wavg
    // [B][H][W / 8][C] = max / mean of the output's columns 8 g .. 8 g + 7 (EPI = 5 of both row kernels); out_sp is then null
    float *wmax = nullptr, *wavg = nullptr; size_t wp_stride = 0;
};

// Device copies of a layer's folded BN vectors for the stand-alone entries (amt_fftconv_create, amt_fftpk_create): s1 / t1
// always, s2 / t2 (the BN after the shortcut add) where given (host [channels], null = absent; release() also frees what a
// failed upload left); a shortcut passed to a layer without them is ignored.
struct FcBnCopies {
    float *s1 = nullptr, *t1 = nullptr, *s2 = nullptr, *t2 = nullptr;
    hipError_t upload(const float *hs1, const float *ht1, const float *hs2, const float *ht2, int channels) {
        const float *h[4] = {hs1, ht1, hs2, ht2};
        float **d[4] = {&s1, &t1, &s2, &t2};
        hipError_t e = hipSuccess;
        for (int i = 0; i < 4 && e == hipSuccess; ++i) {
            if (h[i]) e = hipMalloc(d[i], channels * sizeof(float));
            if (h[i] && e == hipSuccess) e = hipMemcpy(*d[i], h[i], channels * sizeof(float), hipMemcpyHostToDevice);
        }
        return e;
    }
    void release() {
        for (float **p : {&s1, &t1, &s2, &t2}) { if (*p) (void)hipFree(*p); *p = nullptr; }
    }
};

// kernel: host [4][16][32][32] (Keras layout kh, kw, cin, cout)
int amt_fftconv_layer_create_internal(amt_fftconv_layer **out, const float *kernel);
void amt_fftconv_layer_destroy_internal(amt_fftconv_layer *L);
size_t amt_fftconv_freq_floats(int B, int H);                                // floats of one [289][B][H][64] tensor
int amt_fftconv_forward_fft(const amt_fftconv_layer *L, const float *in_sp, size_t in_stride, int B, int H, int W,
                            float *Xf, float *amaxf, hipStream_t st);
int amt_fftconv_gemm(const amt_fftconv_layer *L, const float *Xf, const float *amaxf, int B, int H, float *Yf, hipStream_t st);
int amt_fftconv_gemm_chunks_per_wg(int B);                                   // chunks of 8 windows per GEMM workgroup
int amt_fftconv_inverse_epilogue(const amt_fftconv_layer *L, const float *Yf, const FcEpilogue &ep, int B, int H, int W,
                                 float *out_sp, size_t out_stride, float *Xf_next, float *amaxf_next, float *amax_out,
                                 hipStream_t st);

// ---- packed-image form of the 10 x 64, 64 -> 64 layers (amt_fftpk.hip) ----------------------------------------------
struct amt_fftpk_layer;
// kernel: host [4][16][64][64] (Keras layout kh, kw, cin, cout); synchronises the null stream (weights are transformed on the device)
int amt_fftpk_layer_create_internal(amt_fftpk_layer **out, const float *kernel);
void amt_fftpk_layer_destroy_internal(amt_fftpk_layer *L);
size_t amt_fftpk_freq_floats(int B);                                         // floats of one [B][577][128] tensor
int amt_fftpk_forward_fft(const amt_fftpk_layer *L, const float *in_sp, size_t in_stride, int B, float *Xf, float *amaxf, hipStream_t st);
int amt_fftpk_gemm(const amt_fftpk_layer *L, const float *Xf, const float *amaxf, int B, float *Yf, hipStream_t st);
int amt_fftpk_inverse_epilogue(const amt_fftpk_layer *L, const float *Yf, const FcEpilogue &ep, int B, float *out_sp, size_t out_stride,
                               float *Xf_next, float *amaxf_next, float *amax_out, hipStream_t st);

// ---- one handle for both forms: amt_rdcnn_forward chains either kind with the same host code -------------------------
// At most one of row / pk is set; H x W is the layer's image (the packed form has it fixed at 10 x 64).
struct FcLayer {
    amt_fftconv_layer *row = nullptr;
    amt_fftpk_layer *pk = nullptr;
    int H = 0, W = 0;
    explicit operator bool() const { return row || pk; }
};
static inline size_t fc_freq_floats(const FcLayer &l, int B) {
    return l.pk ? amt_fftpk_freq_floats(B) : amt_fftconv_freq_floats(B, l.H);
}
static inline int fc_forward_fft(const FcLayer &l, const float *in_sp, size_t in_stride, int B, float *Xf, float *amaxf, hipStream_t st) {
    return l.pk ? amt_fftpk_forward_fft(l.pk, in_sp, in_stride, B, Xf, amaxf, st)
                : amt_fftconv_forward_fft(l.row, in_sp, in_stride, B, l.H, l.W, Xf, amaxf, st);
}
static inline int fc_gemm(const FcLayer &l, const float *Xf, const float *amaxf, int B, float *Yf, hipStream_t st) {
    return l.pk ? amt_fftpk_gemm(l.pk, Xf, amaxf, B, Yf, st) : amt_fftconv_gemm(l.row, Xf, amaxf, B, l.H, Yf, st);
}
static inline int fc_inverse_epilogue(const FcLayer &l, const float *Yf, const FcEpilogue &ep, int B, float *out_sp, size_t out_stride,
                                      float *Xf_next, float *amaxf_next, float *amax_out, hipStream_t st) {
    return l.pk ? amt_fftpk_inverse_epilogue(l.pk, Yf, ep, B, out_sp, out_stride, Xf_next, amaxf_next, amax_out, st)
                : amt_fftconv_inverse_epilogue(l.row, Yf, ep, B, l.H, l.W, out_sp, out_stride, Xf_next, amaxf_next, amax_out, st);
}
