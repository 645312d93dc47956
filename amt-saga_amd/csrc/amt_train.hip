// RDCNN training step for gfx950: forward in training mode, backward, Adagrad.
//
// Replaces, for the graph of the reference's RDCNN.py:176-233, what ``res_net.train`` /
// ``res_net.test`` run through Keras (RDCNN.py:503-526, :559-589): ``model.train_on_batch`` /
// ``test_on_batch`` of a model compiled with ``keras.optimizers.Adagrad()`` and
// ``mean_squared_error`` (one output) or ``sparse_categorical_crossentropy`` (RDCNN.py:245-254).
// CPU restatement and its pinning (PyTorch autograd): oracle/train.py, tests/test_oracle_train.py.
//
// Training runs at the reference's batch sizes (8 windows, main.py -batch_size), far from the
// inference loop's thousands, so this file favours one small set of exact, deterministic kernels
// over per-layer fusion:
//   * every contraction -- convolution forward (im2col rows x kernel), its data gradient
//     (dZ x kernel^T -> col2im) and its weight gradient (im2col^T x dZ), the Dense layers and their
//     gradients -- is ONE tiled GEMM kernel on the f32 matrix pipe (v_mfma_f32_32x32x2_f32, 64 x 64 tile
//     per workgroup, operands staged through LDS, optional transposed operands, split over the
//     contraction with a fixed-order reduction: no float atomics anywhere);
//   * BatchNormalization in training mode: per-channel batch statistics by two-stage column reductions,
//     moving statistics updated with momentum 0.99; its backward needs two more column sums;
//   * sigmoid, shortcut add, max / average pooling and their gradients are elementwise / gather kernels;
//   * Adagrad (a += g^2, p -= lr g / (sqrt(a) + eps); accumulators start at 0 as in Keras 2.2 / tf.keras 1.13 or
//     at 0.1 as in tf.keras >= 1.14 -- the reference pins neither) is one elementwise kernel per tensor.
// A small tape (list of ops over numbered tensors) is built from the topology (amt_rdcnn_topology.h) once; a step
// walks it forwards, then backwards accumulating gradients per tensor (the shortcut source receives two).
#include "amt_common.h"
#include "amt_launch_core.h"
#include "amt_convh.h"
#include "amt_rdcnn_topology.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

typedef float tf32x16 __attribute__((ext_vector_type(16)));
#define TR_BN_EPS 1e-3f
#define TR_BN_MOMENTUM 0.99f
#define TG_TM 64
#define TG_TN 64
#define TG_KC 32

// ---- GEMM: C[M][N] = sum_k A(m,k) B(k,n) (+ bias[n]); A stored [M][lda] (or [K][lda] when TA),
//      B stored [K][ldb] (or [N][ldb] when TB).  gridDim.z slices of the contraction write partial
//      tiles to `part` ([z][M][N]); splitk_reduce_kernel adds them in z order.
// WN = 2: 64 x 64 tile, waves 2 x 2;  WN = 1: 128 x 32 tile, waves 4 x 1 (the convolutions' N is 32 channels half
// of the time: a 64-wide tile would leave every second MFMA column block empty)
template <bool TA, bool TB, int WN>
__global__ __launch_bounds__(256) void tgemm_kernel(const float *__restrict__ A, int lda,
                                                     const float *__restrict__ B, int ldb,
                                                     float *__restrict__ C, int ldc, int M, int N, int K,
                                                     int kslice, const float *__restrict__ bias,
                                                     float *__restrict__ part) {
    constexpr int TM = 32 * (4 / WN), TN = 32 * WN;
    __shared__ float As[TM][TG_KC + 1];
    __shared__ float Bs[TG_KC][TN + 1];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
    const int kbeg = blockIdx.z * kslice, kend = min(K, kbeg + kslice);
    const int mi = WN == 2 ? wid >> 1 : wid, ni = WN == 2 ? wid & 1 : 0;
    tf32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    constexpr int NA = (TM * TG_KC) / 256, NB = (TG_KC * TN) / 256;
    float ra[NA], rb[NB];
    // the next k-step's tiles are requested before this step's MFMAs and parked in LDS after them: the global
    // latency runs under the matrix work instead of in front of it
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int idx = tid + i * 256;
            int r, c;
            if (TA) { c = idx / TM; r = idx - c * TM; } else { r = idx / TG_KC; c = idx - r * TG_KC; }
            const int m = m0 + r, k = k0 + c;
            ra[i] = (m < M && k < kend) ? (TA ? A[(size_t)k * lda + m] : A[(size_t)m * lda + k]) : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int idx = tid + i * 256;
            int c, j;
            if (TB) { j = idx / TG_KC; c = idx - j * TG_KC; } else { c = idx / TN; j = idx - c * TN; }
            const int k = k0 + c, n = n0 + j;
            rb[i] = (n < N && k < kend) ? (TB ? B[(size_t)n * ldb + k] : B[(size_t)k * ldb + n]) : 0.f;
        }
    };
    if (kbeg < kend) gload(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += TG_KC) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int idx = tid + i * 256;
            int r, c;
            if (TA) { c = idx / TM; r = idx - c * TM; } else { r = idx / TG_KC; c = idx - r * TG_KC; }
            As[r][c] = ra[i];
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int idx = tid + i * 256;
            int c, j;
            if (TB) { j = idx / TG_KC; c = idx - j * TG_KC; } else { c = idx / TN; j = idx - c * TN; }
            Bs[c][j] = rb[i];
        }
        __syncthreads();
        if (k0 + TG_KC < kend) gload(k0 + TG_KC);
#pragma unroll
        for (int kk = 0; kk < TG_KC; kk += 2) {
            const float a = As[mi * 32 + (lane & 31)][kk + (lane >> 5)];
            const float b = Bs[kk + (lane >> 5)][ni * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }
    const int n = n0 + ni * 32 + (lane & 31);
    if (n >= N) return;
    const float bv = (bias && !part) ? bias[n] : 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int m = m0 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (m >= M) continue;
        if (part) part[((size_t)blockIdx.z * M + m) * N + n] = acc[e];
        else C[(size_t)m * ldc + n] = acc[e] + bv;
    }
}
__global__ void splitk_reduce_kernel(const float *__restrict__ part, int Z, float *__restrict__ C, int ldc,
                                     int M, int N, const float *__restrict__ bias) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t MN = (size_t)M * N;
    if (i >= MN) return;
    float v = part[i];
    int z = 1;
    for (; z + 8 <= Z; z += 8) {                             // eight loads in flight, added in z order
        float q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = part[(size_t)(z + u) * MN + i];
#pragma unroll
        for (int u = 0; u < 8; ++u) v += q[u];
    }
    for (; z < Z; ++z) v += part[(size_t)z * MN + i];
    const int m = (int)(i / N), n = (int)(i - (size_t)m * N);
    C[(size_t)m * ldc + n] = v + (bias ? bias[n] : 0.f);
}

// ---- im2col / col2im (Keras "same" padding: before = (k-1)/2, the rest after) -------------------
// One workgroup per output position (b, h, w): its K = KH KW C row is written contiguously, four channels per
// lane and access where C allows (the index arithmetic is 32-bit and per tap, not 64-bit per element).
__global__ __launch_bounds__(256) void im2col_kernel(const float *__restrict__ x, size_t x_stride, int B, int H, int W,
                                                     int C, int KH, int KW, float *__restrict__ col) {
    const int K = KH * KW * C;
    const int pt = (KH - 1) / 2, pl = (KW - 1) / 2;
    const int npos = B * H * W;
    for (int pos = blockIdx.x; pos < npos; pos += gridDim.x) {
        const int w = pos % W, hb = pos / W, h = hb % H, b = hb / H;
        const float *xb = x + (size_t)b * x_stride;
        float *row = col + (size_t)pos * K;
        if ((C & 3) == 0) {
            const int C4 = C >> 2;
            for (int q = threadIdx.x; q < (K >> 2); q += 256) {
                const int tap = q / C4, c4 = q - tap * C4;
                const int dy = tap / KW, dx = tap - dy * KW;
                const int hh = h + dy - pt, ww = w + dx - pl;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (hh >= 0 && hh < H && ww >= 0 && ww < W)
                    v = *reinterpret_cast<const float4 *>(xb + ((size_t)hh * W + ww) * C + 4 * c4);
                *reinterpret_cast<float4 *>(row + 4 * q) = v;
            }
        } else {
            for (int kk = threadIdx.x; kk < K; kk += 256) {
                const int tap = kk / C, ci = kk - tap * C;
                const int dy = tap / KW, dx = tap - dy * KW;
                const int hh = h + dy - pt, ww = w + dx - pl;
                row[kk] = (hh >= 0 && hh < H && ww >= 0 && ww < W) ? xb[((size_t)hh * W + ww) * C + ci] : 0.f;
            }
        }
    }
}
// dX[b][h][w][ci] = sum over taps of dcol[(b, h - dy + pt, w - dx + pl)][(dy, dx, ci)]   (gather: no atomics).
// A workgroup takes 256 / min(C, 256) input positions at a time, lanes over channels, taps in a fixed order.
__global__ __launch_bounds__(256) void col2im_kernel(const float *__restrict__ dcol, int B, int H, int W, int C, int KH,
                                                     int KW, float *__restrict__ dx_) {
    const int K = KH * KW * C;
    const int pt = (KH - 1) / 2, pl = (KW - 1) / 2;
    const int npos = B * H * W;
    const int cw = min(C, 256), ppw = 256 / cw;            // channels per pass of a position, positions per workgroup
    const int sub = threadIdx.x / cw, c0 = threadIdx.x - sub * cw;
    for (int pos = blockIdx.x * ppw + sub; pos < npos && sub < ppw; pos += gridDim.x * ppw) {
        const int w = pos % W, hb = pos / W, h = hb % H, b = hb / H;
        for (int ci = c0; ci < C; ci += cw) {
            float s = 0.f;
            for (int dy = 0; dy < KH; ++dy) {
                const int ho = h - dy + pt;
                if (ho < 0 || ho >= H) continue;
                for (int dx = 0; dx < KW; ++dx) {
                    const int wo = w - dx + pl;
                    if (wo < 0 || wo >= W) continue;
                    s += dcol[(((size_t)b * H + ho) * W + wo) * K + (dy * KW + dx) * C + ci];
                }
            }
            dx_[(size_t)pos * C + ci] = s;
        }
    }
}


// ---- weight gradient of a KH x 16 convolution without the im2col matrix ------------------------------------------------
// dW[dy][dx][ci][co] = sum over (b, h, w) of x(b, h + dy - pt, w + dx - pl, ci) dZ(b, h, w, co).
// blockIdx.y = (dy, 32-channel block of ci, 32-channel block of co); a workgroup walks row segments (b, h, w0 .. w0 + seg) in
// a fixed stride, staging the ONE input row its dy needs (seg + 15 positions x 32 channels) and the dZ segment in LDS; wave v
// owns the four taps dx = 4 v .. 4 v + 3, i.e. four 32 x 32 accumulators on v_mfma_f32_32x32x2_f32 (A = x, rows = ci,
// k = position; B = dZ, columns = co), so one B fragment feeds four MFMAs.  Every workgroup writes its partial sums; they are
// added in workgroup order by splitk_reduce_kernel (no float atomics).
struct WgArgs {
    const float *x, *dz;
    float *part;
    int B, H, W, Cin, Cout, KH, pt, pl;
    int seg, nseg, ntiles;
};
template <int KW>
__global__ __launch_bounds__(256, 3) void wgrad_kernel(WgArgs a) {
    constexpr int TPW = KW / 4;                              // taps per wave
    extern __shared__ __attribute__((aligned(16))) float wg_lds[];
    float *xs = wg_lds;                                      // [seg + KW - 1][32]
    float *ds = wg_lds + (size_t)(a.seg + KW - 1) * 32;      // [seg][32]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ncob = a.Cout / 32, ncib = a.Cin / 32;
    const int cob = blockIdx.y % ncob, cib = (blockIdx.y / ncob) % ncib, dy = blockIdx.y / (ncob * ncib);
    tf32x16 acc[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    const int half = lane >> 5, n = lane & 31;
    for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int sgi = t % a.nseg, bh = t / a.nseg, h = bh % a.H, b = bh / a.H;
        const int hr = h + dy - a.pt;
        if (hr < 0 || hr >= a.H) continue;                   // the whole row is padding (uniform over the workgroup)
        const int w0 = sgi * a.seg, len = min(a.seg, a.W - w0);
        __syncthreads();
        const float *xrow = a.x + ((size_t)(b * a.H + hr) * a.W) * a.Cin + cib * 32;
        for (int idx = tid; idx < (a.seg + KW - 1) * 8; idx += 256) {
            const int pos = idx >> 3, c4 = idx & 7, ws = w0 - a.pl + pos;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ws >= 0 && ws < a.W) v = *reinterpret_cast<const float4 *>(xrow + (size_t)ws * a.Cin + c4 * 4);
            *reinterpret_cast<float4 *>(xs + pos * 32 + c4 * 4) = v;
        }
        const float *drow = a.dz + ((size_t)(b * a.H + h) * a.W + w0) * a.Cout + cob * 32;
        for (int idx = tid; idx < a.seg * 8; idx += 256) {
            const int pos = idx >> 3, c4 = idx & 7;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pos < len) v = *reinterpret_cast<const float4 *>(drow + (size_t)pos * a.Cout + c4 * 4);
            *reinterpret_cast<float4 *>(ds + pos * 32 + c4 * 4) = v;
        }
        __syncthreads();
        const float *xa = xs + (half + wid * TPW) * 32 + n;
        const float *db = ds + half * 32 + n;
        const int ksteps = (len + 1) >> 1;
        for (int q = 0; q < ksteps; ++q) {
            const float bv = db[q * 64];
#pragma unroll
            for (int j = 0; j < TPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[q * 64 + j * 32], bv, acc[j], 0, 0, 0);
        }
    }
    float *out = a.part + (size_t)blockIdx.x * ((size_t)a.KH * KW * a.Cin * a.Cout);
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int tap = dy * KW + wid * TPW + j;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ci = cib * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
            out[((size_t)tap * a.Cin + ci) * a.Cout + cob * 32 + n] = acc[j][e];
        }
    }
}

// ---- column reductions over a [M][C] matrix: two stages, fixed order ---------------------------------
// mode 0 / 3: sum x;  1: sum (x - mu[c])^2;  2: (sum dy, sum dy * zhat) with zhat = (z - mu) * inv
#define CR_SPLIT 512                      // most row splits of a column reduction (the launcher picks 8 .. CR_SPLIT from M)
__global__ __launch_bounds__(256) void colreduce_kernel(const float *__restrict__ x, const float *__restrict__ z,
                                                         const float *__restrict__ mu, const float *__restrict__ inv,
                                                         size_t M, int C, int mode, int nsplit,
                                                         float *__restrict__ part0, float *__restrict__ part1) {
    // block = 8 row-lanes x 32 channels; blockIdx.x = channel block, blockIdx.y = row split
    __shared__ float red0[8][33], red1[8][33];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    const size_t rows = (M + nsplit - 1) / nsplit;
    const size_t r0 = (size_t)blockIdx.y * rows, r1 = min(M, r0 + rows);
    float s0 = 0.f, s1 = 0.f;
    if (c < C) {
        const float m = (mode >= 1 && mu) ? mu[c] : 0.f, iv = mode == 2 ? inv[c] : 0.f;
#pragma unroll 4
        for (size_t r = r0 + rl; r < r1; r += 8) {
            const float v = x[r * C + c];
            if (mode == 0 || mode == 3) s0 += v;
            else if (mode == 1) { const float d = v - m; s0 += d * d; }
            else { s0 += v; s1 += v * ((z[r * C + c] - m) * iv); }
        }
    }
    red0[rl][cl] = s0; red1[rl][cl] = s1;
    __syncthreads();
    if (rl == 0 && c < C) {
        float a = 0.f, b = 0.f;
        for (int i = 0; i < 8; ++i) { a += red0[i][cl]; b += red1[i][cl]; }
        part0[(size_t)blockIdx.y * C + c] = a;
        if (mode == 2) part1[(size_t)blockIdx.y * C + c] = b;
    }
}
// mode 0 -> out0 = sum / M (mean);  mode 1 -> out0 = var = sum / M, out1 = 1/sqrt(var + eps);
// mode 2 -> out0 = sum dy, out1 = sum dy zhat;  mode 3 -> out0 = plain sum
// One workgroup per 32 channels: eight row-lanes add nsplit / 8 partials each (fixed order), LDS combines them.
__global__ __launch_bounds__(256) void colreduce_final_kernel(const float *__restrict__ part0, const float *__restrict__ part1,
                                                               int C, float invM, int mode, int nsplit,
                                                               float *__restrict__ out0, float *__restrict__ out1) {
    __shared__ float red0[8][33], red1[8][33];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    float a = 0.f, b = 0.f;
    if (c < C) {
        int s = rl;
        for (; s + 56 < nsplit; s += 64) {                   // eight partials per lane in flight, added in order
            float q0[8], q1[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                q0[u] = part0[(size_t)(s + 8 * u) * C + c];
                q1[u] = mode == 2 ? part1[(size_t)(s + 8 * u) * C + c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) { a += q0[u]; b += q1[u]; }
        }
        for (; s < nsplit; s += 8) { a += part0[(size_t)s * C + c]; if (mode == 2) b += part1[(size_t)s * C + c]; }
    }
    red0[rl][cl] = a; red1[rl][cl] = b;
    __syncthreads();
    if (rl != 0 || c >= C) return;
    a = 0.f; b = 0.f;
    for (int i = 0; i < 8; ++i) { a += red0[i][cl]; b += red1[i][cl]; }
    if (mode == 0) out0[c] = a * invM;
    else if (mode == 1) { const float v = a * invM; out0[c] = v; out1[c] = 1.0f / sqrtf(v + TR_BN_EPS); }
    else if (mode == 2) { out0[c] = a; out1[c] = b; }
    else out0[c] = a;
}


// ---- fused BatchNormalization passes ---------------------------------------------------------------------------------
// For C a power of two (4 .. 1024; every BatchNormalization of the reference's graphs has 32 2^k channels).  All four
// kernels share one thread layout: a workgroup covers BNF_RPT * RL consecutive rows of the [M][C] matrix, RL = 1024 / C
// row lanes, one float4 (four channels) per thread and row.  Sums over row lanes are taken in lane order by one thread
// per channel quad, partial results per workgroup are combined in workgroup order by a second, tiny launch: fixed order,
// no float atomics.
//   bnf_stats_kernel        per-workgroup (mean, sum of squared deviations from that mean) of every channel; the final
//                           launch merges them pairwise (Chan et al.), so the variance never sees E[x^2] - mean^2
//   bnf_act_kernel          y = (z - mu) inv gamma + beta [-> sigmoid], plus max |output| per window for the next
//                           convolution's operand scaling
//   bnf_bwd_reduce_kernel   sum dy, sum dy zhat with dy = dA a (1 - a) formed on the fly (the sigmoid's gradient)
//   bnf_bwd_apply_kernel    dz = gamma inv (dy - mean dy - zhat mean(dy zhat)),
//                           plus per-workgroup column sums of dz (the bias gradient of the convolution in front) and
//                           max |dz| per window (operand scaling of the data gradient)
#define BNF_RPT 8
__device__ __forceinline__ float4 f4_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float f4_amax(float4 a) { return fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))); }
// sum over the RL row lanes of channel quad cq, in lane order (called by the threads of row lane 0)
__device__ __forceinline__ float4 bnf_lane_sum(const float4 *red, int CQ, int RL, int cq) {
    float4 a = red[cq];
    for (int j = 1; j < RL; ++j) a = f4_add(a, red[j * CQ + cq]);
    return a;
}
// max |.| per window: rows r0 .. r0 + nrows of one workgroup usually lie in one window (HW rows each)
__device__ __forceinline__ void bnf_window_max(const float (&m)[BNF_RPT], int rl, int RL, size_t r0, int nrows, int HW,
                                               float *amax, float *lds16) {
    const size_t w0 = r0 / HW, w1 = (r0 + nrows - 1) / HW;
    for (size_t w = w0; w <= w1; ++w) {                      // one block reduction and ONE atomic per window touched
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < BNF_RPT; ++i) {
            const int r = rl + i * RL;
            if (w0 == w1 || (r < nrows && (r0 + r) / HW == w)) v = fmaxf(v, m[i]);
        }
        v = block_max(v, lds16);
        if (threadIdx.x == 0) atomicMax(reinterpret_cast<int *>(amax) + w, __float_as_int(v));
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void bnf_stats_kernel(const float *__restrict__ x, size_t M, int C,
                                                         float *__restrict__ pmean, float *__restrict__ pm2) {
    __shared__ float4 red[256];
    __shared__ float4 bc[256];
    const int CQ = C >> 2, RL = 256 / CQ, rl = threadIdx.x / CQ, cq = threadIdx.x - rl * CQ;
    const size_t r0 = (size_t)blockIdx.x * (RL * BNF_RPT);
    const int nrows = (int)min((size_t)(RL * BNF_RPT), M - r0);
    float4 v[BNF_RPT];
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < BNF_RPT; ++i) {
        const int r = rl + i * RL;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < nrows) { v[i] = *reinterpret_cast<const float4 *>(x + (r0 + r) * C + 4 * cq); s = f4_add(s, v[i]); }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (rl == 0) {
        const float4 a = bnf_lane_sum(red, CQ, RL, cq);
        const float n = (float)nrows;
        bc[cq] = make_float4(a.x / n, a.y / n, a.z / n, a.w / n);
    }
    __syncthreads();
    const float4 mean = bc[cq];
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < BNF_RPT; ++i) {
        if (rl + i * RL >= nrows) continue;
        const float dx = v[i].x - mean.x, dy = v[i].y - mean.y, dz = v[i].z - mean.z, dw = v[i].w - mean.w;
        q.x += dx * dx; q.y += dy * dy; q.z += dz * dz; q.w += dw * dw;
    }
    red[threadIdx.x] = q;
    __syncthreads();
    if (rl == 0) {
        const float4 a = bnf_lane_sum(red, CQ, RL, cq);
        *reinterpret_cast<float4 *>(pmean + (size_t)blockIdx.x * C + 4 * cq) = mean;
        *reinterpret_cast<float4 *>(pm2 + (size_t)blockIdx.x * C + 4 * cq) = a;
    }
}
__device__ __forceinline__ void bnf_merge(float &na, float &ma, float &qa, float nb, float mb, float qb) {
    if (nb <= 0.f) return;
    const float n = na + nb, d = mb - ma;
    ma += d * (nb / n);
    qa += qb + d * d * (na * nb / n);
    na = n;
}
// one workgroup per 32 channels; eight row lanes merge every eighth partial, lane 0 merges the eight results in order.
// Also the moving statistics (momentum 0.99, unbiased variance: see moving_update_kernel) when `update` is set.
__global__ __launch_bounds__(256) void bnf_stats_final_kernel(const float *__restrict__ pmean, const float *__restrict__ pm2,
                                                               size_t M, int C, int rows_wg, int nwg, float *__restrict__ mu,
                                                               float *__restrict__ var, float *__restrict__ inv,
                                                               float *__restrict__ mm, float *__restrict__ mv, int update,
                                                               float bessel) {
    __shared__ float sn[8][33], sm[8][33], sq[8][33];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    float n = 0.f, m = 0.f, q = 0.f;
    if (c < C) {
        int s = rl;
        for (; s + 56 < nwg; s += 64) {                      // eight partials per lane in flight, merged in order
            float pm[8], pq[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { pm[u] = pmean[(size_t)(s + 8 * u) * C + c]; pq[u] = pm2[(size_t)(s + 8 * u) * C + c]; }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                bnf_merge(n, m, q, (float)min((size_t)rows_wg, M - (size_t)(s + 8 * u) * rows_wg), pm[u], pq[u]);
        }
        for (; s < nwg; s += 8) {
            const float nb = (float)min((size_t)rows_wg, M - (size_t)s * rows_wg);
            bnf_merge(n, m, q, nb, pmean[(size_t)s * C + c], pm2[(size_t)s * C + c]);
        }
    }
    sn[rl][cl] = n; sm[rl][cl] = m; sq[rl][cl] = q;
    __syncthreads();
    if (rl != 0 || c >= C) return;
    for (int i = 1; i < 8; ++i) bnf_merge(n, m, q, sn[i][cl], sm[i][cl], sq[i][cl]);
    const float v = q / (float)M;
    mu[c] = m; var[c] = v; inv[c] = 1.0f / sqrtf(v + TR_BN_EPS);
    if (update) {
        mm[c] = TR_BN_MOMENTUM * mm[c] + (1.0f - TR_BN_MOMENTUM) * m;
        mv[c] = TR_BN_MOMENTUM * mv[c] + (1.0f - TR_BN_MOMENTUM) * (v * bessel);
    }
}
__global__ __launch_bounds__(256) void bnf_act_kernel(const float *__restrict__ z, const float *__restrict__ mu,
                                                       const float *__restrict__ inv, const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, size_t M, int C, int HW, int sig,
                                                       float *__restrict__ out, float *__restrict__ amax) {
    __shared__ float lds16[16];
    const int CQ = C >> 2, RL = 256 / CQ, rl = threadIdx.x / CQ, cq = threadIdx.x - rl * CQ;
    const size_t r0 = (size_t)blockIdx.x * (RL * BNF_RPT);
    const int nrows = (int)min((size_t)(RL * BNF_RPT), M - r0);
    const float4 mu4 = *reinterpret_cast<const float4 *>(mu + 4 * cq), iv4 = *reinterpret_cast<const float4 *>(inv + 4 * cq);
    const float4 g4 = *reinterpret_cast<const float4 *>(gamma + 4 * cq), b4 = *reinterpret_cast<const float4 *>(beta + 4 * cq);
    float m[BNF_RPT];
#pragma unroll
    for (int i = 0; i < BNF_RPT; ++i) {
        const int r = rl + i * RL;
        m[i] = 0.f;
        if (r >= nrows) continue;
        const float4 v = *reinterpret_cast<const float4 *>(z + (r0 + r) * C + 4 * cq);
        float4 y = make_float4((v.x - mu4.x) * iv4.x * g4.x + b4.x, (v.y - mu4.y) * iv4.y * g4.y + b4.y,
                               (v.z - mu4.z) * iv4.z * g4.z + b4.z, (v.w - mu4.w) * iv4.w * g4.w + b4.w);
        if (sig) y = make_float4(1.0f / (1.0f + expf(-y.x)), 1.0f / (1.0f + expf(-y.y)), 1.0f / (1.0f + expf(-y.z)),
                                 1.0f / (1.0f + expf(-y.w)));
        *reinterpret_cast<float4 *>(out + (r0 + r) * C + 4 * cq) = y;
        m[i] = f4_amax(y);
    }
    if (amax) bnf_window_max(m, rl, RL, r0, nrows, HW, amax, lds16);
}
__device__ __forceinline__ float4 bnf_dy(float4 d, const float *a, size_t off) {
    if (!a) return d;
    const float4 s = *reinterpret_cast<const float4 *>(a + off);
    return make_float4(d.x * s.x * (1.0f - s.x), d.y * s.y * (1.0f - s.y), d.z * s.z * (1.0f - s.z), d.w * s.w * (1.0f - s.w));
}
__global__ __launch_bounds__(256) void bnf_bwd_reduce_kernel(const float *__restrict__ dA, const float *__restrict__ a,
                                                              const float *__restrict__ z, const float *__restrict__ mu,
                                                              const float *__restrict__ inv, size_t M, int C,
                                                              float *__restrict__ part0, float *__restrict__ part1) {
    __shared__ float4 red[256];
    const int CQ = C >> 2, RL = 256 / CQ, rl = threadIdx.x / CQ, cq = threadIdx.x - rl * CQ;
    const size_t r0 = (size_t)blockIdx.x * (RL * BNF_RPT);
    const int nrows = (int)min((size_t)(RL * BNF_RPT), M - r0);
    const float4 mu4 = *reinterpret_cast<const float4 *>(mu + 4 * cq), iv4 = *reinterpret_cast<const float4 *>(inv + 4 * cq);
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
#pragma unroll
    for (int i = 0; i < BNF_RPT; ++i) {
        const int r = rl + i * RL;
        if (r >= nrows) continue;
        const size_t off = (r0 + r) * C + 4 * cq;
        const float4 dy = bnf_dy(*reinterpret_cast<const float4 *>(dA + off), a, off);
        const float4 v = *reinterpret_cast<const float4 *>(z + off);
        s0 = f4_add(s0, dy);
        s1.x += dy.x * ((v.x - mu4.x) * iv4.x); s1.y += dy.y * ((v.y - mu4.y) * iv4.y);
        s1.z += dy.z * ((v.z - mu4.z) * iv4.z); s1.w += dy.w * ((v.w - mu4.w) * iv4.w);
    }
    red[threadIdx.x] = s0;
    __syncthreads();
    if (rl == 0) *reinterpret_cast<float4 *>(part0 + (size_t)blockIdx.x * C + 4 * cq) = bnf_lane_sum(red, CQ, RL, cq);
    __syncthreads();
    red[threadIdx.x] = s1;
    __syncthreads();
    if (rl == 0) *reinterpret_cast<float4 *>(part1 + (size_t)blockIdx.x * C + 4 * cq) = bnf_lane_sum(red, CQ, RL, cq);
}
__global__ __launch_bounds__(256) void bnf_bwd_apply_kernel(const float *__restrict__ dA, const float *__restrict__ a,
                                                             const float *__restrict__ z, const float *__restrict__ mu,
                                                             const float *__restrict__ inv, const float *__restrict__ gamma,
                                                             const float *__restrict__ sdy, const float *__restrict__ sdyz,
                                                             float invM, size_t M, int C, int HW, float *dst,
                                                             float *__restrict__ part2, float *__restrict__ gamax) {
    __shared__ float4 red[256];
    __shared__ float lds16[16];
    const int CQ = C >> 2, RL = 256 / CQ, rl = threadIdx.x / CQ, cq = threadIdx.x - rl * CQ;
    const size_t r0 = (size_t)blockIdx.x * (RL * BNF_RPT);
    const int nrows = (int)min((size_t)(RL * BNF_RPT), M - r0);
    const float4 mu4 = *reinterpret_cast<const float4 *>(mu + 4 * cq), iv4 = *reinterpret_cast<const float4 *>(inv + 4 * cq);
    const float4 g4 = *reinterpret_cast<const float4 *>(gamma + 4 * cq);
    const float4 a4 = *reinterpret_cast<const float4 *>(sdy + 4 * cq), b4 = *reinterpret_cast<const float4 *>(sdyz + 4 * cq);
    float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);
    float m[BNF_RPT];
#pragma unroll
    for (int i = 0; i < BNF_RPT; ++i) {
        const int r = rl + i * RL;
        m[i] = 0.f;
        if (r >= nrows) continue;
        const size_t off = (r0 + r) * C + 4 * cq;
        const float4 dy = bnf_dy(*reinterpret_cast<const float4 *>(dA + off), a, off);
        const float4 v = *reinterpret_cast<const float4 *>(z + off);
        float4 d;
        d.x = g4.x * iv4.x * (dy.x - a4.x * invM - ((v.x - mu4.x) * iv4.x) * (b4.x * invM));
        d.y = g4.y * iv4.y * (dy.y - a4.y * invM - ((v.y - mu4.y) * iv4.y) * (b4.y * invM));
        d.z = g4.z * iv4.z * (dy.z - a4.z * invM - ((v.z - mu4.z) * iv4.z) * (b4.z * invM));
        d.w = g4.w * iv4.w * (dy.w - a4.w * invM - ((v.w - mu4.w) * iv4.w) * (b4.w * invM));
        cs = f4_add(cs, d);
        m[i] = f4_amax(d);
        *reinterpret_cast<float4 *>(dst + off) = d;
    }
    if (part2) {
        red[threadIdx.x] = cs;
        __syncthreads();
        if (rl == 0) *reinterpret_cast<float4 *>(part2 + (size_t)blockIdx.x * C + 4 * cq) = bnf_lane_sum(red, CQ, RL, cq);
    }
    if (gamax) bnf_window_max(m, rl, RL, r0, nrows, HW, gamax, lds16);
}

// ---- elementwise ----------------------------------------------------------------------------------
__global__ void bn_apply_kernel(const float *__restrict__ z, const float *__restrict__ mu, const float *__restrict__ inv,
                                const float *__restrict__ gamma, const float *__restrict__ beta, size_t n, int C,
                                float *__restrict__ y) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        y[i] = (z[i] - mu[c]) * inv[c] * gamma[c] + beta[c];
    }
}
__global__ void bn_backward_kernel(const float *dy /* may alias dz */, const float *__restrict__ z, const float *__restrict__ mu,
                                   const float *__restrict__ inv, const float *__restrict__ gamma,
                                   const float *__restrict__ sdy, const float *__restrict__ sdyz, float invM, size_t n,
                                   int C, int training, float *dz) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const float zh = (z[i] - mu[c]) * inv[c];
        dz[i] = training ? gamma[c] * inv[c] * (dy[i] - sdy[c] * invM - zh * (sdyz[c] * invM)) : gamma[c] * inv[c] * dy[i];
    }
}
// The batch is normalised with the BIASED variance, but the moving variance absorbs the UNBIASED one: TensorFlow's
// fused batch norm hands var * M / (M - 1) to the running average (Keras 2.2's own path multiplies by
// M / (M - (1 + epsilon)): 1e-3 / M apart), M = the samples per channel of this batch.  `bessel` = M / (M - 1), 1 for M = 1.
__global__ void moving_update_kernel(float *__restrict__ mm, float *__restrict__ mv, const float *__restrict__ mu,
                                     const float *__restrict__ var, int C, float bessel) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    mm[c] = TR_BN_MOMENTUM * mm[c] + (1.0f - TR_BN_MOMENTUM) * mu[c];
    mv[c] = TR_BN_MOMENTUM * mv[c] + (1.0f - TR_BN_MOMENTUM) * (var[c] * bessel);
}
__global__ void inv_from_var_kernel(const float *__restrict__ var, int C, float *__restrict__ inv) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) inv[c] = 1.0f / sqrtf(var[c] + TR_BN_EPS);
}
__global__ void sigmoid_fwd_kernel(const float *__restrict__ x, size_t n, float *__restrict__ y) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        y[i] = 1.0f / (1.0f + expf(-x[i]));
}
__global__ void sigmoid_bwd_kernel(const float *dy, const float *__restrict__ a, size_t n, float *dx) {   // dy may alias dx
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        dx[i] = dy[i] * a[i] * (1.0f - a[i]);
}
__global__ void add_kernel(const float *__restrict__ a, const float *__restrict__ b, size_t n, float *__restrict__ y) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        y[i] = a[i] + b[i];
}
// pooling (valid, stride = pool); out rows may be written with a row pitch (flatten into the dense input)
__global__ void pool_fwd_kernel(const float *__restrict__ x, int B, int H, int W, int C, int PH, int PW, int is_max,
                                float *__restrict__ y, size_t y_stride) {
    const int HO = H / PH, WO = W / PW;
    const size_t total = (size_t)B * HO * WO * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        size_t r = i / C;
        const int wo = (int)(r % WO); r /= WO;
        const int ho = (int)(r % HO);
        const int b = (int)(r / HO);
        float m = is_max ? -INFINITY : 0.f;
        for (int dy = 0; dy < PH; ++dy)
            for (int dx = 0; dx < PW; ++dx) {
                const float v = x[(((size_t)b * H + ho * PH + dy) * W + wo * PW + dx) * C + c];
                m = is_max ? fmaxf(m, v) : m + v;
            }
        if (!is_max) m /= (float)(PH * PW);
        y[(size_t)b * y_stride + ((size_t)ho * WO + wo) * C + c] = m;
    }
}
// gradient of the pooling: max routes to the FIRST maximum in (dy, dx) order; the part of x the valid
// pooling never read gets zero
__global__ void pool_bwd_kernel(const float *__restrict__ dy_, size_t dy_stride, const float *__restrict__ x, int B, int H,
                                int W, int C, int PH, int PW, int is_max, float *__restrict__ dx_) {
    const int HO = H / PH, WO = W / PW;
    const size_t total = (size_t)B * H * W * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        size_t r = i / C;
        const int w = (int)(r % W); r /= W;
        const int h = (int)(r % H);
        const int b = (int)(r / H);
        const int ho = h / PH, wo = w / PW;
        float g = 0.f;
        if (ho < HO && wo < WO) {
            const float d = dy_[(size_t)b * dy_stride + ((size_t)ho * WO + wo) * C + c];
            if (!is_max) g = d / (float)(PH * PW);
            else {
                int best = 0; float bv = -INFINITY;
                for (int dy = 0; dy < PH; ++dy)
                    for (int dx = 0; dx < PW; ++dx) {
                        const float v = x[(((size_t)b * H + ho * PH + dy) * W + wo * PW + dx) * C + c];
                        if (v > bv) { bv = v; best = dy * PW + dx; }
                    }
                g = ((h - ho * PH) * PW + (w - wo * PW)) == best ? d : 0.f;
            }
        }
        dx_[i] = g;
    }
}
__global__ void copy_rows_kernel(const float *__restrict__ src, size_t src_stride, float *__restrict__ dst,
                                 size_t dst_stride, int B, size_t n) {
    const size_t total = (size_t)B * n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / n, j = i - b * n;
        dst[b * dst_stride + j] = src[b * src_stride + j];
    }
}
// loss + gradient wrt the last Dense's output.  K == 1: pred = sigmoid(z), loss = mean (pred - y)^2 (Keras
// mean_squared_error on the activation-scale target); K > 1: softmax + sparse categorical cross-entropy.
__global__ void loss_kernel(const float *__restrict__ z, const float *__restrict__ y, int B, int K, float *__restrict__ pred,
                            float *__restrict__ dz, float *__restrict__ loss_rows) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float *l = z + (size_t)b * K;
    if (K == 1) {
        const float p = 1.0f / (1.0f + expf(-l[0]));
        const float d = p - y[b];
        pred[b] = p;
        loss_rows[b] = d * d;
        dz[b] = 2.0f * d / (float)B * p * (1.0f - p);
    } else {
        float m = -INFINITY;
        for (int k = 0; k < K; ++k) m = fmaxf(m, l[k]);
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += expf(l[k] - m);
        int yi = (int)y[b];
        yi = yi < 0 ? 0 : (yi >= K ? K - 1 : yi);
        for (int k = 0; k < K; ++k) {
            const float p = expf(l[k] - m) / s;
            pred[(size_t)b * K + k] = p;
            dz[(size_t)b * K + k] = (p - (k == yi ? 1.0f : 0.0f)) / (float)B;
        }
        loss_rows[b] = -(l[yi] - m - logf(s));
    }
}
__global__ void adagrad_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ acc, size_t n,
                               float lr, float eps) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float gi = g[i];
        const float a = acc[i] + gi * gi;
        acc[i] = a;
        p[i] = p[i] - lr * gi / (sqrtf(a) + eps);
    }
}

// =====================================================================================
// host side
// =====================================================================================
namespace {

#define TR_TRY(x) do { const int rc_ = (x); if (rc_ != AMT_OK) return rc_; } while (0)

// The AMT_TRAIN_* environment, read once: when a trainer (which holds one of these) is created
struct TrainOptions {
    bool fast = amt_env_switch("AMT_TRAIN_FAST", true);              // =0: every convolution on im2col + f32 GEMM (+ col2im)
    bool wgrad_direct = amt_env_switch("AMT_TRAIN_WGRAD", true);     // =0: weight gradients through im2col + GEMM
    bool fused_bn = amt_env_switch("AMT_TRAIN_FUSED_BN", true);      // =0: the generic column-reduction BatchNormalization
    size_t fast_min_m = (size_t)amt_env_number("AMT_TRAIN_FAST_MIN_M", 2048, 0);   // fewest output positions (B H W) for the fast forms
    bool trace = amt_env_switch("AMT_TRAIN_TRACE", false);           // set: synchronise and report after every op
};

// Per-batch device storage: knows its capacity and frees what it replaces when it grows.  Reads as the pointer.
struct DevBuf {
    float *p = nullptr;
    size_t cap = 0;                      // floats
    operator float *() const { return p; }
    // At least n floats; the contents do not survive growth.  hipFree synchronises the device, so no kernel of this or
    // an earlier step still reads the block that goes and freeing needs no ordering of its own; whoever derived a
    // pointer from p derives it again (ensure_batch: the tensors' am_slot / gam_slot; everything else is re-read from
    // the buffer at each use).
    int reserve(size_t n) {
        if (p && n <= cap) return AMT_OK;
        release();
        if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(float)) != hipSuccess) { p = nullptr; return AMT_E_NOMEM; }
        cap = n;
        return AMT_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
};

struct Param { float *w = nullptr, *g = nullptr, *acc = nullptr; size_t n = 0, off = 0 /* in the canonical blob */; bool trainable = true; };

enum OpKind { OP_CONV /* and Dense: a 1 x 1 convolution over one position */, OP_BN, OP_SIGMOID, OP_ADD, OP_POOL, OP_FLATTEN, OP_KINDS };
struct Op {
    OpKind kind;
    int in0 = -1, in1 = -1, out = -1;             // tensor ids
    int H = 0, W = 0, Cin = 0, Cout = 0, kh = 1, kw = 1;    // conv / pool (kh, kw = pool)
    int is_max = 0;
    int p0 = -1, p1 = -1, p2 = -1, p3 = -1;       // params: conv (kernel, bias); bn (gamma, beta, mean, var)
    int flat_off = 0;                              // OP_FLATTEN: column offset in the dense input
    float *bmu = nullptr, *binv = nullptr, *bvar = nullptr;      // BN batch statistics of the last forward
    bool is_input = false;                         // OP_CONV reading a tower's input: no data gradient
    // OP_CONV on the split-fp16 kernels (amt_convh.h): forward and, when the transposed shape is covered too, the data
    // gradient; job = index of the layer's weight-preparation job (-1: the GEMM path)
    int job = -1;
    bool fast_bwd = false;
    amt_convh_plan fplan, bplan;
    void *wp_f = nullptr, *wp_b = nullptr;
    // OP_BN on the fused passes (bnf_*): sig_out >= 0 when the sigmoid that follows is folded in (its output tensor is
    // written directly and the OP_SIGMOID is skipped, forwards and backwards)
    bool bn_fused = false;
    int sig_out = -1;
    bool skip = false;                             // OP_SIGMOID folded into the BatchNormalization in front of it
};
// g is the tensor's own gradient buffer; gptr is where its gradient currently lives (its own buffer, or -- after a
// shortcut Add handed the same gradient to two tensors -- the buffer of the tensor it came from: gradients are only
// ever written into the destination's own buffer, never in place into a source, so such a view stays valid).
// am / gam: per-window max |v| / max |g| left by the producing kernel this step (null: not measured)
struct Tensor {
    int H, W, C;
    DevBuf v, g;
    float *gptr = nullptr; bool g_set = false;
    float *am_slot = nullptr, *gam_slot = nullptr, *am = nullptr, *gam = nullptr;
    size_t numel(int B) const { return (size_t)B * H * W * C; }
};

struct Step { int B; bool training; hipStream_t st; };

static unsigned grid1(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, 65535); }

}  // namespace

struct amt_trainer {
    amt_rdcnn_desc d;
    TrainOptions opt;
    std::vector<Param> params;                    // canonical order (rdcnn.py pack_weights)
    std::vector<Op> ops;
    std::vector<Tensor> tensors;
    std::vector<int> inputs;                      // tensor id of each tower's input
    int t_flat = -1, t_logits = -1;
    int flat = 0, capB = 0;
    size_t blob_floats = 0;
    float lr = 0.01f, eps = 1e-7f, acc0 = 0.f;
    std::vector<float *> allocs;                  // created once, owned until destroy: arenas, packed weights, BN statistics, job tables
    // parameters live in three arenas of one layout (weights, gradients, Adagrad accumulators): one update launch
    float *w_arena = nullptr, *g_arena = nullptr, *a_arena = nullptr;
    size_t arena_cap = 0, arena_used = 0;
    // split-fp16 convolutions: per-layer weight jobs (device copy), max |w| / exponent slots
    std::vector<amt_convh_pack_job> jobs;
    amt_convh_pack_job *jobs_dev = nullptr;
    float *wmax = nullptr;
    int *sw = nullptr;
    int max_job_elems = 0;
    // per batch size (ensure_batch) -- besides every tensor's v and g: im2col / scratch image, column partials
    // (red2: the column sums of dz per workgroup, the bias gradient of the convolution in front), the head's outputs,
    // and amax = [2 jobs][capB] scratch rows + [2 tensors][capB] producer-measured per-window maxima
    DevBuf col, red0, red1, red2, amax, pred, loss_rows, dlogits;
    DevBuf part;                                  // split-K / weight-gradient partials, grown where they are needed
    int colsum_of = -1;                           // tensor whose gradient's column partials red2 holds (-1: none)
    int colsum_nwg = 0;
};

namespace {

int talloc(amt_trainer *t, size_t n, float **out, bool zero = false) {
    float *p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(float)) != hipSuccess) return AMT_E_NOMEM;
    t->allocs.push_back(p);
    if (zero) AMT_HIP_CHECK(hipMemset(p, 0, std::max<size_t>(n, 1) * sizeof(float)));
    *out = p;
    return AMT_OK;
}

// ---- the tape, from the topology (amt_rdcnn_topology.h) ----------------------------------------------------------------
int new_tensor(amt_trainer *t, int H, int W, int C) {
    Tensor x; x.H = H; x.W = W; x.C = C;
    t->tensors.push_back(x);
    return (int)t->tensors.size() - 1;
}
// n floats at blob offset off become the next parameter: a 256-byte aligned slice of the arenas
int add_param(amt_trainer *t, const float *wh, size_t off, size_t n, bool trainable, int *idx) {
    Param p;
    p.n = n; p.off = off; p.trainable = trainable;
    const size_t at = t->arena_used;
    if (at + n > t->arena_cap) return AMT_E_NOMEM;
    t->arena_used = (at + n + 63) & ~(size_t)63;
    p.w = t->w_arena + at;
    AMT_HIP_CHECK(hipMemcpy(p.w, wh + off, n * sizeof(float), hipMemcpyHostToDevice));
    if (trainable) { p.g = t->g_arena + at; p.acc = t->a_arena + at; }
    t->params.push_back(p);
    *idx = (int)t->params.size() - 1;
    return AMT_OK;
}
// a convolution over H x W positions, or a Dense layer as the 1 x 1 convolution over one position: kernel, bias, output tensor
int add_conv(amt_trainer *t, const float *wh, int in, int H, int W, int Cin, int Cout, int kh, int kw, size_t kernel_off,
             size_t bias_off, int *out) {
    Op o; o.kind = OP_CONV; o.in0 = in; o.H = H; o.W = W; o.Cin = Cin; o.Cout = Cout; o.kh = kh; o.kw = kw;
    o.is_input = std::find(t->inputs.begin(), t->inputs.end(), in) != t->inputs.end();
    TR_TRY(add_param(t, wh, kernel_off, (size_t)kh * kw * Cin * Cout, true, &o.p0));
    TR_TRY(add_param(t, wh, bias_off, Cout, true, &o.p1));
    *out = o.out = new_tensor(t, H, W, Cout);
    t->ops.push_back(o);
    return AMT_OK;
}
int add_bn(amt_trainer *t, const float *wh, size_t off, int in, int *out) {
    const int H = t->tensors[in].H, W = t->tensors[in].W, C = t->tensors[in].C;
    Op o; o.kind = OP_BN; o.in0 = in; o.Cout = C;
    int *const idx[4] = {&o.p0, &o.p1, &o.p2, &o.p3};          // gamma, beta: trainable; moving mean, variance: not
    for (int k = 0; k < 4; ++k) TR_TRY(add_param(t, wh, off + (size_t)k * C, C, k < 2, idx[k]));
    TR_TRY(talloc(t, C, &o.bmu));
    TR_TRY(talloc(t, C, &o.binv));
    TR_TRY(talloc(t, C, &o.bvar));
    *out = o.out = new_tensor(t, H, W, C);
    t->ops.push_back(o);
    return AMT_OK;
}
int add_sigmoid(amt_trainer *t, int in) {
    const Tensor x = t->tensors[in];
    Op o; o.kind = OP_SIGMOID; o.in0 = in; o.out = new_tensor(t, x.H, x.W, x.C);
    t->ops.push_back(o);
    return o.out;
}
int add_pool(amt_trainer *t, int in, int ph, int pw, int is_max) {
    const Tensor x = t->tensors[in];
    Op o; o.kind = OP_POOL; o.in0 = in; o.is_max = is_max; o.kh = ph; o.kw = pw; o.H = x.H; o.W = x.W; o.Cin = x.C;
    o.out = new_tensor(t, x.H / ph, x.W / pw, x.C);
    t->ops.push_back(o);
    return o.out;
}

int build_tape(amt_trainer *t, const RdTopology &tp, const float *wh) {
    const amt_rdcnn_desc &d = t->d;
    std::vector<int> tails;
    for (int tw = 0; tw < d.n_towers; ++tw) {
        int cur = new_tensor(t, d.in_h[tw], d.in_w[tw], 1);
        t->inputs.push_back(cur);
        int src = cur;                                        // where the next shortcut starts
        for (int i = 0; i < d.conv_layers; ++i) {
            const RdLayer &l = tp.layers[(size_t)tw * d.conv_layers + i];
            TR_TRY(add_conv(t, wh, cur, l.H, l.W, l.cin, l.cout, l.kh, l.kw, l.kernel, l.bias, &cur));
            TR_TRY(add_bn(t, wh, l.bn, cur, &cur));
            cur = add_sigmoid(t, cur);
            if (l.residual) {
                int a = src;
                if (l.sc_proj) TR_TRY(add_conv(t, wh, a, l.sH, l.sW, l.sC, l.cout, 1, 1, l.sc_kernel, l.sc_bias, &a));
                if (l.sc_pool) a = add_pool(t, a, l.sc_ph, l.sc_pw, 0);
                if (l.sc_bn) TR_TRY(add_bn(t, wh, l.sc_bnorm, a, &a));
                Op ad; ad.kind = OP_ADD; ad.in0 = a; ad.in1 = cur; ad.out = new_tensor(t, l.H, l.W, l.cout);
                t->ops.push_back(ad);
                TR_TRY(add_bn(t, wh, l.res_bn, ad.out, &cur));
                src = cur;
            }
            if (l.pool_after) cur = add_pool(t, cur, l.ph, l.pw, 1);
        }
        tails.push_back(cur);
    }
    t->flat = tp.flat;
    t->t_flat = new_tensor(t, 1, 1, tp.flat);
    for (int tw = 0; tw < d.n_towers; ++tw) {
        Op f; f.kind = OP_FLATTEN; f.in0 = tails[tw]; f.out = t->t_flat; f.flat_off = tp.flat_off[tw];
        t->ops.push_back(f);
    }
    int h = -1;
    TR_TRY(add_conv(t, wh, t->t_flat, 1, 1, tp.flat, d.dense_units, 1, 1, tp.d1_kernel, tp.d1_bias, &h));
    h = add_sigmoid(t, h);
    TR_TRY(add_conv(t, wh, h, 1, 1, d.dense_units, d.output_classes, 1, 1, tp.d2_kernel, tp.d2_bias, &t->t_logits));
    return AMT_OK;
}

// BatchNormalizations on the fused passes, with the sigmoid behind them folded in
void choose_fused_bn(amt_trainer *t) {
    for (size_t i = 0; i < t->ops.size(); ++i) {
        Op &o = t->ops[i];
        if (!t->opt.fused_bn || o.kind != OP_BN) continue;
        const int C = o.Cout;
        if (C < 4 || C > 1024 || (C & (C - 1)) != 0) continue;
        o.bn_fused = true;
        if (i + 1 < t->ops.size() && t->ops[i + 1].kind == OP_SIGMOID && t->ops[i + 1].in0 == o.out) {
            o.sig_out = t->ops[i + 1].out;
            t->ops[i + 1].skip = true;
        }
    }
}
// convolutions the split-fp16 kernels cover: plans, packed-weight storage and the weight-preparation jobs
int choose_fast_convs(amt_trainer *t) {
    int njobs = 0;
    for (Op &o : t->ops) {
        if (!t->opt.fast || o.kind != OP_CONV || (o.kh == 1 && o.kw == 1)) continue;
        if (amt_convh_plan_init(&o.fplan, o.kh, o.kw, o.Cin, o.Cout, o.H, o.W) != AMT_OK) continue;
        o.job = njobs++;
        o.fast_bwd = !o.is_input && amt_convh_plan_init(&o.bplan, o.kh, o.kw, o.Cout, o.Cin, o.H, o.W) == AMT_OK;
    }
    if (!njobs) return AMT_OK;
    float *tmp = nullptr;
    TR_TRY(talloc(t, njobs, &t->wmax, true));
    TR_TRY(talloc(t, njobs, &tmp, true));
    t->sw = reinterpret_cast<int *>(tmp);
    t->jobs.resize(njobs);
    for (Op &o : t->ops) {
        if (o.job < 0) continue;
        float *a = nullptr, *b = nullptr;
        TR_TRY(talloc(t, (amt_convh_packed_bytes(&o.fplan) + 3) / 4, &a));
        if (o.fast_bwd) TR_TRY(talloc(t, (amt_convh_packed_bytes(&o.bplan) + 3) / 4, &b));
        o.wp_f = a; o.wp_b = b;
        amt_convh_pack_job &j = t->jobs[o.job];
        j.w = t->params[o.p0].w; j.packed_fwd = a; j.packed_bwd = b;
        j.wmax = t->wmax + o.job; j.sw = t->sw + o.job;
        j.ntap = o.kh * o.kw; j.Cin = o.Cin; j.Cout = o.Cout;
        t->max_job_elems = std::max(t->max_job_elems, j.ntap * j.Cin * j.Cout);
    }
    float *jd = nullptr;
    const size_t jb = (size_t)njobs * sizeof(amt_convh_pack_job);
    TR_TRY(talloc(t, (jb + 3) / 4, &jd));
    AMT_HIP_CHECK(hipMemcpy(jd, t->jobs.data(), jb, hipMemcpyHostToDevice));
    t->jobs_dev = reinterpret_cast<amt_convh_pack_job *>(jd);
    return AMT_OK;
}

int trainer_init(amt_trainer *t, const RdTopology &tp, const float *wh) {
    const amt_rdcnn_desc &d = t->d;
    // upper bound of the slices' padding: 8 parameters per convolution (kernel, bias, BN x 2 incl. shortcut) + the head
    const size_t nparams = (size_t)d.n_towers * (size_t)d.conv_layers * 16 + 64;
    t->arena_cap = tp.total + 64 * nparams;
    TR_TRY(talloc(t, t->arena_cap, &t->w_arena, true));
    TR_TRY(talloc(t, t->arena_cap, &t->g_arena, true));
    TR_TRY(talloc(t, t->arena_cap, &t->a_arena, true));
    if (t->acc0 > 0.f) {
        std::vector<float> a0(t->arena_cap, t->acc0);
        AMT_HIP_CHECK(hipMemcpy(t->a_arena, a0.data(), a0.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    TR_TRY(build_tape(t, tp, wh));
    choose_fused_bn(t);
    return choose_fast_convs(t);
}

size_t bnf_rows_wg(int C) { return (size_t)(1024 / C) * BNF_RPT; }
int bnf_nwg(size_t M, int C) { return (int)((M + bnf_rows_wg(C) - 1) / bnf_rows_wg(C)); }

// storage for B windows: every per-batch buffer grows (and frees what it held) when a larger batch arrives
int ensure_batch(amt_trainer *t, int B) {
    if (B <= t->capB) return AMT_OK;
    t->capB = 0;                                  // a regrowth that fails half-way leaves no batch size valid
    size_t col_need = 0, red_need = 0;
    int maxC = 1;
    for (Tensor &x : t->tensors) {
        TR_TRY(x.v.reserve(x.numel(B)));
        TR_TRY(x.g.reserve(x.numel(B)));
        col_need = std::max(col_need, x.numel(B));
    }
    for (const Op &o : t->ops) {
        if (o.kind == OP_CONV) col_need = std::max(col_need, (size_t)B * o.H * o.W * o.kh * o.kw * o.Cin);
        if (o.kind == OP_CONV || o.kind == OP_BN) maxC = std::max(maxC, o.Cout);     // column sums over Cout
        if (o.kind == OP_BN) {
            if (o.bn_fused) red_need = std::max(red_need, (size_t)bnf_nwg(t->tensors[o.in0].numel(B) / o.Cout, o.Cout) * o.Cout);
        }
    }
    red_need = std::max(red_need, (size_t)CR_SPLIT * maxC);
    TR_TRY(t->col.reserve(col_need));
    TR_TRY(t->red0.reserve(red_need));
    TR_TRY(t->red1.reserve(red_need));
    TR_TRY(t->red2.reserve(red_need));
    // per-window maxima: two scratch rows per split-fp16 layer (operands no producer measured) + two per tensor.  The
    // tensors' rows are the only pointers kept INTO a per-batch buffer: derived here, after every growth
    TR_TRY(t->amax.reserve((2 * t->jobs.size() + 2 * t->tensors.size()) * (size_t)B));
    float *base = t->amax + 2 * t->jobs.size() * (size_t)B;
    for (Tensor &x : t->tensors) { x.am_slot = base; x.gam_slot = base + B; base += 2 * (size_t)B; }
    const int K = t->d.output_classes;
    TR_TRY(t->pred.reserve((size_t)B * K));
    TR_TRY(t->loss_rows.reserve(B));
    TR_TRY(t->dlogits.reserve((size_t)B * K));
    t->capB = B;
    return AMT_OK;
}

// ---- shared launches ----------------------------------------------------------------------------------------------------
// GEMM dispatch with split over the contraction when the output grid is small
int gemm(amt_trainer *t, bool TA, bool TB, const float *A, int lda, const float *B, int ldb, float *C, int ldc,
         int M, int N, int K, const float *bias, hipStream_t st) {
    const int wn = N <= 32 ? 1 : 2;
    const int tm = 32 * (4 / wn), tn = 32 * wn;
    const int gx = (N + tn - 1) / tn, gy = (M + tm - 1) / tm;
    int Z = 1;
    const long tiles = (long)gx * gy;
    if (tiles < 512 && K > 4 * TG_KC) Z = (int)std::min<long>((512 + tiles - 1) / tiles, (K + 4 * TG_KC - 1) / (4 * TG_KC));
    Z = std::min(Z, 256);
    int kslice = ((K + Z - 1) / Z + TG_KC - 1) / TG_KC * TG_KC;
    Z = (K + kslice - 1) / kslice;
    float *part = nullptr;
    if (Z > 1) {
        TR_TRY(t->part.reserve((size_t)Z * M * N));
        part = t->part;
    }
    if (TA && TB) return AMT_E_UNSUPPORTED;
    auto kern = TA ? (wn == 1 ? tgemm_kernel<true, false, 1> : tgemm_kernel<true, false, 2>)
              : TB ? (wn == 1 ? tgemm_kernel<false, true, 1> : tgemm_kernel<false, true, 2>)
                   : (wn == 1 ? tgemm_kernel<false, false, 1> : tgemm_kernel<false, false, 2>);
    kern<<<dim3(gx, gy, Z), 256, 0, st>>>(A, lda, B, ldb, C, ldc, M, N, K, kslice, bias, part);
    if (Z > 1) splitk_reduce_kernel<<<grid1((size_t)M * N), 256, 0, st>>>(part, Z, C, ldc, M, N, bias);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

int colreduce(amt_trainer *t, const float *x, const float *z, const float *mu, const float *inv, size_t M, int C, int mode,
              float *out0, float *out1, hipStream_t st) {
    // ~64 rows per row-lane and split, between 8 splits and enough workgroups to cover the chip twice
    int nsplit = (int)std::min<size_t>(CR_SPLIT, std::max<size_t>(8, M / 512));
    nsplit = (nsplit + 7) & ~7;
    colreduce_kernel<<<dim3((C + 31) / 32, nsplit), 256, 0, st>>>(x, z, mu, inv, M, C, mode, nsplit, t->red0, t->red1);
    colreduce_final_kernel<<<(C + 31) / 32, 256, 0, st>>>(t->red0, t->red1, C, 1.0f / (float)M, mode, nsplit, out0, out1);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

// weight gradient without im2col (wgrad_kernel): KH x 16 kernels on 32-multiples of channels
bool wgrad_direct_ok(const Op &o) { return o.kw == 16 && o.Cin % 32 == 0 && o.Cout % 32 == 0 && o.W >= 16; }
int wgrad_direct(amt_trainer *t, const Op &o, const float *x, const float *dz, float *dW, int B, hipStream_t st) {
    WgArgs a;
    a.x = x; a.dz = dz; a.B = B; a.H = o.H; a.W = o.W; a.Cin = o.Cin; a.Cout = o.Cout; a.KH = o.kh;
    a.pt = (o.kh - 1) / 2; a.pl = (o.kw - 1) / 2;
    a.nseg = (o.W + 191) / 192;
    a.seg = ((o.W + a.nseg - 1) / a.nseg + 1) & ~1;
    a.ntiles = B * o.H * a.nseg;
    const int ngroups = o.kh * (o.Cin / 32) * (o.Cout / 32);
    const int P = std::max(1, std::min(a.ntiles, 512 / ngroups));
    const size_t nW = (size_t)o.kh * o.kw * o.Cin * o.Cout;
    TR_TRY(t->part.reserve((size_t)P * nW));
    a.part = t->part;
    const size_t lds = (size_t)(2 * a.seg + 15) * 32 * sizeof(float);
    wgrad_kernel<16><<<dim3(P, ngroups), 256, lds, st>>>(a);
    splitk_reduce_kernel<<<grid1(nW), 256, 0, st>>>(t->part, P, dW, o.Cout, o.kh * o.kw * o.Cin, o.Cout, nullptr);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

// layers too small to fill the chip stay on the GEMM path (a handful of workgroups walking the whole contraction one
// after the other is slower than the split-K GEMM)
bool fast_now(const amt_trainer *t, const Op &o, int B) { return o.job >= 0 && (size_t)B * o.H * o.W >= t->opt.fast_min_m; }

// the convolution's input as the GEMM's row operand: the activation itself (1 x 1) or its im2col image in col
const float *conv_rows(amt_trainer *t, const Op &o, const float *x, int B, hipStream_t st) {
    if (o.kh == 1 && o.kw == 1) return x;
    const size_t M = (size_t)B * o.H * o.W;
    im2col_kernel<<<(unsigned)std::min<size_t>(M, 1u << 20), 256, 0, st>>>(x, (size_t)o.H * o.W * o.Cin, B, o.H, o.W, o.Cin, o.kh, o.kw, t->col);
    return t->col;
}
// per-window max |x| of a split-fp16 operand: what its producer measured, or one pass into scratch row `row` of amax
int operand_amax(amt_trainer *t, const float *measured, const float *x, size_t n, int B, int row, hipStream_t st, const float **am) {
    *am = measured;
    if (measured) return AMT_OK;
    float *scratch = t->amax + (size_t)row * B;
    *am = scratch;
    return amt_convh_absmax(x, n, B, scratch, st);
}

// ---- gradient hand-over ------------------------------------------------------------------------------------------------
// A kernel that can write "value (+ what is there)" asks claim() for the destination's own buffer and the addend (null on
// the first arrival); afterwards the tensor's gradient lives in its own buffer.
float *claim(amt_trainer *t, int id, const float **acc) {
    Tensor &x = t->tensors[id];
    *acc = x.g_set ? x.gptr : nullptr;
    x.gptr = x.g; x.g_set = true; x.gam = nullptr;
    return x.g;
}
// A kernel that can only write: launch(dst) runs it into the destination's own buffer on the first arrival, into col
// followed by an add on a later one
template <class F>
int write_or_add(amt_trainer *t, int id, size_t n, hipStream_t st, F launch) {
    const float *acc = nullptr;
    float *dst = claim(t, id, &acc);
    if (!acc) { launch(dst); return AMT_OK; }
    if (n > t->col.cap) return AMT_E_NOMEM;
    launch(t->col);
    add_kernel<<<grid1(n), 256, 0, st>>>(acc, t->col, n, dst);
    return AMT_OK;
}
// the gradient of tensor `id` is (also) the n floats at src: a view on the first arrival, a sum into the own buffer after
int give_view(amt_trainer *t, int id, const float *src, size_t n, hipStream_t st) {
    Tensor &x = t->tensors[id];
    if (!x.g_set) { x.gptr = const_cast<float *>(src); x.g_set = true; x.gam = nullptr; return AMT_OK; }
    add_kernel<<<grid1(n), 256, 0, st>>>(x.gptr, src, n, x.g);
    x.gptr = x.g; x.gam = nullptr;
    return AMT_OK;
}
// src is a scratch buffer that will be reused (copy on the first arrival, add into the own buffer after), or the own
// buffer itself, already written (first arrival only)
int give_copy(amt_trainer *t, int id, const float *src, size_t n, hipStream_t st) {
    Tensor &x = t->tensors[id];
    if (!x.g_set) {
        if (x.g != src) AMT_HIP_CHECK(hipMemcpyAsync(x.g, src, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    } else {
        add_kernel<<<grid1(n), 256, 0, st>>>(x.gptr, src, n, x.g);
    }
    x.gptr = x.g; x.g_set = true; x.gam = nullptr;
    return AMT_OK;
}

// ---- the ops: one forward and one backward per kind; gout = the gradient arriving at the op's output -------------------
int fwd_conv(amt_trainer *t, Op &o, const Step &s) {
    Tensor &in = t->tensors[o.in0], &out = t->tensors[o.out];
    const float *bias = t->params[o.p1].w;
    if (fast_now(t, o, s.B)) {
        const float *am = nullptr;
        TR_TRY(operand_amax(t, in.am, in.v, in.numel(1), s.B, 2 * o.job, s.st, &am));
        return amt_convh_run(&o.fplan, in.v, out.v, nullptr, s.B, o.wp_f, t->sw + o.job, bias, am, (o.kh - 1) / 2, (o.kw - 1) / 2, s.st);
    }
    const int M = s.B * o.H * o.W, Kc = o.kh * o.kw * o.Cin;
    return gemm(t, false, false, conv_rows(t, o, in.v, s.B, s.st), Kc, t->params[o.p0].w, o.Cout, out.v, o.Cout, M, o.Cout, Kc, bias, s.st);
}
int bwd_conv(amt_trainer *t, Op &o, const Step &s, const float *gout) {
    Tensor &in = t->tensors[o.in0], &out = t->tensors[o.out];
    const size_t M = (size_t)s.B * o.H * o.W, nin = in.numel(s.B);
    const int Kc = o.kh * o.kw * o.Cin;
    float *dW = t->params[o.p0].g, *db = t->params[o.p1].g;
    if (t->opt.wgrad_direct && wgrad_direct_ok(o) && M >= t->opt.fast_min_m) TR_TRY(wgrad_direct(t, o, in.v, gout, dW, s.B, s.st));
    else TR_TRY(gemm(t, true, false, conv_rows(t, o, in.v, s.B, s.st), Kc, gout, o.Cout, dW, o.Cout, Kc, o.Cout, (int)M, nullptr, s.st));
    // bias gradient: the column sums of dz -- per-workgroup partials are there when the BatchNormalization behind this
    // convolution just wrote dz
    if (t->colsum_of == o.out) {
        colreduce_final_kernel<<<(o.Cout + 31) / 32, 256, 0, s.st>>>(t->red2, t->red2, o.Cout, 1.0f / (float)M, 3, t->colsum_nwg, db, nullptr);
        t->colsum_of = -1;
    } else {
        TR_TRY(colreduce(t, gout, nullptr, nullptr, nullptr, M, o.Cout, 3, db, nullptr, s.st));
    }
    if (o.is_input) return AMT_OK;                              // no gradient wrt the network input
    if (o.fast_bwd && fast_now(t, o, s.B)) {
        // dX = correlation of dOut with the flipped, transposed kernel (mirror-image padding), written into the input's
        // gradient buffer, plus what the shortcut branch already handed to that tensor
        const float *am = nullptr, *acc = nullptr;
        TR_TRY(operand_amax(t, out.gam, gout, out.numel(1), s.B, 2 * o.job + 1, s.st, &am));
        float *dst = claim(t, o.in0, &acc);
        return amt_convh_run(&o.bplan, gout, dst, acc, s.B, o.wp_b, t->sw + o.job, nullptr, am, o.kh - 1 - (o.kh - 1) / 2,
                             o.kw - 1 - (o.kw - 1) / 2, s.st);
    }
    // dcol = dOut W^T (into col); a 1 x 1 kernel's (a Dense layer's) dcol is dX itself, any other is gathered back to the image
    TR_TRY(gemm(t, false, true, gout, o.Cout, t->params[o.p0].w, o.Cout, t->col, Kc, (int)M, Kc, o.Cout, nullptr, s.st));
    if (o.kh == 1 && o.kw == 1) return give_copy(t, o.in0, t->col, nin, s.st);
    // gathered into the input's own gradient buffer on the first arrival; on a later one into dOut's own buffer, dead
    // once both GEMMs above have read it, and added from there
    float *img = in.g;
    if (in.g_set) {
        if (gout != out.g || out.numel(s.B) < nin) return AMT_E_NOMEM;
        img = out.g;
    }
    col2im_kernel<<<(unsigned)std::min<size_t>(M, 1u << 20), 256, 0, s.st>>>(t->col, s.B, o.H, o.W, o.Cin, o.kh, o.kw, img);
    return give_copy(t, o.in0, img, nin, s.st);
}

// statistics the BatchNormalization normalises with, into o.bmu / o.binv: of the batch when training (o.bvar too; the
// moving statistics absorb them), the moving ones otherwise -- for the fused and the generic apply alike
int bn_statistics(amt_trainer *t, Op &o, const float *x, size_t M, const Step &s) {
    float *mov_mean = t->params[o.p2].w, *mov_var = t->params[o.p3].w;
    if (!s.training) {
        AMT_HIP_CHECK(hipMemcpyAsync(o.bmu, mov_mean, o.Cout * sizeof(float), hipMemcpyDeviceToDevice, s.st));
        inv_from_var_kernel<<<(o.Cout + 63) / 64, 64, 0, s.st>>>(mov_var, o.Cout, o.binv);
        return AMT_OK;
    }
    const float bessel = M > 1 ? (float)((double)M / ((double)M - 1.0)) : 1.0f;
    if (o.bn_fused) {
        const int nwg = bnf_nwg(M, o.Cout);
        bnf_stats_kernel<<<nwg, 256, 0, s.st>>>(x, M, o.Cout, t->red0, t->red1);
        bnf_stats_final_kernel<<<(o.Cout + 31) / 32, 256, 0, s.st>>>(t->red0, t->red1, M, o.Cout, (int)bnf_rows_wg(o.Cout), nwg, o.bmu,
                                                                     o.bvar, o.binv, mov_mean, mov_var, 1, bessel);
        return AMT_OK;
    }
    TR_TRY(colreduce(t, x, nullptr, nullptr, nullptr, M, o.Cout, 0, o.bmu, nullptr, s.st));
    TR_TRY(colreduce(t, x, nullptr, o.bmu, nullptr, M, o.Cout, 1, o.bvar, o.binv, s.st));
    moving_update_kernel<<<(o.Cout + 63) / 64, 64, 0, s.st>>>(mov_mean, mov_var, o.bmu, o.bvar, o.Cout, bessel);
    return AMT_OK;
}
int fwd_bn(amt_trainer *t, Op &o, const Step &s) {
    Tensor &in = t->tensors[o.in0];
    const size_t nin = in.numel(s.B), M = nin / o.Cout;
    const float *gamma = t->params[o.p0].w, *beta = t->params[o.p1].w;
    TR_TRY(bn_statistics(t, o, in.v, M, s));
    if (o.bn_fused) {
        Tensor &dst = t->tensors[o.sig_out >= 0 ? o.sig_out : o.out];
        bnf_act_kernel<<<bnf_nwg(M, o.Cout), 256, 0, s.st>>>(in.v, o.bmu, o.binv, gamma, beta, M, o.Cout, in.H * in.W,
                                                             o.sig_out >= 0 ? 1 : 0, dst.v, dst.am_slot);
        dst.am = dst.am_slot;
    } else {
        bn_apply_kernel<<<grid1(nin), 256, 0, s.st>>>(in.v, o.bmu, o.binv, gamma, beta, nin, o.Cout, t->tensors[o.out].v);
    }
    return AMT_OK;
}
int bwd_bn(amt_trainer *t, Op &o, const Step &s, const float *gout) {
    Tensor &in = t->tensors[o.in0];
    const size_t nin = in.numel(s.B), M = nin / o.Cout;
    const float *gamma = t->params[o.p0].w;
    float *dgamma = t->params[o.p0].g, *dbeta = t->params[o.p1].g;
    if (o.bn_fused) {
        // dgamma = sum dy zhat, dbeta = sum dy, with dy = dA a (1 - a) when the sigmoid is folded in
        const int nwg = bnf_nwg(M, o.Cout);
        const float *a = o.sig_out >= 0 ? t->tensors[o.sig_out].v.p : nullptr;
        bnf_bwd_reduce_kernel<<<nwg, 256, 0, s.st>>>(gout, a, in.v, o.bmu, o.binv, M, o.Cout, t->red0, t->red1);
        colreduce_final_kernel<<<(o.Cout + 31) / 32, 256, 0, s.st>>>(t->red0, t->red1, o.Cout, 1.0f / (float)M, 2, nwg, dbeta, dgamma);
        // A BatchNormalization's input feeds nothing else: build_tape puts one behind a convolution, behind a shortcut's
        // Add, or behind the projection / average pool of a shortcut (which has a BatchNormalization of its own only when
        // it has one of those).  So this is the first gradient to arrive there, and the kernel only writes.
        const float *acc = nullptr;
        float *dst = claim(t, o.in0, &acc);
        if (acc) return AMT_E_UNSUPPORTED;
        bnf_bwd_apply_kernel<<<nwg, 256, 0, s.st>>>(gout, a, in.v, o.bmu, o.binv, gamma, dbeta, dgamma, 1.0f / (float)M, M, o.Cout,
                                                    in.H * in.W, dst, t->red2, in.gam_slot);
        // red2 now holds this launch's column partials: the bias gradient of the convolution in front, if there is one
        // (any partials another convolution was still waiting for are gone)
        in.gam = in.gam_slot; t->colsum_of = o.in0; t->colsum_nwg = nwg;
        return AMT_OK;
    }
    // generic path: dy -> scratch, two column sums, dz
    if (nin > t->col.cap) return AMT_E_NOMEM;
    AMT_HIP_CHECK(hipMemcpyAsync(t->col, gout, nin * sizeof(float), hipMemcpyDeviceToDevice, s.st));
    TR_TRY(colreduce(t, t->col, in.v, o.bmu, o.binv, M, o.Cout, 2, dbeta, dgamma, s.st));
    bn_backward_kernel<<<grid1(nin), 256, 0, s.st>>>(t->col, in.v, o.bmu, o.binv, gamma, dbeta, dgamma, 1.0f / (float)M, nin, o.Cout, 1, t->col);
    return give_copy(t, o.in0, t->col, nin, s.st);
}

int fwd_sigmoid(amt_trainer *t, Op &o, const Step &s) {
    Tensor &in = t->tensors[o.in0];
    sigmoid_fwd_kernel<<<grid1(in.numel(s.B)), 256, 0, s.st>>>(in.v, in.numel(s.B), t->tensors[o.out].v);
    return AMT_OK;
}
int bwd_sigmoid(amt_trainer *t, Op &o, const Step &s, const float *gout) {
    const size_t n = t->tensors[o.in0].numel(s.B);
    const float *a = t->tensors[o.out].v;
    return write_or_add(t, o.in0, n, s.st, [&](float *dst) { sigmoid_bwd_kernel<<<grid1(n), 256, 0, s.st>>>(gout, a, n, dst); });
}

int fwd_add(amt_trainer *t, Op &o, const Step &s) {
    Tensor &in = t->tensors[o.in0];
    add_kernel<<<grid1(in.numel(s.B)), 256, 0, s.st>>>(in.v, t->tensors[o.in1].v, in.numel(s.B), t->tensors[o.out].v);
    return AMT_OK;
}
int bwd_add(amt_trainer *t, Op &o, const Step &s, const float *gout) {
    const size_t n = t->tensors[o.in0].numel(s.B);
    TR_TRY(give_view(t, o.in0, gout, n, s.st));
    return give_view(t, o.in1, gout, n, s.st);
}

int fwd_pool(amt_trainer *t, Op &o, const Step &s) {
    Tensor &in = t->tensors[o.in0], &out = t->tensors[o.out];
    pool_fwd_kernel<<<grid1(out.numel(s.B)), 256, 0, s.st>>>(in.v, s.B, o.H, o.W, o.Cin, o.kh, o.kw, o.is_max, out.v, out.numel(1));
    out.am = in.am;                             // a max / average of values bounded by the window's maximum stays bounded by it
    return AMT_OK;
}
int bwd_pool(amt_trainer *t, Op &o, const Step &s, const float *gout) {
    Tensor &in = t->tensors[o.in0], &out = t->tensors[o.out];
    const size_t n = in.numel(s.B);
    return write_or_add(t, o.in0, n, s.st, [&](float *dst) {
        pool_bwd_kernel<<<grid1(n), 256, 0, s.st>>>(gout, out.numel(1), in.v, s.B, o.H, o.W, o.Cin, o.kh, o.kw, o.is_max, dst);
    });
}

int fwd_flatten(amt_trainer *t, Op &o, const Step &s) {
    Tensor &in = t->tensors[o.in0];
    copy_rows_kernel<<<grid1(in.numel(s.B)), 256, 0, s.st>>>(in.v, in.numel(1), t->tensors[o.out].v + o.flat_off, (size_t)t->flat, s.B, in.numel(1));
    return AMT_OK;
}
int bwd_flatten(amt_trainer *t, Op &o, const Step &s, const float *gout) {
    // rows of the dense input's gradient -> this tower's last activation (written straight into its grad)
    Tensor &in = t->tensors[o.in0];
    copy_rows_kernel<<<grid1(in.numel(s.B)), 256, 0, s.st>>>(gout + o.flat_off, (size_t)t->flat, in.g, in.numel(1), s.B, in.numel(1));
    in.gptr = in.g; in.g_set = true;
    return AMT_OK;
}

struct OpFns {
    int (*fwd)(amt_trainer *, Op &, const Step &);
    int (*bwd)(amt_trainer *, Op &, const Step &, const float *gout);
};
const OpFns OP_TABLE[OP_KINDS] = {   // indexed by OpKind
    {fwd_conv, bwd_conv}, {fwd_bn, bwd_bn}, {fwd_sigmoid, bwd_sigmoid}, {fwd_add, bwd_add},
    {fwd_pool, bwd_pool}, {fwd_flatten, bwd_flatten}};

// AMT_TRAIN_TRACE: synchronise and report after every op (a diagnostic for locating a failing launch)
void trace_op(const amt_trainer *t, const char *phase, size_t op_no, const Op &o, hipStream_t st) {
    if (!t->opt.trace) return;
    const hipError_t e = hipStreamSynchronize(st);
    fprintf(stderr, "[amt_train] %s op %d kind %d H %d W %d Cin %d Cout %d k %dx%d : %s\n", phase, (int)op_no, (int)o.kind, o.H, o.W,
            o.Cin, o.Cout, o.kh, o.kw, hipGetErrorString(e));
    fflush(stderr);
}

}  // namespace

extern "C" {

int amt_trainer_destroy(amt_trainer *t) {
    if (!t) return AMT_OK;
    for (float *p : t->allocs) (void)hipFree(p);
    for (Tensor &x : t->tensors) { x.v.release(); x.g.release(); }
    for (DevBuf *b : {&t->col, &t->red0, &t->red1, &t->red2, &t->amax, &t->pred, &t->loss_rows, &t->dlogits, &t->part}) b->release();
    delete t;
    return AMT_OK;
}

int amt_trainer_create(amt_trainer **out, const amt_rdcnn_desc *desc, const float *wh, size_t n_floats, float lr,
                       float epsilon, float initial_accumulator) {
    if (!out || !desc || !wh) return AMT_E_INVALID;
    RdTopology tp;
    if (amt_rdcnn_topology(*desc, &tp) != AMT_OK || tp.total != n_floats || n_floats == 0) return AMT_E_SHAPE;
    if (!tp.shortcut_ok) return AMT_E_UNSUPPORTED;
    amt_trainer *t = new amt_trainer();
    t->d = *desc;
    t->blob_floats = tp.total;
    if (lr > 0.f) t->lr = lr;
    if (epsilon > 0.f) t->eps = epsilon;
    t->acc0 = initial_accumulator > 0.f ? initial_accumulator : 0.f;
    const int rc = trainer_init(t, tp, wh);       // the status of what failed: AMT_E_NOMEM an allocation, AMT_E_HIP a copy
    if (rc != AMT_OK) { amt_trainer_destroy(t); return rc; }
    *out = t;
    return AMT_OK;
}

int amt_trainer_step(amt_trainer *t, const float *const *x, const float *y, int B, int update, float *loss_host,
                     float *pred_out, void *stream) {
    if (!t || !x || !y || B <= 0) return AMT_E_INVALID;
    for (size_t i = 0; i < t->inputs.size(); ++i) if (!x[i]) return AMT_E_INVALID;
    const Step s{B, update != 0, (hipStream_t)stream};
    const int K = t->d.output_classes;
    TR_TRY(ensure_batch(t, B));
    for (size_t i = 0; i < t->inputs.size(); ++i) {
        Tensor &in = t->tensors[t->inputs[i]];
        AMT_HIP_CHECK(hipMemcpyAsync(in.v, x[i], in.numel(B) * sizeof(float), hipMemcpyDeviceToDevice, s.st));
    }
    // per-step state: the measured maxima, where each gradient lives, whose column partials red2 holds
    AMT_HIP_CHECK(hipMemsetAsync(t->amax, 0, t->amax.cap * sizeof(float), s.st));
    for (Tensor &x_ : t->tensors) { x_.am = nullptr; x_.gam = nullptr; x_.g_set = false; x_.gptr = nullptr; }
    t->colsum_of = -1;
    if (!t->jobs.empty()) {
        // the weights moved in the last update: measure their range and lay them out for the split-fp16 kernels again
        // (two launches for every layer)
        const int nj = (int)t->jobs.size();
        AMT_HIP_CHECK(hipMemsetAsync(t->wmax, 0, nj * sizeof(float), s.st));
        TR_TRY(amt_convh_pack_all(t->jobs_dev, nj, t->max_job_elems, s.st));
    }
    // ---------------- forward ----------------------------------------------------------------
    for (size_t i = 0; i < t->ops.size(); ++i) {
        Op &o = t->ops[i];
        if (o.skip) continue;                                    // a sigmoid folded into the BatchNormalization in front
        TR_TRY(OP_TABLE[o.kind].fwd(t, o, s));
        trace_op(t, "fwd", i, o, s.st);
    }
    AMT_LAUNCH_CHECK();
    // ---------------- loss --------------------------------------------------------------------
    loss_kernel<<<(B + 63) / 64, 64, 0, s.st>>>(t->tensors[t->t_logits].v, y, B, K, t->pred, t->dlogits, t->loss_rows);
    if (pred_out) AMT_HIP_CHECK(hipMemcpyAsync(pred_out, t->pred, (size_t)B * K * sizeof(float), hipMemcpyDeviceToDevice, s.st));
    if (loss_host) {
        std::vector<float> rows(B);
        AMT_HIP_CHECK(hipMemcpyAsync(rows.data(), t->loss_rows, B * sizeof(float), hipMemcpyDeviceToHost, s.st));
        AMT_HIP_CHECK(hipStreamSynchronize(s.st));
        double sum = 0;
        for (float v : rows) sum += v;
        *loss_host = (float)(sum / B);
    }
    if (!update) return AMT_OK;
    // ---------------- backward ----------------------------------------------------------------
    TR_TRY(give_view(t, t->t_logits, t->dlogits, (size_t)B * K, s.st));
    for (size_t i = t->ops.size(); i-- > 0;) {
        Op &o = t->ops[i];
        if (o.skip) continue;
        const Tensor &from = t->tensors[o.kind == OP_BN && o.sig_out >= 0 ? o.sig_out : o.out];   // whose gradient arrives here
        if (!from.g_set) continue;                               // no gradient reaches this op
        trace_op(t, "bwd-enter", i, o, s.st);
        TR_TRY(OP_TABLE[o.kind].bwd(t, o, s, from.gptr));
    }
    AMT_LAUNCH_CHECK();
    // ---------------- update -------------------------------------------------------------------
    adagrad_kernel<<<grid1(t->arena_used), 256, 0, s.st>>>(t->w_arena, t->g_arena, t->a_arena, t->arena_used, t->lr, t->eps);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

static int copy_out(amt_trainer *t, float *host, size_t n, bool grads) {
    if (!t || !host) return AMT_E_INVALID;
    if (t->blob_floats != n) return AMT_E_SHAPE;
    AMT_HIP_CHECK(hipDeviceSynchronize());
    for (const Param &p : t->params) {
        if (grads && !p.trainable) memset(host + p.off, 0, p.n * sizeof(float));
        else AMT_HIP_CHECK(hipMemcpy(host + p.off, grads ? p.g : p.w, p.n * sizeof(float), hipMemcpyDeviceToHost));
    }
    return AMT_OK;
}
int amt_trainer_get_weights(amt_trainer *t, float *weights_host, size_t n_floats) { return copy_out(t, weights_host, n_floats, false); }
int amt_trainer_get_grads(amt_trainer *t, float *grads_host, size_t n_floats) { return copy_out(t, grads_host, n_floats, true); }

}  // extern "C"
