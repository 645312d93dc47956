// The small layers of the RDCNN forward (amt_rdcnn.hip): first layer (VALU and matrix-pipe forms), shortcut
// projection, max-pool, Dense (+ its split-K reduction) and the output activation.
#pragma once

// ---- first layer (Cin = 1): direct convolution on the VALU ---------------------
// A workgroup walks row tiles of 256/COUT*4 output columns of one window row.  The
// input rows (with the zero halo) and all weights sit in LDS; thread = (column
// group, cout) computes 4 consecutive columns x 1 channel, so one weight read
// feeds 4 FMAs and the input reads are wave broadcasts.  Stores are coalesced NHWC.
struct Conv1Params {
    const float *in; size_t in_win_stride;       // [B][H][W]
    float *out; size_t out_win_stride;
    const float *sc; size_t sc_win_stride;
    const float *w;                              // [KH*KW][COUT]
    const float *s1, *t1, *s2, *t2;
    int B, H, W, KH, KW, COUT;
    float *amax_out = nullptr;                   // [B] max |output| per window (atomicMax; conv1_mfma_kernel) or null
};
#define C1_PPT 4
__global__ __launch_bounds__(256) void conv1_kernel(Conv1Params p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int ntap = p.KH * p.KW;
    const int groups = 256 / p.COUT;             // column groups per workgroup
    const int TWc = groups * C1_PPT;             // output columns per tile
    const int XW = TWc + p.KW - 1;               // staged input columns
    float *wl = smem;                            // [ntap][COUT]
    float *xt = smem + ntap * p.COUT;            // [KH][XW]
    for (int i = threadIdx.x; i < ntap * p.COUT; i += 256) wl[i] = p.w[i];
    const int pad_t = (p.KH - 1) / 2, pad_l = (p.KW - 1) / 2;
    const int co = threadIdx.x % p.COUT;
    const int pg = threadIdx.x / p.COUT;
    const int tiles_w = (p.W + TWc - 1) / TWc;
    const long total = (long)p.B * p.H * tiles_w;
    const float s1 = p.s1[co], t1 = p.t1[co];
    const float s2 = p.s2 ? p.s2[co] : 1.f, t2 = p.t2 ? p.t2[co] : 0.f;
    for (long tile = blockIdx.x; tile < total; tile += gridDim.x) {
        const int tc = (int)(tile % tiles_w);
        long rest = tile / tiles_w;
        const int r = (int)(rest % p.H);
        const int b = (int)(rest / p.H);
        const int c0 = tc * TWc;
        const float *x = p.in + (size_t)b * p.in_win_stride;
        __syncthreads();                         // previous tile consumed (and wl visible)
        for (int i = threadIdx.x; i < p.KH * XW; i += 256) {
            const int dy = i / XW, cx = i - dy * XW;
            const int gr = r + dy - pad_t, gc = c0 + cx - pad_l;
            xt[i] = (gr >= 0 && gr < p.H && gc >= 0 && gc < p.W) ? x[(size_t)gr * p.W + gc] : 0.f;
        }
        __syncthreads();
        float acc[C1_PPT];
#pragma unroll
        for (int q = 0; q < C1_PPT; ++q) acc[q] = 0.f;
        for (int dy = 0; dy < p.KH; ++dy) {
            const float *xr = xt + dy * XW + pg * C1_PPT;
            const float *wr = wl + dy * p.KW * p.COUT + co;
            for (int dx = 0; dx < p.KW; ++dx) {
                const float wv = wr[dx * p.COUT];
#pragma unroll
                for (int q = 0; q < C1_PPT; ++q) acc[q] = fmaf(xr[dx + q], wv, acc[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < C1_PPT; ++q) {
            const int c = c0 + pg * C1_PPT + q;
            if (c >= p.W) continue;
            const size_t sp = (size_t)r * p.W + c;
            float v = sigmoidf_(acc[q] * s1 + t1);
            if (p.sc) v = (v + p.sc[(size_t)b * p.sc_win_stride + sp * p.COUT + co]) * s2 + t2;
            p.out[(size_t)b * p.out_win_stride + sp * p.COUT + co] = v;
        }
    }
}

// ---- first layer on the matrix pipe (Cout = 32) ---------------------------------------------
// GEMM view: M = output positions, N = 32 filters, K = KH*KW taps; v_mfma_f32_32x32x2_f32 (f32
// in, f32 accumulate: the same k-ordered fmaf chain as conv1_kernel).  The whole [K][32] kernel
// lives in K/2 B-fragment registers per lane; an A fragment is one ds_read_b32 of the
// single-channel input tile (lane = position, lane half = the odd tap of a tap pair, i.e. the
// next column).  A workgroup (4 waves) owns a TH x TW tile of <= 512 positions = <= 16 M-tiles,
// wave w takes M-tiles w, w+4, ...; workgroups walk the tiles grid-stride.
#define C1M_PCAP 512
template <int KH, int KW>
__global__ __launch_bounds__(256) void conv1_mfma_kernel(Conv1Params p, int TH, int TW, int tiles_h,
                                                          int tiles_w) {
    constexpr int K = KH * KW, NK2 = K / 2;
    static_assert(K % 2 == 0 && KW % 2 == 0, "tap pairs share a kernel row");
    constexpr int PAD_T = (KH - 1) / 2, PAD_L = (KW - 1) / 2;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int RPW = TW + KW - 1, THin = TH + KH - 1;
    int *pos_rc = reinterpret_cast<int *>(smem);            // [PCAP] r | c << 16 (tile-local)
    int *pos_sp = pos_rc + C1M_PCAP;                         // [PCAP] global spatial index or -1
    float *tpatch = reinterpret_cast<float *>(pos_sp + C1M_PCAP);   // [4 waves][32][HX_TPITCH]
    float *xt = tpatch + 4 * 32 * HX_TPITCH;                 // [THin][RPW]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    float *tb = tpatch + wid * 32 * HX_TPITCH;
    const int c4 = (lane & 7) * 4;
    const int PT = TH * TW, nmt = (PT + 31) >> 5;
    for (int q = tid; q < C1M_PCAP; q += 256) {
        const int r = q / TW, c = q - r * TW;
        pos_rc[q] = q < PT ? (r | (c << 16)) : -1;
    }
    const int co = lane & 31;
    float bq[NK2];
#pragma unroll
    for (int i = 0; i < NK2; ++i) bq[i] = p.w[(2 * i + (lane >> 5)) * 32 + co];
    const float s1 = p.s1[co], t1 = p.t1[co];
    float4 s2v = make_float4(1.f, 1.f, 1.f, 1.f), t2v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.s2) s2v = *reinterpret_cast<const float4 *>(p.s2 + c4);
    if (p.t2) t2v = *reinterpret_cast<const float4 *>(p.t2 + c4);
    const long total = (long)p.B * tiles_h * tiles_w;
    for (long tile = blockIdx.x; tile < total; tile += gridDim.x) {
        const int tc = (int)(tile % tiles_w);
        const long rest = tile / tiles_w;
        const int tr = (int)(rest % tiles_h);
        const int b = (int)(rest / tiles_h);
        const int r0 = tr * TH, c0 = tc * TW;
        const float *x = p.in + (size_t)b * p.in_win_stride;
        __syncthreads();                                     // previous tile consumed (pos_rc visible)
        for (int i = tid; i < THin * RPW; i += 256) {
            const int ri = i / RPW, ci = i - ri * RPW;
            const int gr = r0 + ri - PAD_T, gc = c0 + ci - PAD_L;
            xt[i] = (gr >= 0 && gr < p.H && gc >= 0 && gc < p.W) ? x[(size_t)gr * p.W + gc] : 0.f;
        }
        for (int q = tid; q < C1M_PCAP; q += 256) {
            const int rc = pos_rc[q];
            const int r = r0 + (rc & 0xFFFF), c = c0 + (rc >> 16);
            pos_sp[q] = (rc >= 0 && r < p.H && c < p.W) ? r * p.W + c : -1;
        }
        __syncthreads();
        float tmax = 0.f;                                    // max |output| of this wave's share of the tile
        for (int mt = wid; mt < nmt; mt += 4) {
            const int rc = pos_rc[mt * 32 + (lane & 31)];
            const int abase = rc >= 0 ? (rc & 0xFFFF) * RPW + (rc >> 16) + (lane >> 5) : (lane >> 5);
            f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
            for (int i = 0; i < NK2; ++i) {
                constexpr int dummy = 0; (void)dummy;
                const int dy = (2 * i) / KW, dx = (2 * i) % KW;
                const float a = xt[abase + dy * RPW + dx];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bq[i], acc, 0, 0, 0);
            }
            // turn the 32 x 32 tile through a wave-private LDS patch: 16-byte stores, 4 channels per lane
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                tb[row * HX_TPITCH + co] = sigmoidf_(acc[e] * s1 + t1);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = (lane >> 3) + 8 * i;
                const int sp = pos_sp[mt * 32 + row];
                float4 v = *reinterpret_cast<const float4 *>(tb + row * HX_TPITCH + c4);
                if (sp < 0) continue;
                if (p.sc) {
                    const float4 sc = *reinterpret_cast<const float4 *>(p.sc + (size_t)b * p.sc_win_stride + (size_t)sp * 32 + c4);
                    v.x = (v.x + sc.x) * s2v.x + t2v.x; v.y = (v.y + sc.y) * s2v.y + t2v.y;
                    v.z = (v.z + sc.z) * s2v.z + t2v.z; v.w = (v.w + sc.w) * s2v.w + t2v.w;
                }
                tmax = fmaxf(tmax, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
                *reinterpret_cast<float4 *>(p.out + (size_t)b * p.out_win_stride + (size_t)sp * 32 + c4) = v;
            }
        }
        if (p.amax_out) {                                    // one window per tile
            tmax = wave_max(tmax);
            if (lane == 0) atomicMax(reinterpret_cast<int *>(p.amax_out) + b, __float_as_int(tmax));
        }
    }
}
// tile of <= 512 positions that needs the fewest 32-position M-tiles over the image

// ---- shortcut projection: BN(avgpool(conv1x1(x)))  (RDCNN.py:328-334) -----------
// The 1x1 convolution and the average pool commute; pooling first cuts the
// contraction work by the pool area.  A workgroup owns <= 64 output columns of one
// output row: phase 1 pools the inputs into LDS (coalesced over channels), phase 2
// contracts the pooled vectors with the [CIN][COUT] kernel (coalesced over cout).
struct ProjParams {
    const float *in; size_t in_win_stride;       // [B][H][W][CIN]
    float *out; size_t out_win_stride;           // [B][HO][WO][COUT]
    const float *w;                              // [CIN][COUT] or null (identity channels)
    const float *s, *t;                          // folded: out = s*(sum) + t  (bias inside t)
    int B, H, W, CIN, COUT, PH, PW, HO, WO;
};
#define PJ_TW 64
__global__ __launch_bounds__(256) void proj_kernel(ProjParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];   // [PJ_TW][CIN]
    const int wo0 = blockIdx.x * PJ_TW;
    const int ho = blockIdx.y, b = blockIdx.z;
    const int nwo = min(PJ_TW, p.WO - wo0);
    const float inv = 1.0f / (float)(p.PH * p.PW);
    const float *x = p.in + (size_t)b * p.in_win_stride;
    for (int i = threadIdx.x; i < nwo * p.CIN; i += 256) {
        const int wl = i / p.CIN, ci = i - wl * p.CIN;
        const int wo = wo0 + wl;
        float a = 0.f;
        for (int dy = 0; dy < p.PH; ++dy)
            for (int dx = 0; dx < p.PW; ++dx)
                a += x[((size_t)(ho * p.PH + dy) * p.W + (wo * p.PW + dx)) * p.CIN + ci];
        smem[i] = a * inv;
    }
    __syncthreads();
    // four consecutive output channels per thread: 16-byte weight loads and output stores
    float *o = p.out + (size_t)b * p.out_win_stride + ((size_t)ho * p.WO + wo0) * p.COUT;
    const int C4 = p.COUT >> 2;
    for (int i = threadIdx.x; i < nwo * C4; i += 256) {
        const int wl = i / C4, co = (i - wl * C4) << 2;
        float4 acc;
        if (p.w) {
            acc = make_float4(0.f, 0.f, 0.f, 0.f);
            const float *pv = smem + wl * p.CIN;
            for (int ci = 0; ci < p.CIN; ++ci) {
                const float4 wv = *reinterpret_cast<const float4 *>(p.w + (size_t)ci * p.COUT + co);
                const float a = pv[ci];
                acc.x = fmaf(a, wv.x, acc.x); acc.y = fmaf(a, wv.y, acc.y);
                acc.z = fmaf(a, wv.z, acc.z); acc.w = fmaf(a, wv.w, acc.w);
            }
        } else {
            acc = *reinterpret_cast<const float4 *>(smem + wl * p.CIN + co);
        }
        const float4 sv = *reinterpret_cast<const float4 *>(p.s + co);
        const float4 tv = *reinterpret_cast<const float4 *>(p.t + co);
        acc.x = acc.x * sv.x + tv.x; acc.y = acc.y * sv.y + tv.y;
        acc.z = acc.z * sv.z + tv.z; acc.w = acc.w * sv.w + tv.w;
        *reinterpret_cast<float4 *>(o + (size_t)wl * p.COUT + co) = acc;
    }
}

// ---- MaxPooling2D (valid, stride = pool) ------------------------------------------
__global__ __launch_bounds__(256) void maxpool_kernel(const float *__restrict__ in,
                                                       size_t in_win_stride, float *__restrict__ out,
                                                       size_t out_win_stride, int B, int H, int W,
                                                       int C, int PH, int PW, int HO, int WO) {
    // four channels per thread (C is a multiple of 32): 16-byte loads and stores
    const int C4 = C >> 2;
    const size_t total = (size_t)B * HO * WO * C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % C4) << 2;
        size_t r = i / C4;
        const int wo = (int)(r % WO); r /= WO;
        const int ho = (int)(r % HO);
        const int b = (int)(r / HO);
        const float *x = in + (size_t)b * in_win_stride;
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        for (int dy = 0; dy < PH; ++dy)
            for (int dx = 0; dx < PW; ++dx) {
                const float4 v = *reinterpret_cast<const float4 *>(
                    x + ((size_t)(ho * PH + dy) * W + (wo * PW + dx)) * C + c);
                m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
            }
        *reinterpret_cast<float4 *>(out + (size_t)b * out_win_stride + ((size_t)ho * WO + wo) * C + c) = m;
    }
}

// ---- Dense: C[M][N] = act(A[M][K] B[K][N] + bias[N]) on v_mfma_f32_32x32x2_f32 -----
// M = windows is small (<= 512 per chunk) and N = 300, so the grid of output tiles is
// tiny; to fill the chip a workgroup owns one 32x32 output tile and its 4 waves split K
// four ways (wave-private LDS staging, [32][33] pitch: conflict-free fragment reads), then
// the four partial tiles are summed through LDS in a fixed order (deterministic).  A long
// contraction (the 5120-wide flatten of the timing head) is additionally split over
// gridDim.z workgroups that write partial tiles; dense_reduce_kernel adds them in z order.
#define DN_KC 32
#define DN_KSPLIT 8
__global__ __launch_bounds__(256) void dense_kernel(const float *__restrict__ A, int K,
                                                     const float *__restrict__ Bm,
                                                     const float *__restrict__ bias, int N,
                                                     float *__restrict__ Cm, int M, int act,
                                                     float *__restrict__ part) {
    __shared__ float as[4][32 * 33];
    __shared__ float bs[4][DN_KC * 32];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
    const int KS = gridDim.z;
    const int Kz = ((K + KS - 1) / KS + 4 * DN_KC - 1) / (4 * DN_KC) * (4 * DN_KC);   // K range per workgroup
    const int kz1 = min(K, (int)(blockIdx.z + 1) * Kz);
    const int kq = Kz / 4;                                           // K range per wave, chunk aligned
    const int kbeg = blockIdx.z * Kz + wid * kq, kend = min(kz1, kbeg + kq);
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float *aw = as[wid], *bw = bs[wid];
    for (int k0 = 0; k0 < kq; k0 += DN_KC) {                         // same trip count in every wave
        __syncthreads();
        for (int i = lane; i < 32 * DN_KC; i += 64) {
            const int r = i / DN_KC, kk = i - r * DN_KC;
            const int k = kbeg + k0 + kk;
            aw[r * 33 + kk] = (m0 + r < M && k < kend) ? A[(size_t)(m0 + r) * K + k] : 0.f;
        }
        for (int i = lane; i < DN_KC * 32; i += 64) {
            const int kk = i >> 5, c = i & 31;
            const int k = kbeg + k0 + kk;
            bw[i] = (k < kend && n0 + c < N) ? Bm[(size_t)k * N + n0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < DN_KC; kk += 2) {
            const float a = aw[(lane & 31) * 33 + kk + (lane >> 5)];
            const float bv = bw[(kk + (lane >> 5)) * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc, 0, 0, 0);
        }
    }
    __syncthreads();
    // partial tiles -> LDS [wave][row][col(33)], then every thread sums 4 outputs
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        as[wid][row * 33 + (lane & 31)] = acc[e];
    }
    __syncthreads();
    for (int i = tid; i < 32 * 32; i += 256) {
        const int row = i >> 5, col = i & 31;
        const int m = m0 + row, n = n0 + col;
        if (m < M && n < N) {
            float v = ((as[0][row * 33 + col] + as[1][row * 33 + col]) +
                       (as[2][row * 33 + col] + as[3][row * 33 + col]));
            if (part) { part[((size_t)blockIdx.z * M + m) * N + n] = v; continue; }
            v += bias[n];
            if (act == 1) v = sigmoidf_(v);
            Cm[(size_t)m * N + n] = v;
        }
    }
}
__global__ void dense_reduce_kernel(const float *__restrict__ part, int KS, const float *__restrict__ bias,
                                    int N, float *__restrict__ Cm, int M, int act) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)M * N) return;
    float v = part[i];
    for (int z = 1; z < KS; ++z) v += part[(size_t)z * M * N + i];
    v += bias[i % N];
    if (act == 1) v = sigmoidf_(v);
    Cm[i] = v;
}

// ---- output activation: softmax (K > 1) or sigmoid + range scaling (K == 1) -------
__global__ void head_output_kernel(const float *__restrict__ logits, float *__restrict__ y, int B,
                                   int K, float lo, float hi) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float *l = logits + (size_t)b * K;
    float *o = y + (size_t)b * K;
    if (K == 1) {
        const float a = 1.0f / (1.0f + expf(-l[0]));
        o[0] = a * (hi - lo) + lo;                 // RDCNN.py:308-310 with out_func range [0,1]
    } else {
        float m = -INFINITY;
        for (int k = 0; k < K; ++k) m = fmaxf(m, l[k]);
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += expf(l[k] - m);
        for (int k = 0; k < K; ++k) o[k] = expf(l[k] - m) / s;
    }
}
