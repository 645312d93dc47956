// f32 MFMA convolution of the RDCNN forward (amt_rdcnn.hip, conv mode 0), and the launch parameters all of its
// convolution kernels share.
//
// Data layout in HBM: activations NHWC f32, [B][H][W][C]; the flatten order of
// Keras (H, W, C) is then the memory order, so Dense consumes it as is.
//
// Conv kernel (Cin multiple of 32): one 256-thread workgroup computes
// 128*MT output positions x Cout channels.  GEMM view: M = positions,
// N = Cout, K = (dy, dx, cin).  v_mfma_f32_32x32x2_f32 (f32 in, f32 acc: a
// k-ordered fmaf chain per (tap, 32-channel chunk), the chunks' sums added in
// tap order) -- the contraction the north star puts on MFMA while keeping
// float parity with the CPU.
//   * the input tile incl. the conv halo (explicit zeros = Keras "same"
//     padding, asymmetric for even kernels) is staged once per 32-channel
//     chunk into LDS as [pos][33] (pad 1 float: A-fragment reads hit 32
//     distinct banks);
//   * weights are pre-arranged on the host as [cchunk][tap][c][j][nt] so a
//     (tap, chunk) slab is one linear copy into a double-buffered LDS slab
//     and a lane's B fragments for all N-tiles are one ds_read_b32/b64/b128;
//   * one barrier per tap; 16 k-steps x MT x NT MFMAs between barriers;
//   * epilogue: acc*s1+t1 -> sigmoid -> (+shortcut)*s2+t2 -> coalesced NHWC
//     stores (a store instruction = two full 128-B channel rows).
#pragma once

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define RD_CC 32           // channels per staged chunk
#define RD_CSTRIDE 33      // LDS floats per staged position

struct ConvParams {
    const float *in;  size_t in_win_stride;      // [B][H][W][CIN]
    float *out;       size_t out_win_stride;     // [B][H][W][COUT]
    const float *sc;  size_t sc_win_stride;      // shortcut tensor (same shape as out) or null
    const float *w;                              // pre-arranged weights
    const float *s1, *t1, *s2, *t2;              // folded BN (s2/t2 null if no residual)
    int B, H, W;
    int TH, TW, NWIN;                            // workgroup tile
    int tiles_h, tiles_w;
    int cout_total;                              // channels of the output tensor (>= the kernel's COUT
                                                 // when the layer is split over blockIdx.y N-slices)
    // rank-1 shortcut (conv_f16x3s_kernel): the first residual block projects the ONE-channel network
    // input with a 1x1 kernel + BN (RDCNN.py:328-334); instead of materialising that [H][W][COUT]
    // tensor the epilogue forms (x * w_c) * s_c + t_c itself -- the operations of proj_kernel
    const float *sc1 = nullptr; size_t sc1_win_stride = 0;      // [B][H][W] (null: not used)
    const float *sc1_w = nullptr, *sc1_s = nullptr, *sc1_t = nullptr;   // [COUT]
    int pad_t = 0, pad_l = 0;                    // TRAIN form of conv_f16x3s_kernel only: rows / columns of padding before the image
};

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + __expf(-v)); }

template <int KH, int KW, int CIN, int COUT, int MT>
__global__ __launch_bounds__(256) void conv_mfma_kernel(ConvParams p) {
    constexpr int NT = COUT / 32;
    constexpr int NCHUNK = CIN / RD_CC;
    constexpr int NTAPS = KH * KW;
    constexpr int PCAP = 128 * MT;               // positions per workgroup
    constexpr int PAD_T = (KH - 1) / 2, PAD_L = (KW - 1) / 2;
    constexpr int WSLAB = RD_CC * COUT;           // floats per (tap, chunk) weight slab
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *wbuf = smem;                           // [2][WSLAB]
    int *pos_sp = reinterpret_cast<int *>(smem + 2 * WSLAB);   // [PCAP] spatial index or -1
    int *pos_win = pos_sp + PCAP;                 // [PCAP] global window
    float *in_lds = reinterpret_cast<float *>(pos_win + PCAP); // [POSIN][33]

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int THin = p.TH + KH - 1, TWin = p.TW + KW - 1;
    // block -> (window group, tile row, tile col)
    int bid = blockIdx.x;
    const int tc = bid % p.tiles_w; bid /= p.tiles_w;
    const int tr = bid % p.tiles_h; bid /= p.tiles_h;
    const int win0 = bid * p.NWIN;
    const int r0 = tr * p.TH, c0 = tc * p.TW;
    const int ptile = p.TH * p.TW;

    for (int q = tid; q < PCAP; q += 256) {
        const int w_ = q / ptile, rem = q - w_ * ptile;
        const int r = rem / p.TW, c = rem - r * p.TW;
        const bool ok = w_ < p.NWIN && (win0 + w_) < p.B && (r0 + r) < p.H && (c0 + c) < p.W;
        pos_sp[q] = ok ? (r0 + r) * p.W + (c0 + c) : -1;
        pos_win[q] = win0 + w_;
    }
    // per-lane LDS base (floats) of the A fragment for each of this wave's M-tiles
    int abase[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        int q = (wid * MT + mt) * 32 + (lane & 31);
        int w_ = q / ptile, rem = q - w_ * ptile;
        int r = rem / p.TW, c = rem - r * p.TW;
        if (w_ >= p.NWIN) { w_ = 0; r = 0; c = 0; }       // padding rows of the tile: any valid address
        abase[mt] = ((w_ * THin + r) * TWin + c) * RD_CSTRIDE + (lane >> 5);
    }
    f32x16 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mt][nt][e] = 0.f;

    constexpr int WV4 = WSLAB / 4 / 256;          // float4 per thread per slab (1, 2 or 4)
    static_assert(WSLAB % (4 * 256) == 0, "slab split");
    // N-slice of this workgroup (layers whose output-tile grid cannot fill the chip are split
    // over blockIdx.y into COUT-wide channel slices, each with its own weight block)
    const int cout_off = blockIdx.y * COUT;
    const float4 *wg4 = reinterpret_cast<const float4 *>(p.w + (size_t)blockIdx.y * ((size_t)CIN * NTAPS * COUT));

    for (int ch = 0; ch < NCHUNK; ++ch) {
        __syncthreads();                          // previous chunk fully consumed
        // ---- stage the input tile (32 channels) with its zero halo -------------
        {
            const int c4 = tid & 7;               // float4 within the 32 channels
            const int cl = tid >> 3;              // column lane 0..31
            for (int wr = 0; wr < p.NWIN * THin; ++wr) {
                const int w_ = wr / THin, ri = wr - w_ * THin;
                const int gr = r0 - PAD_T + ri;
                const int gw = win0 + w_;
                const bool rok = gr >= 0 && gr < p.H && gw < p.B;
                const float *src = p.in + (size_t)gw * p.in_win_stride +
                                   ((size_t)gr * p.W) * CIN + ch * RD_CC + c4 * 4;
                float *dst = in_lds + (size_t)wr * TWin * RD_CSTRIDE + c4 * 4;
                for (int ci = cl; ci < TWin; ci += 32) {
                    const int gc = c0 - PAD_L + ci;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (rok && gc >= 0 && gc < p.W)
                        v = *reinterpret_cast<const float4 *>(src + (size_t)gc * CIN);
                    float *d = dst + ci * RD_CSTRIDE;
                    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
                }
            }
        }
        // ---- first weight slab of this chunk ---------------------------------
        {
            const float4 *src = wg4 + (size_t)(ch * NTAPS) * (WSLAB / 4);
            float4 *dst = reinterpret_cast<float4 *>(wbuf);
#pragma unroll
            for (int i = 0; i < WV4; ++i) dst[tid + i * 256] = src[tid + i * 256];
        }
        __syncthreads();
        int cur = 0;
        for (int dy = 0; dy < KH; ++dy) {
            for (int dx = 0; dx < KW; ++dx) {
                const int tap = dy * KW + dx;
                float4 wpre[WV4];
                const bool more = tap + 1 < NTAPS;
                if (more) {
                    const float4 *src = wg4 + (size_t)(ch * NTAPS + tap + 1) * (WSLAB / 4);
#pragma unroll
                    for (int i = 0; i < WV4; ++i) wpre[i] = src[tid + i * 256];
                }
                const int tapoff = (dy * TWin + dx) * RD_CSTRIDE;
                const float *wb = wbuf + cur * WSLAB + ((lane >> 5) * 32 + (lane & 31)) * NT;
                // blocked summation: the 32 products of one (tap, chunk) go through a fresh accumulator (an fmaf
                // chain of length 32 inside the matrix pipe) which is then added to the running sum -- 64 + 32
                // roundings on the critical path of a K = 2048 contraction instead of 2048.  A single chain over
                // all of K (round 1-2) sat 11x farther from the float64 result than numpy's blocked GEMM on the
                // timing head at N = 2048 (profiles/r02/rdcnn_error_vs_f64.json); OpenBLAS blocks K the same way.
                f32x16 part[MT][NT];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                        for (int e = 0; e < 16; ++e) part[mt][nt][e] = 0.f;
#pragma unroll
                for (int cp = 0; cp < RD_CC / 2; ++cp) {
                    float a[MT];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) a[mt] = in_lds[abase[mt] + tapoff + 2 * cp];
                    float bfr[NT];
                    const float *wrow = wb + (2 * cp) * 32 * NT;
                    if constexpr (NT == 1) {
                        bfr[0] = wrow[0];
                    } else if constexpr (NT == 2) {
                        const float2 t2 = *reinterpret_cast<const float2 *>(wrow);
                        bfr[0] = t2.x; bfr[1] = t2.y;
                    } else {
                        const float4 t4 = *reinterpret_cast<const float4 *>(wrow);
                        bfr[0] = t4.x; bfr[1] = t4.y; bfr[2] = t4.z; bfr[3] = t4.w;
                    }
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
                            part[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                                a[mt], bfr[nt], part[mt][nt], 0, 0, 0);
                }
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                        for (int e = 0; e < 16; ++e) acc[mt][nt][e] = __fadd_rn(acc[mt][nt][e], part[mt][nt][e]);
                if (more) {
                    float4 *dst = reinterpret_cast<float4 *>(wbuf + (cur ^ 1) * WSLAB);
#pragma unroll
                    for (int i = 0; i < WV4; ++i) dst[tid + i * 256] = wpre[i];
                }
                __syncthreads();
                cur ^= 1;
            }
        }
    }
    // ---- epilogue ---------------------------------------------------------------
    const int j = lane & 31;
    const int CT = p.cout_total;
    float s1[NT], t1[NT], s2[NT], t2[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        s1[nt] = p.s1[cout_off + nt * 32 + j]; t1[nt] = p.t1[cout_off + nt * 32 + j];
        s2[nt] = p.s2 ? p.s2[cout_off + nt * 32 + j] : 1.f;
        t2[nt] = p.t2 ? p.t2[cout_off + nt * 32 + j] : 0.f;
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
            const int q = (wid * MT + mt) * 32 + row;
            const int sp = pos_sp[q];
            if (sp < 0) continue;
            const int gw = pos_win[q];
            float *o = p.out + (size_t)gw * p.out_win_stride + (size_t)sp * CT + cout_off + j;
            const float *scp = p.sc ? p.sc + (size_t)gw * p.sc_win_stride + (size_t)sp * CT + cout_off + j : nullptr;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                float v = sigmoidf_(acc[mt][nt][e] * s1[nt] + t1[nt]);
                if (scp) v = (v + scp[nt * 32]) * s2[nt] + t2[nt];
                o[nt * 32] = v;
            }
        }
    }
}
