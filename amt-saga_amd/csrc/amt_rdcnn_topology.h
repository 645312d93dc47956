// THE topology walk of the RDCNN graph (RDCNN.py:176-233 of the reference, _add_shortcut :312-335), host only: what every
// conv layer of every tower looks like and where its parameters sit in the canonical weight blob (rdcnn.py pack_weights).
// amt_rdcnn_param_count, amt_rdcnn_create and amt_trainer_create all read this one description; the rules --
//   * the filters start at 32 and double after every feature_expand_frequency-th layer,
//   * a shortcut closes at every residual_frequency-th layer, from the previous closing point (or the tower's input),
//   * the shortcut has a 1 x 1 projection only if the channel count changed, an average pool only if H or W changed, and
//     its own BatchNormalization only if either changed,
//   * the max pool comes after the block,
//   * blob order per layer: kernel, bias, bn | shortcut kernel, bias, bn | residual bn; then dense1, dense2 (kernel, bias) --
// are stated here and nowhere else in C++.  A BatchNormalization group is gamma, beta, mean, variance: 4 x C floats.
#pragma once
#include "amt_saga.h"
#include <stddef.h>
#include <vector>

struct RdLayer {
    int tower;
    int H, W, cin, cout, kh, kw;         // the convolution ('same' padding: H x W in and out)
    bool residual;                       // a shortcut closes behind this layer
    int sH, sW, sC;                      //   its source: the previous closing point or the tower's input
    bool sc_proj, sc_pool, sc_bn;        //   1 x 1 projection sC -> cout / average pool (sc_ph, sc_pw) / BN of its own
    int sc_ph, sc_pw;                    //   floor(sH / H), floor(sW / W): 1, 1 without a pool
    bool pool_after;                     // max pool (ph, pw) behind the block
    int ph, pw, oH, oW;                  //   dims the next layer sees (H, W without a pool)
    // float offsets in the canonical blob; groups the layer does not own stay 0 and are not to be read
    size_t kernel, bias, bn, sc_kernel, sc_bias, sc_bnorm, res_bn;
};
struct RdTopology {
    std::vector<RdLayer> layers;         // tower-major, conv_layers per tower
    int n_towers = 0;
    int out_h[2], out_w[2], out_c[2];    // each tower's last activation
    int flat_off[2];                     //   and its column in the dense input
    int flat = 0;
    size_t d1_kernel = 0, d1_bias = 0, d2_kernel = 0, d2_bias = 0;
    size_t total = 0;                    // floats of the whole blob
    bool shortcut_ok = true;             // false: some shortcut's valid average pool does not reproduce the main branch's
                                         // H x W (the count stands; both creates answer AMT_E_UNSUPPORTED)
};

// AMT_OK; AMT_E_INVALID for a tower count outside 1..2; AMT_E_UNSUPPORTED when a max pool collapses an activation.
static inline int amt_rdcnn_topology(const amt_rdcnn_desc &d, RdTopology *out) {
    if (d.n_towers < 1 || d.n_towers > 2) return AMT_E_INVALID;
    RdTopology tp;
    tp.n_towers = d.n_towers;
    size_t off = 0;
    auto take = [&off](size_t n) { const size_t at = off; off += n; return at; };
    for (int t = 0; t < d.n_towers; ++t) {
        int H = d.in_h[t], W = d.in_w[t], C = 1, fo = 32;
        int sH = H, sW = W, sC = 1;
        for (int i = 1; i <= d.conv_layers; ++i) {
            RdLayer l = {};
            l.tower = t;
            l.H = H; l.W = W; l.cin = C; l.cout = fo; l.kh = d.kh[t]; l.kw = d.kw[t];
            l.kernel = take((size_t)l.kh * l.kw * C * fo);
            l.bias = take(fo);
            l.bn = take(4 * (size_t)fo);
            C = fo;
            l.sc_ph = l.sc_pw = 1;
            if (d.residual_frequency > 0 && i % d.residual_frequency == 0) {
                l.residual = true;
                l.sH = sH; l.sW = sW; l.sC = sC;
                l.sc_proj = sC != C;
                l.sc_pool = sH != H || sW != W;
                l.sc_bn = l.sc_proj || l.sc_pool;
                if (l.sc_pool) {
                    l.sc_ph = sH / H; l.sc_pw = sW / W;                    // floor(sh1 / sh2), RDCNN.py:325-326
                    if (sH / l.sc_ph != H || sW / l.sc_pw != W) tp.shortcut_ok = false;
                }
                if (l.sc_proj) { l.sc_kernel = take((size_t)sC * C); l.sc_bias = take(C); }
                if (l.sc_bn) l.sc_bnorm = take(4 * (size_t)C);
                l.res_bn = take(4 * (size_t)C);
                sH = H; sW = W; sC = C;
            }
            if (d.pool_layer_frequency > 0 && i % d.pool_layer_frequency == 0) {
                l.pool_after = true;
                l.ph = d.pool_h[t]; l.pw = d.pool_w[t];
                H /= l.ph; W /= l.pw;
                if (H < 1 || W < 1) return AMT_E_UNSUPPORTED;
            }
            l.oH = H; l.oW = W;
            if (d.feature_expand_frequency > 0 && i % d.feature_expand_frequency == 0) fo *= 2;
            tp.layers.push_back(l);
        }
        tp.out_h[t] = H; tp.out_w[t] = W; tp.out_c[t] = C;
        tp.flat_off[t] = tp.flat;
        tp.flat += H * W * C;
    }
    tp.d1_kernel = take((size_t)tp.flat * d.dense_units);
    tp.d1_bias = take(d.dense_units);
    tp.d2_kernel = take((size_t)d.dense_units * d.output_classes);
    tp.d2_bias = take(d.output_classes);
    tp.total = off;
    *out = tp;
    return AMT_OK;
}
