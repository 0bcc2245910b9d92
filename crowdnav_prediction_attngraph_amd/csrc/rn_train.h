// rn_train.h -- kernels of the robot-node sequence's training path (cn_rn_seq_fwd / cn_rn_seq_bwd in policy.hip) that are not GEMMs:
// the value / log-probability head on given actions and its backward, the fixed-order row reduction of their partials, and
// robot_linear.0's weight gradient.  Part of policy.hip's translation unit.
#pragma once
#include "rn_chain.h"

namespace {

// critic_linear + DiagGaussian.log_probs of GIVEN actions (model.py:82-90, distributions.py:36-44): one wavefront per sample
// NS = O / 64 strides of the 64 lanes over the O = human_node_output_size trunk features (4 at the default 256, up to 8)
template <int NS>
__global__ __launch_bounds__(256) void rn_head_fwd_kernel(int B, const float *__restrict__ ac, const float *__restrict__ wv, const float *__restrict__ bv,
                                                          const float *__restrict__ wm, const float *__restrict__ bm, const float *__restrict__ logstd,
                                                          const float *__restrict__ actions, float *__restrict__ value, float *__restrict__ logp)
{
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= B) return;
    constexpr int O = 64 * NS;
    const float *a = ac + (size_t)e * (2 * O), *c = a + O;
    float sv = 0.f, s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int d = lane + 64 * k;
        sv += c[d] * wv[d]; s0 += a[d] * wm[d]; s1 += a[d] * wm[O + d];
    }
    sv = wv_sum(sv); s0 = wv_sum(s0); s1 = wv_sum(s1);
    if (lane == 0) {
        value[e] = sv + bv[0];
        const float mean0 = s0 + bm[0], mean1 = s1 + bm[1], ls0 = logstd[0], ls1 = logstd[1];
        logp[e] = rn_gauss_logp(actions[2 * e], actions[2 * e + 1], mean0, mean1, ls0, ls1, expf(ls0), expf(ls1));
    }
}

// Backward of the heads AND of the second trunk layers' tanh: from d_value [B], d_logp [B]
//   d_mean_j = d_logp (a_j - mean_j) / sd_j^2 ; d_logstd_j += d_logp ((a_j - mean_j)^2 / sd_j^2 - 1)
//   d2[:, 0:O]   = (d_mean_0 wm[0] + d_mean_1 wm[1]) (1 - actor^2) ;  d2[:, O:2 O] = d_value wv (1 - critic^2)
// and the heads' own weight gradients (they are reductions over all B samples into 3 O + 5 numbers): every workgroup keeps its sums in
// registers and writes ONE partial row; rn_reduce_rows_kernel adds the rows in order (deterministic).
constexpr int rn_head_cols(int O) { return 3 * O + 8; } // d fm_w[0] | d fm_w[1] | d cl_w | d fm_b (2) d cl_b d logstd (2) pad (3)
constexpr int RN_HEAD_COLS = rn_head_cols(256);         // the default output size
template <int NS>
__global__ __launch_bounds__(256) void rn_head_bwd_kernel(int B, const float *__restrict__ ac, const float *__restrict__ wv, const float *__restrict__ wm,
                                                          const float *__restrict__ bm, const float *__restrict__ logstd, const float *__restrict__ actions,
                                                          const float *__restrict__ d_value, const float *__restrict__ d_logp, float *__restrict__ d2,
                                                          float *__restrict__ partials)
{
    constexpr int O = 64 * NS, COLS = rn_head_cols(O);
    __shared__ float red[4][COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float w0[NS], w1[NS], wc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) { const int d = lane + 64 * k; w0[k] = wm[d]; w1[k] = wm[O + d]; wc[k] = wv[d]; }
    const float ls0 = logstd[0], ls1 = logstd[1];
    const float iv0 = expf(-2.0f * ls0), iv1 = expf(-2.0f * ls1);
    float g0[NS], g1[NS], gc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) g0[k] = g1[k] = gc[k] = 0.f;
    float sb0 = 0.f, sb1 = 0.f, sbc = 0.f, sl0 = 0.f, sl1 = 0.f;
    for (int e = blockIdx.x * 4 + wave; e < B; e += gridDim.x * 4) {
        const float *a = ac + (size_t)e * (2 * O), *c = a + O;
        float av[NS], cv[NS], s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int k = 0; k < NS; ++k) { const int d = lane + 64 * k; av[k] = a[d]; cv[k] = c[d]; s0 += av[k] * w0[k]; s1 += av[k] * w1[k]; }
        s0 = wv_sum(s0); s1 = wv_sum(s1);
        const float dv = d_value[e], dl = d_logp[e];
        const float e0 = actions[2 * e] - (s0 + bm[0]), e1 = actions[2 * e + 1] - (s1 + bm[1]);
        const float dm0 = dl * e0 * iv0, dm1 = dl * e1 * iv1;
        float *o = d2 + (size_t)e * (2 * O);
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int d = lane + 64 * k;
            o[d] = (dm0 * w0[k] + dm1 * w1[k]) * (1.0f - av[k] * av[k]);
            o[O + d] = dv * wc[k] * (1.0f - cv[k] * cv[k]);
            g0[k] += dm0 * av[k]; g1[k] += dm1 * av[k]; gc[k] += dv * cv[k];
        }
        sb0 += dm0; sb1 += dm1; sbc += dv; sl0 += dl * (e0 * e0 * iv0 - 1.0f); sl1 += dl * (e1 * e1 * iv1 - 1.0f);
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) { const int d = lane + 64 * k; red[wave][d] = g0[k]; red[wave][O + d] = g1[k]; red[wave][2 * O + d] = gc[k]; }
    if (lane == 0) {
        float *q = &red[wave][3 * O];
        q[0] = sb0; q[1] = sb1; q[2] = sbc; q[3] = sl0; q[4] = sl1; q[5] = q[6] = q[7] = 0.f;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < COLS; j += 256)
        partials[(size_t)blockIdx.x * COLS + j] = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
}

// NS = O / 64 is a template parameter (register arrays, the LDS row): one instantiation per output size of the device box
#define RN_HEAD_DISPATCH(NSV, CALL) \
    switch (NSV) { case 1: { constexpr int NS = 1; CALL; } break; case 2: { constexpr int NS = 2; CALL; } break; case 3: { constexpr int NS = 3; CALL; } break; \
                   case 4: { constexpr int NS = 4; CALL; } break; case 5: { constexpr int NS = 5; CALL; } break; case 6: { constexpr int NS = 6; CALL; } break; \
                   case 7: { constexpr int NS = 7; CALL; } break; default: { constexpr int NS = 8; CALL; } break; }

// out[j] = sum over the rows of part[R][Cn], in a fixed order: a workgroup owns 16 columns, its sixteen thread groups each walk every
// sixteenth row (independent loads) and meet in LDS as a fixed binary tree.  rl_layout: the columns are robot_linear's [10][256] partials
// (9 weights + bias, feature innermost) and land in dW [256,9] / db [256] (out = dW, out2 = db).
__global__ __launch_bounds__(256) void rn_reduce_rows_kernel(int R, int Cn, const float *__restrict__ part, float *__restrict__ out, float *__restrict__ out2,
                                                             int rl_layout)
{
    __shared__ float red[16][17];
    const int c = threadIdx.x & 15, g = threadIdx.x >> 4, j = blockIdx.x * 16 + c;
    float s = 0.f;
    if (j < Cn)
        for (int r = g; r < R; r += 16) s += part[(size_t)r * Cn + j];
    red[g][c] = s;
    __syncthreads();
    if (g == 0 && j < Cn) {
        float t[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) t[k] = red[k][c];
#pragma unroll
        for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
            for (int k = 0; k < w; ++k) t[k] = t[k] + t[k + w];
        if (!rl_layout) out[j] = t[0];
        else { const int q = j >> 8, n = j & 255; if (q < 9) out[n * 9 + q] = t[0]; else out2[n] = t[0]; }
    }
}

// robot_linear.0's weight gradient: dW [256,9] and db [256] from drs [B,256] (already gated by the ReLU) and the 9 inputs
// (temporal_edges 2 | robot_node 7).  thread = output feature; every workgroup writes one partial [10][256] (9 weights + bias, feature innermost)
__global__ __launch_bounds__(256) void rn_rl_wgrad_kernel(int B, const float *__restrict__ drs, const float *__restrict__ temporal,
                                                          const float *__restrict__ robot_node, float *__restrict__ partials)
{
    const int n = threadIdx.x;
    float acc[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int e = blockIdx.x; e < B; e += gridDim.x) {
        const float d = drs[(size_t)e * 256 + n];
        acc[0] += d * temporal[e * 2]; acc[1] += d * temporal[e * 2 + 1];
#pragma unroll
        for (int q = 0; q < 7; ++q) acc[2 + q] += d * robot_node[e * 7 + q];
        acc[9] += d;
    }
#pragma unroll
    for (int q = 0; q < 10; ++q) partials[((size_t)blockIdx.x * 10 + q) * 256 + n] = acc[q];
}

} // namespace
