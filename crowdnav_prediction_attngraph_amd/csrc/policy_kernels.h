// policy_kernels.h -- the small kernels around the policy's GEMMs: row compaction (row_offsets_kernel, compact_visible_kernel,
// scatter_rows_kernel), the two narrow input layers (embed0_kernel, robot_embed_kernel), the GRU cell's pointwise part, the
// critic / DiagGaussian head and the weight folds of cn_policy_set_weights.  Part of policy.hip's translation unit.
#pragma once
#include "rn_chain.h"

namespace {

// Row compaction: row_off[e] = sum_{e' < e} nd(e'), nd = clamp(detected_human_num, 1, H); row_off[E] = number of live
// (env, human) rows.  Padded humans (index >= nd) only ever meet an exactly-zero robot-human attention weight, so the
// whole human-human block runs on live rows only.  Single block, Hillis-Steele scan over per-thread chunk sums.
// cls_cnt[2] / cls_list[2][E] (optional): the envs of the two rare big attention size classes (16 < nd <= 32, nd > 32);
// the order inside a bin is arbitrary (LDS atomics) and has no effect on any result (a unit writes only its own rows).
__global__ __launch_bounds__(1024) void row_offsets_kernel(int E, int H, const float *__restrict__ det, int *__restrict__ row_off,
                                                           unsigned long long *__restrict__ live_total, int *__restrict__ cls_cnt,
                                                           int *__restrict__ cls_list)
{
    __shared__ int part[1024];
    __shared__ int cnt[2];
    const int t = threadIdx.x;
    if (t < 2) cnt[t] = 0;
    const int chunk = (E + 1023) / 1024;
    const int lo = t * chunk, hi = min(lo + chunk, E);
    int sum = 0;
    for (int e = lo; e < hi; ++e) { int nd = (int)det[e]; nd = nd < 1 ? 1 : (nd > H ? H : nd); sum += nd; }
    part[t] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - sum; // exclusive prefix of this thread's chunk
    for (int e = lo; e < hi; ++e) {
        row_off[e] = run;
        int nd = (int)det[e]; nd = nd < 1 ? 1 : (nd > H ? H : nd);
        run += nd;
        if (cls_list && nd > 16) {
            const int c = nd <= 32 ? 0 : 1;
            cls_list[(size_t)c * E + atomicAdd(&cnt[c], 1)] = e;
        }
    }
    if (cls_cnt) {
        __syncthreads();
        if (t < 2) cls_cnt[t] = cnt[t];
    }
    if (t == 1023) {
        row_off[E] = part[1023];
        if (live_total) *live_total += (unsigned long long)part[1023]; // measurement aid: total live rows over the profiled launches
    }
}

// embedding_layer.0 (K = D <= 16) on live rows: out[row_off[e] + j][n] = relu(sum_d x[e][j][d] * W[n][d] + b[n]), n < 128
__global__ __launch_bounds__(128) void embed0_kernel(int E, int H, int D, const float *__restrict__ x, const float *__restrict__ W,
                                                     const float *__restrict__ b, const int *__restrict__ row_off, float *__restrict__ out)
{
    const int n = threadIdx.x;
    float w[16];
#pragma unroll
    for (int d = 0; d < 16; ++d) w[d] = d < D ? W[n * D + d] : 0.0f;
    const float bn = b[n];
    for (int e = blockIdx.x; e < E; e += gridDim.x) {
        const int r0 = row_off[e], nd = row_off[e + 1] - r0;
        for (int j = 0; j < nd; ++j) {
            const float *xr = x + ((size_t)e * H + j) * D;
            float acc = bn;
#pragma unroll
            for (int d = 0; d < 16; ++d)
                if (d < D) acc += xr[d] * w[d];
            out[(size_t)(r0 + j) * 128 + n] = fmaxf(acc, 0.0f);
        }
    }
}

// robot_linear.0: out[e][n] = relu(W[n][0:2] . temporal_edges[e] + W[n][2:9] . robot_node[e] + b[n]), n < 256
// (torch.cat((temporal_edges, robot_node), -1), selfAttn_srnn_temp_node.py:397)
__global__ __launch_bounds__(256) void robot_embed_kernel(int E, const float *__restrict__ temporal, const float *__restrict__ robot_node,
                                                          const float *__restrict__ W, const float *__restrict__ b, float *__restrict__ out)
{
    const int n = threadIdx.x;
    float w[9];
#pragma unroll
    for (int d = 0; d < 9; ++d) w[d] = W[n * 9 + d];
    const float bn = b[n];
    for (int e = blockIdx.x; e < E; e += gridDim.x) {
        float acc = bn;
        acc += temporal[e * 2] * w[0];
        acc += temporal[e * 2 + 1] * w[1];
#pragma unroll
        for (int d = 0; d < 7; ++d) acc += robot_node[e * 7 + d] * w[2 + d];
        out[(size_t)e * 256 + n] = fmaxf(acc, 0.0f);
    }
}

// args.sort_humans = False: the visible humans of a sample moved to the front (stable), the others behind them; detected = max(1, visible)
// (an all-invisible sample keeps human 0: selfAttn_srnn_temp_node.py:381-383).  One wavefront per sample, lane = human.
__global__ __launch_bounds__(64) void compact_visible_kernel(int B, int H, int D, const float *__restrict__ se, const uint8_t *__restrict__ vis,
                                                             float *__restrict__ out, float *__restrict__ det)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const bool isH = lane < H;
    unsigned long long m = __ballot(isH && vis[(size_t)b * H + (isH ? lane : 0)] != 0);
    if (m == 0ull) m = 1ull;
    const unsigned long long valid = H >= 64 ? ~0ull : ((1ull << H) - 1ull);
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const int cnt = __popcll(m);
    const bool v = (m >> lane) & 1ull;
    const int rank = v ? __popcll(m & below) : cnt + __popcll(~m & valid & below);
    if (isH) {
        const float *src = se + ((size_t)b * H + lane) * D;
        float *dst = out + ((size_t)b * H + rank) * D;
        for (int d = 0; d < D; ++d) dst[d] = src[d];
    }
    if (lane == 0) det[b] = (float)cnt;
}

// test tap: scatter the compacted [rows,256] activations back to [E,H,256] (zeros on padded humans)
__global__ __launch_bounds__(256) void scatter_rows_kernel(int E, int H, const float *__restrict__ src, const int *__restrict__ row_off,
                                                           float *__restrict__ dst)
{
    const int e = blockIdx.x, c = threadIdx.x;
    const int r0 = row_off[e], nd = row_off[e + 1] - r0;
    for (int j = 0; j < H; ++j) dst[((size_t)e * H + j) * 256 + c] = j < nd ? src[(size_t)(r0 + j) * 256 + c] : 0.0f;
}

// GRU cell pointwise part (PyTorch formulation, gate order r,z,n) with the done mask applied to h
// (rl/networks/srnn_model.py:43-46): gi = x W_ih^T + b_ih (bias already added), gh_raw = h W_hh^T (no bias, unmasked).
// One block per env, R threads (the hidden size, at most 256).
__global__ __launch_bounds__(256) void gru_pointwise_kernel(int E, int R, const float *__restrict__ gi, const float *__restrict__ gh_raw,
                                                            const float *__restrict__ b_hh, const float *__restrict__ h_in,
                                                            const float *__restrict__ masks, float *__restrict__ h_out)
{
    const int e = blockIdx.x, c = threadIdx.x;
    if (e >= E) return;
    const float m = masks[e];
    const float *gie = gi + (size_t)e * 3 * R, *ghe = gh_raw + (size_t)e * 3 * R;
    const float hr = m * ghe[c] + b_hh[c], hz = m * ghe[R + c] + b_hh[R + c], hn = m * ghe[2 * R + c] + b_hh[2 * R + c];
    const float r = 1.0f / (1.0f + expf(-(gie[c] + hr)));
    const float z = 1.0f / (1.0f + expf(-(gie[R + c] + hz)));
    const float n = tanhf(gie[2 * R + c] + r * hn);
    const float h = m * h_in[(size_t)e * R + c];
    h_out[(size_t)e * R + c] = (1.0f - z) * n + z * h;
}

// critic_linear + DiagGaussian head (model.py:64-72, distributions.py:36-44,76-95): one wavefront per env.
// ac [E,2O]: columns 0..O-1 actor features, O..2O-1 critic features (O = 256 by default, a multiple of 64).
__global__ __launch_bounds__(256) void gauss_head_kernel(int E, int O, const float *__restrict__ ac, int ld, const float *__restrict__ wv,
                                                         const float *__restrict__ bv, const float *__restrict__ wm,
                                                         const float *__restrict__ bm, const float *__restrict__ logstd,
                                                         const float *__restrict__ eps, float *__restrict__ value,
                                                         float *__restrict__ action, float *__restrict__ logp)
{
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E) return;
    const float *a = ac + (size_t)e * ld, *c = a + O;
    float sv = 0.f, s0 = 0.f, s1 = 0.f;
    for (int d = lane; d < O; d += 64) { // the same terms in the same order as the four unrolled steps this was at O = 256
        sv += c[d] * wv[d];
        s0 += a[d] * wm[d];
        s1 += a[d] * wm[O + d];
    }
    sv = wv_sum(sv); s0 = wv_sum(s0); s1 = wv_sum(s1);
    if (lane == 0) {
        value[e] = sv + bv[0];
        if (action) {
            float a0, a1;
            const float lp = rn_gauss_sample(s0 + bm[0], s1 + bm[1], logstd[0], logstd[1], eps != nullptr, eps ? eps[2 * e] : 0.0f, eps ? eps[2 * e + 1] : 0.0f,
                                             a0, a1);
            action[2 * e] = a0; action[2 * e + 1] = a1;
            logp[e] = lp;
        }
    }
}

// Weight folding: C[n][k] = scale * sum_j A[n][j] * B[j][k]  (fp64 accumulation), A [N,J], B [J,K]
__global__ void fold_mm_kernel(int N, int J, int K, const float *__restrict__ A, const float *__restrict__ B, float scale, float *__restrict__ C)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
    if (k >= K || n >= N) return;
    double acc = 0.0;
    for (int j = 0; j < J; ++j) acc += (double)A[(size_t)n * J + j] * (double)B[(size_t)j * K + k];
    C[(size_t)n * K + k] = (float)(acc * (double)scale);
}
// c[n] = scale * (sum_j A[n][j] * b[j] + b2[n])
__global__ void fold_bias_kernel(int N, int J, const float *__restrict__ A, const float *__restrict__ b, const float *__restrict__ b2,
                                 float scale, float *__restrict__ c)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double acc = b2[n];
    for (int j = 0; j < J; ++j) acc += (double)A[(size_t)n * J + j] * (double)b[j];
    c[n] = (float)(acc * (double)scale);
}

// C[N,K] = A^T B with A [J,N], B [J,K];  c[n] = sum_j A[j][n] * b[j]
__global__ void fold_mm_tn_kernel(int N, int J, int K, const float *__restrict__ A, const float *__restrict__ B, float *__restrict__ C)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
    if (k >= K || n >= N) return;
    double acc = 0.0;
    for (int j = 0; j < J; ++j) acc += (double)A[(size_t)j * N + n] * (double)B[(size_t)j * K + k];
    C[(size_t)n * K + k] = (float)acc;
}
__global__ void fold_bias_tn_kernel(int N, int J, const float *__restrict__ A, const float *__restrict__ b, float *__restrict__ c)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double acc = 0.0;
    for (int j = 0; j < J; ++j) acc += (double)A[(size_t)j * N + n] * (double)b[j];
    c[n] = (float)acc;
}

constexpr size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

} // namespace
