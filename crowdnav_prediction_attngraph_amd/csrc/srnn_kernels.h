// srnn_kernels.h -- the two kernels of the DS-RNN baseline's rollout forward (rl/networks/srnn_model.py:389-468), launched by srnn.hip:
//   srnn_edge_gru_kernel   both edge GRUs (srnn_model.py:418-433): encoder, mask * h, the two products as MFMA, the gates -- h' leaves once
//   srnn_node_kernel       everything behind the edge state (srnn_model.py:436-468 + the DiagGaussian head), a workgroup per 8 envs
#pragma once
#include "common.h"
#include "split_bf16.h"

namespace {

typedef float sr_f4 __attribute__((ext_vector_type(4)));

constexpr int SR_EMB = 64;              // edge embedding = K of W_ih
constexpr int SR_HID = 256;             // edge hidden = K of W_hh
constexpr int SR_K = SR_EMB + SR_HID;   // one A row: [ReLU(enc x) | mask * h]
constexpr int SR_TILE = 64;             // edge rows per workgroup
constexpr int SR_EDGE_THREADS = 512;    // 8 wavefronts, two 16-column blocks of hidden units each
constexpr int SR_LDH = SR_HID + 8;      // bf16 row stride of the mask * h planes: 528 B, 16-byte aligned, 16 rows' fragment reads spread over the banks
constexpr int SR_LDE = SR_EMB + 4;      // fp32 row stride of the embedding (split mode)
constexpr int SR_LDF = SR_K + 4;        // fp32 row stride of the exact mode's [embedding | mask * h]
// split mode: hi + lo planes of mask * h (67 584 B) + the fp32 embedding (17 408 B) = 84 992 B; exact mode: 64 * 324 * 4 = 82 944 B
constexpr size_t SR_EDGE_LDS = (size_t)2 * SR_TILE * SR_LDH * sizeof(__bf16) + (size_t)SR_TILE * SR_LDE * sizeof(float);

struct SrnnEdgeW {                      // one weight set (temporal or spatial edge GRU) of the handle's snapshot
    const float *enc_w, *enc_b;         // [64,din], [64]
    const float *w_ih, *w_hh;           // [768,64], [768,256] fp32 (exact mode)
    const float *b_ih, *b_hh;           // [768] each
    const __bf16 *hh_hi, *hh_lo;        // split planes of w_hh
    int din;
};

// What the training forward (srnn_train.hip) keeps of one step for the backward, per weight set and gathered row: the gates r, z, n and
// hn = W_hn (mask * h) + b_hn as four planes of 256, and the 64-wide post-ReLU embedding.  The rollout passes an empty one (SAVE = 0).
struct SrnnEdgeSave {
    float *gates_t, *gates_s;           // [rows of the set, 4, 256]
    float *emb_t, *emb_s;               // [rows of the set, 64]
};

__device__ __forceinline__ float sr_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// Rows are the E * (H + 1) edges, gathered per weight set: workgroups [0, tiles_t) take 64 temporal rows (env e, slot 0) each, the others 64
// spatial rows (env r / H, slot 1 + r % H).  A tile's A operand [64, 320] = [ReLU(enc x) | mask * h] is built once in LDS, the weights stream
// from the L2 straight into B fragments, and every wavefront owns two 16-column blocks of hidden units for all 64 rows with four accumulators
// per block: r and z over K = 64 + 256, W_in x over 64, W_hn h over 256.
//   W_hh (mask * h), K = 256: SPLIT = bf16 hi / lo planes (split_bf16.h) on v_mfma_f32_16x16x32_bf16 (lo*hi + hi*lo + hi*hi; each 16-byte B
//                    fragment is 8 consecutive k of one gate row); exact = v_mfma_f32_16x16x4_f32.  |h| < 1, so the split's 2^-17 relative
//                    error per term stays near 1e-6 absolute in the sum.
//   W_ih x, K = 64:  exact fp32 MFMA in BOTH modes.  The embedding is not bounded -- the observation pads unseen humans with 15 m, which
//                    gives embeddings of 10 .. 30 -- and as a bf16x3 product this K = 64 sum alone was 1.1e-4 off the reference at the bar
//                    of 1e-4.  At the fp32 MFMA rate its 64 columns cost as much as the split 256 (16 x 64 = 1024 vs 3 x 256 = 768 bf16
//                    k-columns); the kernel is bound by the weight stream, not by the MFMA pipe.
// edge_out may be edge_in itself: a tile reads its own rows only, all of them before the barrier except the element each lane re-reads in
// the epilogue right before it writes that same element.
// SAVE = 1 (the training forward): the same arithmetic, and every row also leaves its gates and its embedding in `sv`.
template <int SPLIT, int SAVE = 0>
__global__ __launch_bounds__(SR_EDGE_THREADS) void srnn_edge_gru_kernel(int E, int H, int tiles_t, SrnnEdgeW wt, SrnnEdgeW ws, const float *__restrict__ temporal,
                                                                        const float *__restrict__ spatial, const float *edge_in,
                                                                        const float *__restrict__ masks, float *edge_out, SrnnEdgeSave sv = SrnnEdgeSave{})
{
    extern __shared__ __attribute__((aligned(16))) char sr_smem[];
    __bf16 *xh = reinterpret_cast<__bf16 *>(sr_smem);                       // split mode: mask * h, hi and lo planes, then the embedding
    __bf16 *xl = xh + SR_TILE * SR_LDH;
    float *xf = reinterpret_cast<float *>(sr_smem);                         // exact mode: [embedding | mask * h] in fp32
    float *xe = SPLIT ? reinterpret_cast<float *>(xl + SR_TILE * SR_LDH) : xf;
    constexpr int lde = SPLIT ? SR_LDE : SR_LDF;
    const bool is_t = (int)blockIdx.x < tiles_t;
    const SrnnEdgeW w = is_t ? wt : ws;
    const long long nrows = is_t ? (long long)E : (long long)E * H;
    const long long r0 = (long long)(is_t ? blockIdx.x : blockIdx.x - tiles_t) * SR_TILE;
    const int tid = threadIdx.x;
    auto env_of = [&](long long r) { return is_t ? r : r / H; };
    auto edge_row = [&](long long r) { return is_t ? r * (H + 1) : (r / H) * (H + 1) + 1 + r % H; };   // row of the [E * (H+1), 256] state
    auto put_h = [&](int row, int col, float v) {
        if (SPLIT) {
            const __bf16 hi = (__bf16)v;
            xh[row * SR_LDH + col] = hi;
            xl[row * SR_LDH + col] = (__bf16)(v - (float)hi);
        } else {
            xf[row * SR_LDF + SR_EMB + col] = v;
        }
    };
    // ---- A tile: the encoder on the VALU (K = 2 or D), and mask * h; rows past the end are zero ----
    const float *xin = is_t ? temporal : spatial;
    const int din = w.din;
    for (int idx = tid; idx < SR_TILE * SR_EMB; idx += SR_EDGE_THREADS) {
        const int row = idx >> 6, c = idx & 63;
        float v = 0.0f;
        if (r0 + row < nrows) {
            const float *x = xin + (size_t)(r0 + row) * din;
            v = w.enc_b[c];
            for (int k = 0; k < din; ++k) v = fmaf(w.enc_w[c * din + k], x[k], v);
            v = fmaxf(v, 0.0f);
            if (SAVE) (is_t ? sv.emb_t : sv.emb_s)[(size_t)(r0 + row) * SR_EMB + c] = v;
        }
        xe[row * lde + c] = v;
    }
    for (int idx = tid; idx < SR_TILE * (SR_HID / 4); idx += SR_EDGE_THREADS) {
        const int row = idx >> 6, c4 = (idx & 63) * 4;
        sr_f4 h = {0.f, 0.f, 0.f, 0.f};
        if (r0 + row < nrows) {
            const float m = masks[env_of(r0 + row)];
            h = *reinterpret_cast<const sr_f4 *>(edge_in + (size_t)edge_row(r0 + row) * SR_HID + c4);
            h *= m;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) put_h(row, c4 + q, h[q]);
    }
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    for (int cbi = 0; cbi < 2; ++cbi) {
        const int col = (wave * 2 + cbi) * 16 + li;      // this lane's hidden unit (B column, C/D column)
        sr_f4 ar[4], az[4], ai[4], ah[4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) ar[rb] = az[rb] = ai[rb] = ah[rb] = sr_f4{0.f, 0.f, 0.f, 0.f};
        // W_ih x: exact fp32 in both modes
#pragma unroll 4
        for (int ks = 0; ks < SR_EMB / 4; ++ks) {
            const int k0 = ks * 4 + lk;
            float b[3];
#pragma unroll
            for (int g = 0; g < 3; ++g) b[g] = w.w_ih[(size_t)(g * SR_HID + col) * SR_EMB + k0];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const float a = xe[(rb * 16 + li) * lde + k0];
                ar[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[0], ar[rb], 0, 0, 0);
                az[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[1], az[rb], 0, 0, 0);
                ai[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[2], ai[rb], 0, 0, 0);
            }
        }
        if (SPLIT) {
            // W_hh (mask * h), one k-step of 32: B fragments of the three gate rows (hi and lo), then 9 MFMAs per 16-row block
#pragma unroll 2
            for (int ks = 0; ks < SR_HID / 32; ++ks) {
                const int k0 = ks * 32 + lk * 8;
                bf16x8 bh[3], bl[3];
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    const size_t o = (size_t)(g * SR_HID + col) * SR_HID + k0;
                    bh[g] = *reinterpret_cast<const bf16x8 *>(w.hh_hi + o);
                    bl[g] = *reinterpret_cast<const bf16x8 *>(w.hh_lo + o);
                }
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) {
                    const int o = (rb * 16 + li) * SR_LDH + k0;
                    const bf16x8 a_hi = *reinterpret_cast<const bf16x8 *>(&xh[o]);
                    const bf16x8 a_lo = *reinterpret_cast<const bf16x8 *>(&xl[o]);
                    ar[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo, bh[0], ar[rb], 0, 0, 0);
                    az[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo, bh[1], az[rb], 0, 0, 0);
                    ah[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo, bh[2], ah[rb], 0, 0, 0);
                    ar[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, bl[0], ar[rb], 0, 0, 0);
                    az[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, bl[1], az[rb], 0, 0, 0);
                    ah[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, bl[2], ah[rb], 0, 0, 0);
                    ar[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, bh[0], ar[rb], 0, 0, 0);
                    az[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, bh[1], az[rb], 0, 0, 0);
                    ah[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, bh[2], ah[rb], 0, 0, 0);
                }
            }
        } else {
#pragma unroll 4
            for (int ks = 0; ks < SR_HID / 4; ++ks) {
                const int k0 = ks * 4 + lk;
                float b[3];
#pragma unroll
                for (int g = 0; g < 3; ++g) b[g] = w.w_hh[(size_t)(g * SR_HID + col) * SR_HID + k0];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) {
                    const float a = xf[(rb * 16 + li) * SR_LDF + SR_EMB + k0];
                    ar[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[0], ar[rb], 0, 0, 0);
                    az[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[1], az[rb], 0, 0, 0);
                    ah[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[2], ah[rb], 0, 0, 0);
                }
            }
        }
        // ---- gates (torch's GRU, order r, z, n); C/D layout: column = lane & 15, row = 4 * (lane >> 4) + i ----
        const float br = w.b_ih[col] + w.b_hh[col], bz = w.b_ih[SR_HID + col] + w.b_hh[SR_HID + col];
        const float bin = w.b_ih[2 * SR_HID + col], bhn = w.b_hh[2 * SR_HID + col];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long long r = r0 + rb * 16 + lk * 4 + i;
                if (r < nrows) {
                    const size_t o = (size_t)edge_row(r) * SR_HID + col;
                    const float h = edge_in[o] * masks[env_of(r)];
                    const float rg = sr_sigmoid(ar[rb][i] + br), zg = sr_sigmoid(az[rb][i] + bz);
                    const float ng = tanhf(ai[rb][i] + bin + rg * (ah[rb][i] + bhn));
                    edge_out[o] = (1.0f - zg) * ng + zg * h;
                    if (SAVE) {
                        float *g = (is_t ? sv.gates_t : sv.gates_s) + (size_t)r * (4 * SR_HID) + col;
                        g[0] = rg; g[SR_HID] = zg; g[2 * SR_HID] = ng; g[3 * SR_HID] = ah[rb][i] + bhn;
                    }
                }
            }
    }
}

#ifndef SRNN_EDGE_KERNEL_ONLY   // srnn_train.hip launches the edge kernel only
// split a fp32 matrix into bf16 hi / lo planes (split_bf16.h)
__global__ void srnn_split_kernel(int n, const float *__restrict__ w, __bf16 *__restrict__ hi, __bf16 *__restrict__ lo)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const __bf16 h = (__bf16)w[i];
        hi[i] = h;
        lo[i] = (__bf16)(w[i] - (float)h);
    }
}

// W_hh [768,256] transposed and split: planes [256,768] whose rows are the 768 k of one hidden unit (the B fragments of the backward's
// carry product d_gh . W_hh, srnn_train_kernels.h)
__global__ void srnn_split_t_kernel(const float *__restrict__ w, __bf16 *__restrict__ hi, __bf16 *__restrict__ lo)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;       // index into the [256,768] planes
    if (i < 768 * SR_HID) {
        const float v = w[(size_t)(i % 768) * SR_HID + i / 768];
        const __bf16 h = (__bf16)v;
        hi[i] = h;
        lo[i] = (__bf16)(v - (float)h);
    }
}

// ---- everything behind the edge state ----
constexpr int SR_G = 8;                 // envs per workgroup: every weight row is read once per 8 envs
constexpr int SR_NODE_THREADS = 256;

struct SrnnNodeW {
    const float *at_w, *at_b, *as_w, *as_b;                 // attn.{temporal,spatial}_edge_layer.0 [64,256]
    const float *rl_w, *rl_b;                               // robot_linear [3,7]
    const float *enc_w, *enc_b;                             // humanNodeRNN.encoder_linear [64,3]
    const float *eae_w, *eae_b;                             // humanNodeRNN.edge_attention_embed [64,512]
    const float *w_ih, *w_hh, *b_ih, *b_hh;                 // humanNodeRNN.gru [384,128] x 2, [384] x 2
    const float *out_w, *out_b;                             // humanNodeRNN.output_linear [256,128]
    const float *a0_w, *a0_b, *a2_w, *a2_b, *c0_w, *c0_b, *c2_w, *c2_b;   // actor / critic trunks [256,256]
    const float *cl_w, *cl_b, *fm_w, *fm_b, *logstd;        // critic_linear [1,256], dist.fc_mean [2,256], dist.logstd._bias [2]
};

struct SrnnNodeIO {
    const float *robot_node, *edge, *node_in, *masks, *eps;                 // [E,7], [E,H+1,256] (the NEW edge state), [E,128], [E], [E,2] or null
    float *value, *action, *logp, *node_out;                                // [E], [E,2] or null, [E] or null, [E,128] or null
    float *tap_attn, *tap_weighted, *tap_node, *tap_feat;                   // [E,H], [E,256], [E,256], [E,256]
};

enum { SR_ACT_NONE = 0, SR_ACT_RELU = 1, SR_ACT_TANH = 2 };

// y[g][n] = act(b[n] + sum_k W[n][k] x[g][k]) for the workgroup's 8 envs: one thread per output unit, the weight row read once as float4,
// the activations broadcast from LDS.  K % 4 == 0, rows of W 16-byte aligned.  (Reading W transposed, 256 consecutive bytes per wavefront and
// k, was measured and is no faster: the layer is bound by the eight 16-byte LDS reads per 32 FMAs, not by the weight loads.)
template <int ACT>
__device__ __forceinline__ void sr_dense(const float *__restrict__ W, const float *__restrict__ b, int N, int K, const float *x, int ldx, float *y, int ldy)
{
    for (int n = threadIdx.x; n < N; n += SR_NODE_THREADS) {
        float acc[SR_G];
        const float bn = b[n];
#pragma unroll
        for (int g = 0; g < SR_G; ++g) acc[g] = bn;
        const sr_f4 *wr = reinterpret_cast<const sr_f4 *>(W + (size_t)n * K);
#pragma unroll 2
        for (int k4 = 0; k4 < K / 4; ++k4) {
            const sr_f4 w4 = wr[k4];
#pragma unroll
            for (int g = 0; g < SR_G; ++g) {
                const sr_f4 x4 = *reinterpret_cast<const sr_f4 *>(x + g * ldx + 4 * k4);
                acc[g] = fmaf(w4[0], x4[0], acc[g]);
                acc[g] = fmaf(w4[1], x4[1], acc[g]);
                acc[g] = fmaf(w4[2], x4[2], acc[g]);
                acc[g] = fmaf(w4[3], x4[3], acc[g]);
            }
        }
#pragma unroll
        for (int g = 0; g < SR_G; ++g) {
            float v = acc[g];
            if (ACT == SR_ACT_RELU) v = fmaxf(v, 0.0f);
            if (ACT == SR_ACT_TANH) v = tanhf(v);
            y[g * ldy + n] = v;
        }
    }
}

// One workgroup per 8 envs, activations in LDS, all arithmetic fp32.  An env's result does not depend on which envs share its workgroup.
// The spatial projection moves to the temporal side: <W_t h_t + b_t, W_s h_j + b_s> = <W_s^T t, h_j> + <t, b_s> with t = W_t h_t + b_t, so the
// H rows of h_s' are read as they left the edge kernel (once for the scores, once for the weighted sum) and never projected.
__global__ __launch_bounds__(SR_NODE_THREADS, 2) void srnn_node_kernel(int E, int H, SrnnNodeW w, SrnnNodeIO io)
{
    __shared__ __attribute__((aligned(16))) float hw[SR_G][512];     // [h_t' | weighted]; later [actor.0 out | critic.0 out]
    __shared__ __attribute__((aligned(16))) float ua[SR_G][256];     // u = W_s^T t; later the node output
    __shared__ __attribute__((aligned(16))) float gi[SR_G][384];     // GRU input side; later the actor features
    __shared__ __attribute__((aligned(16))) float gh[SR_G][384];     // GRU hidden side; later the critic features
    __shared__ __attribute__((aligned(16))) float xn[SR_G][128];     // [ReLU(enc) | ReLU(edge_attention_embed)]
    __shared__ __attribute__((aligned(16))) float hm[SR_G][128];     // mask * h_node, then h_node'
    __shared__ __attribute__((aligned(16))) float te[SR_G][64];      // t
    __shared__ float sc[SR_G][64];                                   // scores, then attention weights
    __shared__ float rn[SR_G][8], r3[SR_G][4], tb[SR_G], res[SR_G][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e0 = blockIdx.x * SR_G;
    const int ng = E - e0 < SR_G ? E - e0 : SR_G;                    // envs of this workgroup (>= 1 by the grid size)
    const size_t HP = (size_t)H + 1;

    for (int g = 0; g < SR_G; ++g) {
        const bool live = g < ng;
        const size_t e = (size_t)(e0 + g);
        hw[g][tid] = live ? io.edge[e * HP * SR_HID + tid] : 0.0f;
        if (tid < 128) hm[g][tid] = live ? io.node_in[e * 128 + tid] * io.masks[e] : 0.0f;
        if (tid < 8) rn[g][tid] = (live && tid < 7) ? io.robot_node[e * 7 + tid] : 0.0f;
    }
    __syncthreads();
    if (tid < SR_G * 3) {                                            // robot_linear [3,7]
        const int g = tid / 3, i = tid % 3;
        float v = w.rl_b[i];
        for (int k = 0; k < 7; ++k) v = fmaf(w.rl_w[i * 7 + k], rn[g][k], v);
        r3[g][i] = v;
    }
    sr_dense<SR_ACT_NONE>(w.at_w, w.at_b, 64, 256, &hw[0][0], 512, &te[0][0], 64);
    __syncthreads();
    {
        float acc[SR_G];
#pragma unroll
        for (int g = 0; g < SR_G; ++g) acc[g] = 0.0f;
#pragma unroll 4
        for (int j = 0; j < 64; ++j) {
            const float wv = w.as_w[j * 256 + tid];
#pragma unroll
            for (int g = 0; g < SR_G; ++g) acc[g] = fmaf(wv, te[g][j], acc[g]);
        }
#pragma unroll
        for (int g = 0; g < SR_G; ++g) ua[g][tid] = acc[g];
        if (tid < SR_G) {
            float v = 0.0f;
            for (int j = 0; j < 64; ++j) v = fmaf(te[tid][j], w.as_b[j], v);
            tb[tid] = v;
        }
        for (int idx = tid; idx < SR_G * 64; idx += SR_NODE_THREADS) {   // encoder_linear [64,3] on robot_linear's output
            const int g = idx >> 6, c = idx & 63;
            float v = w.enc_b[c];
            for (int k = 0; k < 3; ++k) v = fmaf(w.enc_w[c * 3 + k], r3[g][k], v);
            xn[g][c] = fmaxf(v, 0.0f);
        }
    }
    __syncthreads();
    // scores over ALL H slots (no mask), temperature H / sqrt(64) multiplies: one wavefront per (env, slot) pair, 4 columns per lane
    const float temp = (float)H * 0.125f;
    for (int p = wave; p < ng * H; p += SR_NODE_THREADS / 64) {
        const int g = p / H, j = p % H;
        const sr_f4 hv = *reinterpret_cast<const sr_f4 *>(io.edge + ((size_t)(e0 + g) * HP + 1 + j) * SR_HID + lane * 4);
        const sr_f4 uv = *reinterpret_cast<const sr_f4 *>(&ua[g][lane * 4]);
        const float d = wv_sum(hv[0] * uv[0] + hv[1] * uv[1] + hv[2] * uv[2] + hv[3] * uv[3]);
        if (lane == 0) sc[g][j] = (d + tb[g]) * temp;
    }
    __syncthreads();
    for (int g = wave; g < ng; g += SR_NODE_THREADS / 64) {
        const float v = lane < H ? sc[g][lane] : -__builtin_inff();
        const float m = wv_max(v);
        const float ex = lane < H ? expf(v - m) : 0.0f;
        const float s = wv_sum(ex);
        if (lane < H) {
            const float a = ex / s;
            sc[g][lane] = a;
            io.tap_attn[(size_t)(e0 + g) * H + lane] = a;
        }
    }
    __syncthreads();
    for (int g = 0; g < ng; ++g) {
        const float *hs = io.edge + ((size_t)(e0 + g) * HP + 1) * SR_HID + tid;
        float v = 0.0f;
#pragma unroll 4
        for (int j = 0; j < H; ++j) v = fmaf(sc[g][j], hs[(size_t)j * SR_HID], v);
        hw[g][256 + tid] = v;
        io.tap_weighted[(size_t)(e0 + g) * 256 + tid] = v;
    }
    for (int g = ng; g < SR_G; ++g) hw[g][256 + tid] = 0.0f;
    __syncthreads();
    sr_dense<SR_ACT_RELU>(w.eae_w, w.eae_b, 64, 512, &hw[0][0], 512, &xn[0][64], 128);
    __syncthreads();
    sr_dense<SR_ACT_NONE>(w.w_ih, w.b_ih, 384, 128, &xn[0][0], 128, &gi[0][0], 384);
    sr_dense<SR_ACT_NONE>(w.w_hh, w.b_hh, 384, 128, &hm[0][0], 128, &gh[0][0], 384);
    __syncthreads();
    if (tid < 128) {
        for (int g = 0; g < SR_G; ++g) {
            const float rg = sr_sigmoid(gi[g][tid] + gh[g][tid]), zg = sr_sigmoid(gi[g][128 + tid] + gh[g][128 + tid]);
            const float nn = tanhf(gi[g][256 + tid] + rg * gh[g][256 + tid]);
            const float hn = (1.0f - zg) * nn + zg * hm[g][tid];
            hm[g][tid] = hn;
            if (g < ng && io.node_out) io.node_out[(size_t)(e0 + g) * 128 + tid] = hn;
        }
    }
    __syncthreads();
    sr_dense<SR_ACT_NONE>(w.out_w, w.out_b, 256, 128, &hm[0][0], 128, &ua[0][0], 256);
    __syncthreads();
    for (int g = 0; g < ng; ++g) io.tap_node[(size_t)(e0 + g) * 256 + tid] = ua[g][tid];
    sr_dense<SR_ACT_TANH>(w.a0_w, w.a0_b, 256, 256, &ua[0][0], 256, &hw[0][0], 512);
    sr_dense<SR_ACT_TANH>(w.c0_w, w.c0_b, 256, 256, &ua[0][0], 256, &hw[0][256], 512);
    __syncthreads();
    sr_dense<SR_ACT_TANH>(w.a2_w, w.a2_b, 256, 256, &hw[0][0], 512, &gi[0][0], 384);
    sr_dense<SR_ACT_TANH>(w.c2_w, w.c2_b, 256, 256, &hw[0][256], 512, &gh[0][0], 384);
    __syncthreads();
    for (int g = 0; g < ng; ++g) io.tap_feat[(size_t)(e0 + g) * 256 + tid] = gi[g][tid];
    // heads: value = critic_linear . critic features, mean = fc_mean . actor features -- 3 dot products of 256 per env, one wavefront each
    for (int p = wave; p < ng * 3; p += SR_NODE_THREADS / 64) {
        const int g = p / 3, k = p % 3;
        const float *wr = k == 0 ? w.cl_w : w.fm_w + (k - 1) * 256;
        const float *xr = k == 0 ? &gh[g][0] : &gi[g][0];
        const sr_f4 wv4 = *reinterpret_cast<const sr_f4 *>(wr + lane * 4);
        const sr_f4 xv = *reinterpret_cast<const sr_f4 *>(xr + lane * 4);
        const float d = wv_sum(wv4[0] * xv[0] + wv4[1] * xv[1] + wv4[2] * xv[2] + wv4[3] * xv[3]);
        if (lane == 0) res[g][k] = d + (k == 0 ? w.cl_b[0] : w.fm_b[k - 1]);
    }
    __syncthreads();
    if (tid < ng) {
        const size_t e = (size_t)(e0 + tid);
        io.value[e] = res[tid][0];
        if (io.action && io.logp) {
            float lp = 0.0f;
            for (int d = 0; d < 2; ++d) {
                const float mean = res[tid][1 + d], ls = w.logstd[d], sd = expf(ls);
                const float a = io.eps ? mean + sd * io.eps[e * 2 + d] : mean;
                io.action[e * 2 + d] = a;
                lp += -((a - mean) * (a - mean)) / (2.0f * sd * sd) - ls - 0.918938533204672742f;   // log(sqrt(2 pi))
            }
            io.logp[e] = lp;
        }
    }
}

#endif // SRNN_EDGE_KERNEL_ONLY

} // namespace

// The handle (srnn.hip creates it; srnn_train.hip reads its snapshot, planes and mode)
constexpr int SR_NW = sizeof(cn_srnn_weights) / sizeof(const float *);
enum { W_ENC_S = 0, W_GRU_S = 2, W_ENC_T = 6, W_GRU_T = 8, W_ATTN = 12, W_NODE = 16, W_TRUNK = 26, W_HEADS = 34 };   // first field of each group

struct cn_srnn {
    int H, D, maxE, mode, have_weights;
    char *pool;                 // weight snapshot (fp32), split planes of the two W_hh, taps
    const float *w[SR_NW];      // snapshot pointers, in cn_srnn_weights field order
    __bf16 *planes[4];          // split planes of W_hh: spatial hi / lo, temporal hi / lo
    __bf16 *planes_t[4];        // the same of W_hh^T ([256,768]), for the training backward
    float *tap_attn, *tap_weighted, *tap_node, *tap_feat;
    float *edge_ws;             // [maxE,H+1,256], allocated by the first cn_srnn_get_value (which has no edge output of the caller's)
    const float *last_edge;     // the edge state the last forward wrote (the caller's edge_hxs_out, or edge_ws)
    int lastE;
};

static inline SrnnEdgeW srnn_edge_weights(const cn_srnn *p, int spatial)
{
    const int enc = spatial ? W_ENC_S : W_ENC_T, gru = spatial ? W_GRU_S : W_GRU_T, plane = spatial ? 0 : 2;
    SrnnEdgeW w;
    w.enc_w = p->w[enc]; w.enc_b = p->w[enc + 1];
    w.w_ih = p->w[gru]; w.w_hh = p->w[gru + 1]; w.b_ih = p->w[gru + 2]; w.b_hh = p->w[gru + 3];
    w.hh_hi = p->planes[plane]; w.hh_lo = p->planes[plane + 1];
    w.din = spatial ? p->D : 2;
    return w;
}
