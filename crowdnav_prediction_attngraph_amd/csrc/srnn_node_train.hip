// The DS-RNN baseline's edge attention in the PPO update (SRNNBase.attention: rl/networks/srnn_model.py:256-323 over the saved edge states):
// cn_srnn_attn_fwd / cn_srnn_attn_bwd.  A memory stream over h_all [B, H+1, 256] -- slot 0 the temporal edge t, slots 1 .. H the spatial edges s_j:
//
//   te = Wt t + bt (64);  u = Ws^T te (256);  score_j = (H / 8) u . s_j;  a = softmax_j(score);  weighted = sum_j a_j s_j
//
// (te . (Ws s_j + bs) = u . s_j + te . bs, and the second term is the same for every j: the softmax does not see it, bs gets an exactly-zero
// gradient and no [B,H,64] tensor exists).  One wavefront owns a sample: a 256-float row is one 16-byte load per lane, lane l holds elements
// 4 l .. 4 l + 3.  The forward reads h_all once (online softmax over chunks of SA_CHUNK rows, the next chunk in flight), the backward reads it
// once and writes d_h_all once, every element exactly once, no atomics.  Plain fp32, fixed summation orders, nothing of a sample's arithmetic
// depends on another sample: equal arguments give equal bits, and so does a sample alone or as any row of a batch.
//
// The two small products per sample and direction share one arrangement.  A workgroup (16 wavefronts, one per CU: 129 KB of LDS) stages both
// weight matrices once and its wavefronts then walk samples blockIdx * 16 + wave, + 16 * gridDim, ...:
//   proj   (256 -> 64): lane k sums W[k][c] x[c] over c; W sits transposed in LDS with a row stride of 65 floats (lanes = consecutive banks),
//          x[c] comes out of the owning lane's register by v_readlane; four partial sums (c mod 4), added as (0 + 1) + (2 + 3)
//   expand (64 -> 256): lane l sums W[k][4 l .. 4 l + 3] v[k] over k = 0 .. 63 in order; W row-major in LDS, one ds_read_b128 per k
// forward: proj = Wt (+ bt), expand = Ws;  backward: proj = Ws (d_te = Ws d_u), expand = Wt (d_t = Wt^T d_te).
#include "common.h"

namespace {

constexpr int SA_E = 256;                                   // edge state width
constexpr int SA_A = 64;                                    // attention size
constexpr int SA_WAVES = 16, SA_THREADS = SA_WAVES * CN_WAVE;   // four per SIMD: at most 128 VGPRs (116 / 126 used); 8 -> 16 took 5 % off the forward
constexpr int SA_PSTRIDE = SA_A + 1;                        // row stride of the transposed proj matrix in LDS
constexpr int SA_LDS_BYTES = (SA_E * SA_PSTRIDE + SA_A * SA_E) * (int)sizeof(float);
constexpr int SA_MAX_BLOCKS = 256;                          // one workgroup per CU; more samples: the wavefronts stride (tests/test_gpu_strided_grids.py)
constexpr int SA_CHUNK = 8;                                 // rows a wavefront holds in registers (and has in flight) at a time

// both [64][256] row-major in global memory.  Scalar loads: a parameter may be a slice of a flat bucket at any 4-byte offset.
__device__ __forceinline__ void sa_stage(float *lds, const float *__restrict__ proj, const float *__restrict__ expd)
{
    float *P = lds, *X = lds + SA_E * SA_PSTRIDE;
    for (int i = threadIdx.x; i < SA_A * SA_E; i += SA_THREADS) {
        P[(i & (SA_E - 1)) * SA_PSTRIDE + (i >> 8)] = proj[i];
        X[i] = expd[i];
    }
    __syncthreads();
}

__device__ __forceinline__ float sa_proj(const float *P, const float4 x, int lane)
{
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 4
    for (int q = 0; q < SA_E / 4; ++q) {
        const float *p = P + 4 * q * SA_PSTRIDE + lane;
        a0 = fmaf(p[0], wv_readlane(x.x, q), a0);
        a1 = fmaf(p[SA_PSTRIDE], wv_readlane(x.y, q), a1);
        a2 = fmaf(p[2 * SA_PSTRIDE], wv_readlane(x.z, q), a2);
        a3 = fmaf(p[3 * SA_PSTRIDE], wv_readlane(x.w, q), a3);
    }
    return (a0 + a1) + (a2 + a3);
}

__device__ __forceinline__ float4 sa_expand(const float4 *X, const float v, int lane)
{
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
    for (int k = 0; k < SA_A; ++k) {
        const float4 w = X[k * (SA_E / 4) + lane];
        const float s = wv_readlane(v, k);
        o.x = fmaf(s, w.x, o.x); o.y = fmaf(s, w.y, o.y); o.z = fmaf(s, w.z, o.z); o.w = fmaf(s, w.w, o.w);
    }
    return o;
}

struct SaRows { float4 v[SA_CHUNK]; };
// rows j0 .. j0 + 7 of the sample's H spatial slots (rows past H repeat the last one: loaded, never used)
__device__ __forceinline__ void sa_load(SaRows &r, const float *__restrict__ s_rows, int j0, int H, int lane)
{
#pragma unroll
    for (int q = 0; q < SA_CHUNK; ++q) r.v[q] = *reinterpret_cast<const float4 *>(s_rows + (size_t)min(j0 + q, H - 1) * SA_E + 4 * lane);
}
__device__ __forceinline__ float sa_dot(const float4 a, const float4 b) { return wv_sum(fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)))); }
__device__ __forceinline__ void sa_axpy(float4 &o, const float s, const float4 x)
{
    o.x = fmaf(s, x.x, o.x); o.y = fmaf(s, x.y, o.y); o.z = fmaf(s, x.z, o.z); o.w = fmaf(s, x.w, o.w);
}

__global__ __launch_bounds__(SA_THREADS) void srnn_attn_fwd_kernel(int B, int H, const float *__restrict__ h_all, const float *__restrict__ Wt,
                                                                   const float *__restrict__ bt, const float *__restrict__ Ws,
                                                                   float *__restrict__ weighted, float *__restrict__ attn, float *__restrict__ te_out,
                                                                   float *__restrict__ u_out)
{
    extern __shared__ float sa_lds[];
    sa_stage(sa_lds, Wt, Ws);
    const float *P = sa_lds;
    const float4 *X = reinterpret_cast<const float4 *>(sa_lds + SA_E * SA_PSTRIDE);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float bias = bt[lane];
    const float scale = (float)H * 0.125f;                  // H / sqrt(64): the temperature MULTIPLIES
    const size_t stride = (size_t)(H + 1) * SA_E;
    for (size_t b = (size_t)blockIdx.x * SA_WAVES + wave; b < (size_t)B; b += (size_t)gridDim.x * SA_WAVES) {
        const float *hb = h_all + b * stride;
        const float4 t = *reinterpret_cast<const float4 *>(hb + 4 * lane);
        SaRows cur;
        sa_load(cur, hb + SA_E, 0, H, lane);                // in flight under the two products
        const float te = sa_proj(P, t, lane) + bias;
        const float4 u = sa_expand(X, te, lane);
        te_out[b * SA_A + lane] = te;
        *reinterpret_cast<float4 *>(u_out + b * SA_E + 4 * lane) = u;
        // online softmax over chunks of rows: m the running maximum, l the running denominator, acc = sum_j exp(score_j - m) s_j
        float s = 0.f, m = -INFINITY, l = 0.f;              // lane j keeps score_j
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j0 = 0; j0 < H; j0 += SA_CHUNK) {
            SaRows nxt = cur;
            if (j0 + SA_CHUNK < H) sa_load(nxt, hb + SA_E, j0 + SA_CHUNK, H, lane);
            float sc[SA_CHUNK] = {}, cm = m;
#pragma unroll
            for (int q = 0; q < SA_CHUNK; ++q)
                if (j0 + q < H) {
                    sc[q] = sa_dot(u, cur.v[q]) * scale;
                    cm = fmaxf(cm, sc[q]);
                    if (lane == j0 + q) s = sc[q];
                }
            const float corr = expf(m - cm);                // first chunk: exp(-inf) = 0 on zeros
            acc.x *= corr; acc.y *= corr; acc.z *= corr; acc.w *= corr;
            l *= corr;
#pragma unroll
            for (int q = 0; q < SA_CHUNK; ++q)
                if (j0 + q < H) {
                    const float p = expf(sc[q] - cm);
                    l += p;
                    sa_axpy(acc, p, cur.v[q]);
                }
            m = cm;
            cur = nxt;
        }
        const float inv = 1.0f / l;
        if (lane < H) attn[b * H + lane] = expf(s - m) * inv;
        *reinterpret_cast<float4 *>(weighted + b * SA_E + 4 * lane) = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
    }
}

// Backward.  With g = d_weighted and dp_j = g . s_j, dot = sum_j a_j dp_j, d_score_j = a_j (dp_j - dot):
//   d_s_j = a_j g + scale d_score_j u
//   d_u   = scale sum_j d_score_j s_j = scale (sum_j a_j dp_j s_j - dot sum_j a_j s_j)      (both sums in the ONE pass over the rows)
//   d_te  = Ws d_u;  d_t = Wt^T d_te (+ d_t_direct)
// d_score needs dot, i.e. all rows; d_s_j needs no row, so the rows are read once and the H gradient rows are written afterwards.
__global__ __launch_bounds__(SA_THREADS) void srnn_attn_bwd_kernel(int B, int H, const float *__restrict__ h_all, const float *__restrict__ Wt,
                                                                   const float *__restrict__ Ws, const float *__restrict__ attn, const float *__restrict__ u_in,
                                                                   const float *__restrict__ d_weighted, const float *__restrict__ d_t_direct,
                                                                   float *__restrict__ d_h_all, float *__restrict__ d_u_out, float *__restrict__ d_te_out)
{
    extern __shared__ float sa_lds[];
    sa_stage(sa_lds, Ws, Wt);
    const float *P = sa_lds;
    const float4 *X = reinterpret_cast<const float4 *>(sa_lds + SA_E * SA_PSTRIDE);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float scale = (float)H * 0.125f;
    const size_t stride = (size_t)(H + 1) * SA_E;
    for (size_t b = (size_t)blockIdx.x * SA_WAVES + wave; b < (size_t)B; b += (size_t)gridDim.x * SA_WAVES) {
        const float *hb = h_all + b * stride;
        SaRows cur;
        sa_load(cur, hb + SA_E, 0, H, lane);
        const float a = lane < H ? attn[b * H + lane] : 0.0f;                      // lanes = slots
        const float4 g = *reinterpret_cast<const float4 *>(d_weighted + b * SA_E + 4 * lane);
        const float4 u = *reinterpret_cast<const float4 *>(u_in + b * SA_E + 4 * lane);
        float dp = 0.f;
        float4 sa = make_float4(0.f, 0.f, 0.f, 0.f), sw = make_float4(0.f, 0.f, 0.f, 0.f);   // sum_j a_j dp_j s_j and sum_j a_j s_j
        for (int j0 = 0; j0 < H; j0 += SA_CHUNK) {
            SaRows nxt = cur;
            if (j0 + SA_CHUNK < H) sa_load(nxt, hb + SA_E, j0 + SA_CHUNK, H, lane);
#pragma unroll
            for (int q = 0; q < SA_CHUNK; ++q)
                if (j0 + q < H) {
                    const float d = sa_dot(g, cur.v[q]);
                    const float aj = wv_readlane(a, j0 + q);
                    if (lane == j0 + q) dp = d;
                    sa_axpy(sw, aj, cur.v[q]);
                    sa_axpy(sa, aj * d, cur.v[q]);
                }
            cur = nxt;
        }
        const float dot = wv_sum(a * dp);
        const float gs = scale * (a * (dp - dot));                                  // lane j: scale d_score_j
        // (the products rounded before the subtraction, not contracted into it: with one slot sa = fl(dp s) and dot sw = dp s, and d_u -- with it d_te
        // and the three weight gradients -- is the exact zero of a softmax over one element; as fma(-dot, sw, sa) it was the rounding residual of
        // dp s, which summed over 8245 samples put 1.2e-6 into gradients that are zero)
        float4 du;
        {
#pragma clang fp contract(off)
            du = make_float4(scale * (sa.x - dot * sw.x), scale * (sa.y - dot * sw.y), scale * (sa.z - dot * sw.z), scale * (sa.w - dot * sw.w));
        }
        *reinterpret_cast<float4 *>(d_u_out + b * SA_E + 4 * lane) = du;
        float *db = d_h_all + b * stride;
        for (int j = 0; j < H; ++j) {
            const float aj = wv_readlane(a, j), gj = wv_readlane(gs, j);
            *reinterpret_cast<float4 *>(db + (size_t)(1 + j) * SA_E + 4 * lane) =
                make_float4(fmaf(gj, u.x, aj * g.x), fmaf(gj, u.y, aj * g.y), fmaf(gj, u.z, aj * g.z), fmaf(gj, u.w, aj * g.w));
        }
        const float dte = sa_proj(P, du, lane);
        d_te_out[b * SA_A + lane] = dte;
        float4 dt = sa_expand(X, dte, lane);
        if (d_t_direct) {
            const float4 e = *reinterpret_cast<const float4 *>(d_t_direct + b * SA_E + 4 * lane);
            dt.x += e.x; dt.y += e.y; dt.z += e.z; dt.w += e.w;
        }
        *reinterpret_cast<float4 *>(db + 4 * lane) = dt;
    }
}

bool sa_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

} // namespace

#define SA_BOX(who)                                                                                                                           \
    CN_REQUIRE(H >= 1 && H <= CN_MAX_HUMANS, who ": H = %d outside the box 1 <= H <= %d (edge width 256, attention size 64)", H, CN_MAX_HUMANS); \
    CN_REQUIRE(B >= 1, who ": B = %d samples (at least one)", B)

extern "C" int cn_srnn_attn_fwd(int B, int H, const float *h_all, const float *Wt, const float *bt, const float *Ws, float *weighted, float *attn, float *te,
                                float *u, void *stream)
{
    SA_BOX("cn_srnn_attn_fwd");
    CN_REQUIRE(h_all && Wt && bt && Ws && weighted && attn && te && u, "cn_srnn_attn_fwd: null operand");
    CN_REQUIRE(sa_aligned(h_all) && sa_aligned(weighted) && sa_aligned(u), "cn_srnn_attn_fwd: h_all, weighted and u must be 16-byte aligned");
    if (int rc = cn_require_device()) return rc;
    if (int rc = cn_lds_opt_in<&srnn_attn_fwd_kernel>(SA_LDS_BYTES)) return rc;
    const int blocks = (int)min((long long)SA_MAX_BLOCKS, ((long long)B + SA_WAVES - 1) / SA_WAVES);
    hipLaunchKernelGGL(srnn_attn_fwd_kernel, dim3(blocks), dim3(SA_THREADS), SA_LDS_BYTES, (hipStream_t)stream, B, H, h_all, Wt, bt, Ws, weighted, attn, te, u);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_srnn_attn_bwd(int B, int H, const float *h_all, const float *Wt, const float *Ws, const float *attn, const float *u, const float *d_weighted,
                                const float *d_t_direct, float *d_h_all, float *d_u, float *d_te, void *stream)
{
    SA_BOX("cn_srnn_attn_bwd");
    CN_REQUIRE(h_all && Wt && Ws && attn && u && d_weighted && d_h_all && d_u && d_te, "cn_srnn_attn_bwd: null operand (only d_t_direct may be NULL)");
    CN_REQUIRE(sa_aligned(h_all) && sa_aligned(u) && sa_aligned(d_weighted) && sa_aligned(d_t_direct) && sa_aligned(d_h_all) && sa_aligned(d_u),
               "cn_srnn_attn_bwd: h_all, u, d_weighted, d_t_direct, d_h_all and d_u must be 16-byte aligned");
    if (int rc = cn_require_device()) return rc;
    if (int rc = cn_lds_opt_in<&srnn_attn_bwd_kernel>(SA_LDS_BYTES)) return rc;
    const int blocks = (int)min((long long)SA_MAX_BLOCKS, ((long long)B + SA_WAVES - 1) / SA_WAVES);
    hipLaunchKernelGGL(srnn_attn_bwd_kernel, dim3(blocks), dim3(SA_THREADS), SA_LDS_BYTES, (hipStream_t)stream, B, H, h_all, Wt, Ws, attn, u, d_weighted,
                       d_t_direct, d_h_all, d_u, d_te);
    CN_CHECK_LAUNCH();
    return CN_OK;
}
