// rn_chain.h -- the arithmetic of the robot-node chain, once: what rn_fused_kernel (rn_fused.hip, the default sizes) and rn_sized_kernel
// (rn_sized.hip, run-time sizes) both compute, as loop BODIES and scalar formulas, plus the host check of their common argument block.  Each kernel
// keeps its own loops, its dealing of feature blocks to wavefronts, its operand fetch and its scheduling (DESIGN.md section 4 says why: the same
// statements in rn_sized's run-time loop form cost rn_fused_kernel its 128-register budget and change its FMA contraction).  The Gaussian head's
// formulas also serve gauss_head_kernel (policy_kernels.h) and rn_head_fwd_kernel (rn_train.h).
#pragma once
#include "rn_fused.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x4 mfma32(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

enum { A_NONE = 0, A_RELU = 1, A_TANH = 2 };

// The small words: the 64-word tail of a workgroup's LDS table.  Word SM_MASK + i is the done mask of the workgroup's env i (up to 16), words
// SM_EPS + 2 i, + 1 its two noise values, then critic_linear's bias, fc_mean's two and the two logstd; SM_USED .. 63 are padding.
constexpr int SM_MASK = 0, SM_EPS = 16, SM_CLB = 48, SM_FMB = 49, SM_LS = 51, SM_USED = 53, SM_WORDS = 64;

// One k-step of a product's B operand: the activations k = 32 ks + 8 (lane >> 4) .. + 7 of this lane's env as bf16 hi / lo.
// xrow: the env's LDS row + 8 * (lane >> 4)
__device__ __forceinline__ void rn_split(const float *xrow, int ks, bf16x8 &h, bf16x8 &l)
{
    const f32x4 x0 = *reinterpret_cast<const f32x4 *>(xrow + 32 * ks);
    const f32x4 x1 = *reinterpret_cast<const f32x4 *>(xrow + 32 * ks + 4);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const __bf16 h0 = (__bf16)x0[u], h1 = (__bf16)x1[u];
        h[u] = h0; h[4 + u] = h1;
        l[u] = (__bf16)(x0[u] - (float)h0); l[4 + u] = (__bf16)(x1[u] - (float)h1);
    }
}

// A stage's epilogue for one accumulator = the features f0 .. f0 + 3 of this lane's env: bias (the LDS copy; only looked at with BIAS: a run-time
// test of the pointer put every block's bias load into a basic block of its own), relu from feature relu_from on or tanh, float4 store.
// orow: the env's output row + the stage's offset, or nullptr = no store (rn_sized's repeated env columns)
template <int ACT, bool BIAS>
__device__ __forceinline__ void rn_epilogue(f32x4 v, int f0, const float *bias, int relu_from, float *orow)
{
    if (BIAS) v += *reinterpret_cast<const f32x4 *>(bias + f0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (ACT == A_RELU) { if (f0 + q >= relu_from) v[q] = fmaxf(v[q], 0.0f); }
        if (ACT == A_TANH) v[q] = fast_tanh(v[q]);
    }
    if (orow) *reinterpret_cast<f32x4 *>(orow + f0) = v;
}

// A score's dot product over this lane's four columns of u and of one out_sp row.  The two kernels round it differently and each keeps its bits
// (DESIGN.md section 4).  SEPARATE (rn_sized_kernel): the four products rounded on their own, then added.  Otherwise (rn_fused_kernel) the
// contraction into multiply-adds is the compiler's, as it always was there: it fuses rows 0 .. 4 of a chunk and vectorises rows 5 .. 7 unfused.
template <bool SEPARATE>
__device__ __forceinline__ float rn_dot4(float u0, float u1, float u2, float u3, const float (&x)[4])
{
    if (!SEPARATE) return u0 * x[0] + u1 * x[1] + u2 * x[2] + u3 * x[3];
    {
#pragma clang fp contract(off)
        return u0 * x[0] + u1 * x[1] + u2 * x[2] + u3 * x[3];
    }
}

// Robot-human attention (u-form, see hr_attention_kernel in attention.h) of one wavefront's PER envs i0 .. i0 + PER - 1 of the workgroup:
// u = row i of R1 (stride S1), hr -> row i of R0 (stride S0; robot_states are dead: hr takes their place).  r0q / r1q: the envs' first and
// past-the-last out_sp row, wave-uniform.
// out_sp was written a moment ago by the human-human kernel on (mostly) other XCDs: every row read is a trip to the fabric.  A row-by-row loop
// is a chain of such trips (two passes x nd rows x PER envs), so the first 8 rows of ALL the wavefront's envs are fetched up front into
// registers; envs with more rows walk the rest in chunks of 8.  Row indices are clamped and results selected, never guarded: a branch among
// the loads costs a wait at its join.
template <int PER, bool TAPS, bool SEPARATE>
__device__ __forceinline__ void rn_hr_attention(const RnFusedArgs &a, const int (&r0q)[PER], const int (&r1q)[PER], const float *R1, int S1, float *R0,
                                                int S0, int i0, int e0, int E, int H, float scale, int lane)
{
    constexpr int CH = 8;
    int ndq[PER];
    float x[PER][CH][4];
#pragma unroll
    for (int q = 0; q < PER; ++q) ndq[q] = r1q[q] - r0q[q];
#pragma unroll
    for (int q = 0; q < PER; ++q)
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const float *row = a.out_sp + (size_t)(r0q[q] + (u < ndq[q] ? u : ndq[q] - 1)) * 256;
            x[q][u][0] = row[lane]; x[q][u][1] = row[64 + lane]; x[q][u][2] = row[128 + lane]; x[q][u][3] = row[192 + lane];
        }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int i = i0 + q;
        const int r0 = r0q[q], nd = ndq[q];
        const float *ue = R1 + i * S1;
        const float u0 = ue[lane], u1 = ue[64 + lane], u2 = ue[128 + lane], u3 = ue[192 + lane];
        float s = -INFINITY; // lane j holds the score of human j
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const float tot = wv_sum(rn_dot4<SEPARATE>(u0, u1, u2, u3, x[q][u]));
            if (lane == u && u < nd) s = tot * scale;
        }
        for (int j0 = CH; j0 < nd; j0 += CH) {
            float y[CH][4];
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const float *row = a.out_sp + (size_t)(r0 + (j0 + u < nd ? j0 + u : nd - 1)) * 256;
                y[u][0] = row[lane]; y[u][1] = row[64 + lane]; y[u][2] = row[128 + lane]; y[u][3] = row[192 + lane];
            }
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const float tot = wv_sum(rn_dot4<SEPARATE>(u0, u1, u2, u3, y[u]));
                if (lane == j0 + u && j0 + u < nd) s = tot * scale;
            }
        }
        const float mx = wv_max(s);
        const float p = lane < nd ? expf(s - mx) : 0.0f;
        const float denom = wv_sum(p);
        const float at = p / denom;
        float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f;
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const float aj = u < nd ? wv_readlane(at, u) : 0.0f;
            if (u < nd) { o0 += aj * x[q][u][0]; o1 += aj * x[q][u][1]; o2 += aj * x[q][u][2]; o3 += aj * x[q][u][3]; }
        }
        for (int j0 = CH; j0 < nd; j0 += CH) {
            float y[CH][4];
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const float *row = a.out_sp + (size_t)(r0 + (j0 + u < nd ? j0 + u : nd - 1)) * 256;
                y[u][0] = row[lane]; y[u][1] = row[64 + lane]; y[u][2] = row[128 + lane]; y[u][3] = row[192 + lane];
            }
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const float aj = wv_readlane(at, j0 + u < nd ? j0 + u : 0);
                if (j0 + u < nd) { o0 += aj * y[u][0]; o1 += aj * y[u][1]; o2 += aj * y[u][2]; o3 += aj * y[u][3]; }
            }
        }
        float *o = R0 + i * S0;
        o[lane] = o0; o[64 + lane] = o1; o[128 + lane] = o2; o[192 + lane] = o3;
        if (TAPS && e0 + i < E) { // (behind the env's last out_sp row, not between the two passes)
            if (lane < H) a.tap_attn[(size_t)(e0 + i) * H + lane] = at;
            float *t = a.tap_hr + (size_t)(e0 + i) * 256;
            t[lane] = o0; t[64 + lane] = o1; t[128 + lane] = o2; t[192 + lane] = o3;
        }
    }
}

// GRU cell, pointwise part, of one hidden unit (gate order r,z,n; h and gh masked by the done mask m: srnn_model.py:43-46)
__device__ __forceinline__ float rn_gru_cell(float gi_r, float gi_z, float gi_n, float gh_r, float gh_z, float gh_n, float b_r, float b_z, float b_n,
                                             float m, float h_in)
{
    const float hr = m * gh_r + b_r, hz = m * gh_z + b_z, hn = m * gh_n + b_n;
    const float r = fast_sigmoid(gi_r + hr);
    const float z = fast_sigmoid(gi_z + hz);
    const float nn = fast_tanh(gi_n + r * hn);
    const float h = m * h_in;
    return (1.0f - z) * nn + z * h;
}

// DiagGaussian over the two action components (distributions.py:36-44,76-95): log-probability of (a0, a1), sd = exp(ls) ...
constexpr float HALF_LOG_2PI = 0.91893853320467274178f;
__device__ __forceinline__ float rn_gauss_logp(float a0, float a1, float mean0, float mean1, float ls0, float ls1, float sd0, float sd1)
{
    const float d0 = a0 - mean0, d1 = a1 - mean1;
    return (-(d0 * d0) / (2.0f * sd0 * sd0) - ls0 - HALF_LOG_2PI) + (-(d1 * d1) / (2.0f * sd1 * sd1) - ls1 - HALF_LOG_2PI);
}
// ... and the sample mean + sd * eps (noise off: the mode) with its log-probability
__device__ __forceinline__ float rn_gauss_sample(float mean0, float mean1, float ls0, float ls1, bool noise, float eps0, float eps1, float &a0, float &a1)
{
    const float sd0 = expf(ls0), sd1 = expf(ls1);
    a0 = noise ? mean0 + sd0 * eps0 : mean0;
    a1 = noise ? mean1 + sd1 * eps1 : mean1;
    return rn_gauss_logp(a0, a1, mean0, mean1, ls0, ls1, sd0, sd1);
}

// Host: what both kernels take for granted of their argument block
inline int rn_check_args(const RnFusedArgs &a, const char *who)
{
    const bool taps = a.tap_robot || a.tap_attn || a.tap_hr || a.tap_actor;
    CN_REQUIRE(!taps || (a.tap_robot && a.tap_attn && a.tap_hr && a.tap_actor), "%s: the four taps come together", who);
    for (const float *p : {a.te_b, a.edge_b, a.bih, a.bhh, a.ac0_b, a.a2_b, a.c2_b, a.cl_w, a.fm_w}) // the table's vectors are fetched as float4
        CN_REQUIRE(p && ((uintptr_t)p & 15) == 0, "%s: biases and head weights must be 16-byte aligned", who);
    for (const float *p : {a.f_te, a.f_whh, a.f_edge, a.f_wih, a.f_ac0, a.f_a2, a.f_c2})
        CN_REQUIRE(p && ((uintptr_t)p & 15) == 0, "%s: fragment images must be 16-byte aligned", who);
    CN_REQUIRE(a.temporal && a.robot_node && a.hxs_in && a.masks && a.out_sp && a.row_off && a.rl_w && a.rl_b && a.cl_b && a.fm_b && a.logstd && a.value &&
               a.hxs_out, "%s: null pointer", who);
    CN_REQUIRE(!a.action || a.logp, "%s: action and logp go together", who);
    return CN_OK;
}

} // namespace
