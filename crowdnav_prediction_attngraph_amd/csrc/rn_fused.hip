// rn_fused.hip -- the robot-node half of the policy forward as ONE kernel on gfx950 (everything after the human-human block):
//   robot_linear -> [u = Ws^T temporal_edge_layer(.) | encoder_linear] -> robot-human attention over out_sp ->
//   edge_attention_embed -> GRU cell (with the done mask) -> actor / critic trunks (output_linear folded in) -> critic_linear +
//   DiagGaussian head.               rl/networks/selfAttn_srnn_temp_node.py:395-449, srnn_model.py:35-105, model.py:56-80
// As separate launches this is ~12 small kernels whose M = E products fill a fraction of the chip each and whose LDS-using
// blocks cannot even co-reside with the 160 KB workgroups of the fused human-human kernel; here one workgroup (8 wavefronts)
// owns 16 envs, keeps every per-env activation in LDS and walks the ~1.3 MB of weights once, straight from L2 into MFMA operand
// registers.  The products run in the same bf16x3 split precision as the human-human kernel (fp32 operand = hi + lo bf16, products
// hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16, fp32 accumulation): with exact fp32 MFMA (v_mfma_f32_16x16x4_f32, 1/16 of the
// bf16 rate) the seven stages were bound by the fp32 matrix pipe -- in-kernel timers: 83 k of the kernel's 118 k cycles, at ~60 % pipe
// utilisation -- now they are bound by streaming the 1.3 MB weight image.
//
// Products run "transposed" (A operand = weight fragment, B operand = activations): the C layout then holds 4 consecutive output
// features of one env per lane, which is a float4 store into the next layer's [env][feature] LDS image; the B operand of the
// next product is two float4 reads of that image (k = 32 ks + 8*(lane>>4) + 0..7), split to bf16 hi / lo once per stage.
//
// The kernel is a latency chain, so what it waits for is counted (profiles/HISTORY.md section 14): one batch of loads at kernel entry brings
// every small operand (observation, hidden state, masks, noise, biases, head weights) into registers and a 12 KB LDS table; behind it a
// wavefront waits for weight fragments and out_sp rows only, and no stage call is longer than 8 k-steps (32 in sequence on the longest path:
// te 8, edge 8, W_ih 4, ac0 4, a2 / c2 8).  Two instantiations: with the four test taps and without.
#include "rn_chain.h"
#include "row_plan.h"

namespace {

constexpr int TE = 16;     // envs per workgroup
// LDS activation images [16 envs][stride] floats; strides are K + 4 so that the 16 lanes of a float4 read hit distinct banks
constexpr int S512 = 516, S384 = 388, S128 = 132;
constexpr int O_R0 = 0;                     // 512: robot_states (256) -> hr (256) -> ac1 (512)
constexpr int O_R1 = O_R0 + TE * S512;      // 512: z = [u 256 | enc 64 | edge 64] -> ac2 (512)
constexpr int O_R2 = O_R1 + TE * S512;      // 384: gh
constexpr int O_R3 = O_R2 + TE * S384;      // 384: gi
constexpr int O_R4 = O_R3 + TE * S384;      // 128: h_in
constexpr int O_R5 = O_R4 + TE * S128;      // 128: h_new
// the table: every small operand of the chain (biases, head weights, the 16 envs' masks and noise), fetched in the ONE batch at kernel entry
constexpr int O_T = O_R5 + TE * S128;
constexpr int T_TEB = 0, T_EDGEB = T_TEB + 320, T_BIH = T_EDGEB + 64, T_BHH = T_BIH + 384, T_AC0B = T_BHH + 384, T_A2B = T_AC0B + 512;
constexpr int T_C2B = T_A2B + 256, T_CLW = T_C2B + 256, T_FMW = T_CLW + 256;
constexpr int T_VEC4 = (T_FMW + 512) / 4;   // 736 float4
constexpr int T_SM = T_FMW + 512;           // the small words (rn_chain.h)
constexpr int T_FLOATS = T_SM + SM_WORDS;   // 3008 floats, 12 032 B
constexpr int LDS_FLOATS = O_T + T_FLOATS;  // 144 640 B of the 160 KB: one workgroup per CU, as before
static_assert(LDS_FLOATS * sizeof(float) <= 160 * 1024, "rn_fused: LDS");

// out[env][out_off + 16*fb + ..] = act(W[fb] . in[env][in_off ..] + bias) for the feature blocks fb = fb_first, fb_first + fb_step, ...
// Wfrag: baked fragments [fb][K/32][plane hi,lo][64 lanes][8 bf16]; NFB = feature blocks of this wavefront; bias: the LDS copy (table, below),
// only looked at with BIAS: a run-time test of the pointer put every block's bias load into a basic block of its own
template <int K, int NFB, int ACT, bool BIAS>
__device__ __forceinline__ void stage(const float *__restrict__ Wfrag_, int fb_first, int fb_step, const float *bias, const float *in, int in_stride,
                                      float *out, int out_stride, int out_off, int relu_from, int lane)
{
    const bf16x8 *__restrict__ Wfrag = reinterpret_cast<const bf16x8 *>(Wfrag_);
    const int i = lane & 15, g = lane >> 4;
    constexpr int KS = K / 32;
    // activations of env i, k = 32 ks + 8 g .. + 7, as bf16 hi / lo (the B operand of every feature block of this stage), split per k-step
    // inside the loop rather than up front (64 registers less at K = 256)
    bf16x8 bh, bl;
    const float *xrow = in + i * in_stride + 8 * g;
    f32x4 acc[NFB];
#pragma unroll
    for (int j = 0; j < NFB; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // weight fragments: PF k-steps in flight (the scheduling barriers pin the issue points, see hh_fused.hip)
    constexpr int PF = KS < 2 ? KS : 2;
    bf16x8 ah[PF][NFB], al[PF][NFB];
#pragma unroll
    for (int p = 0; p < PF - 1; ++p)
#pragma unroll
        for (int j = 0; j < NFB; ++j) {
            const size_t base = ((size_t)(fb_first + j * fb_step) * KS + (p < KS ? p : KS - 1)) * 128 + lane;
            ah[p][j] = Wfrag[base]; al[p][j] = Wfrag[base + 64];
        }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) { // fully unrolled: ah / al must be statically indexed (a runtime index sends the arrays to scratch)
        const int kp = ks + PF - 1 < KS ? ks + PF - 1 : KS - 1;
#pragma unroll
        for (int j = 0; j < NFB; ++j) {
            const size_t base = ((size_t)(fb_first + j * fb_step) * KS + kp) * 128 + lane;
            ah[(ks + PF - 1) % PF][j] = Wfrag[base]; al[(ks + PF - 1) % PF][j] = Wfrag[base + 64];
        }
        rn_split(xrow, ks, bh, bl);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < NFB; ++j) {
            acc[j] = mfma32(al[ks % PF][j], bh, acc[j]);
            acc[j] = mfma32(ah[ks % PF][j], bl, acc[j]);
            acc[j] = mfma32(ah[ks % PF][j], bh, acc[j]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < NFB; ++j)
        rn_epilogue<ACT, BIAS>(acc[j], (fb_first + j * fb_step) * 16 + 4 * g, bias, relu_from, out + i * out_stride + out_off);
}

// The chain runs in 128 registers per lane (activations split per k-step, two k-steps of weight fragments in flight, at most four feature blocks
// per call, nothing held across the barriers).  On its own that is a few us slower than the 255-register form it replaced in
// round 6 (see git history); but a workgroup then takes HALF of its CU's registers, and the ORCA tail's wavefronts (orca_lp3_kernel on the
// simulator's side stream: 32 registers, no LDS, 37 us of VALU work for the whole chip) run on the same CUs beside this latency chain instead
// of making it wait for CUs of its own: hh_fused -> rn_fused gap 17.7 -> 9.9 us, step 0.2806 -> 0.2705 ms at 4096 envs x 20 humans (same box),
// configs[4] 2.07 -> 2.05 ms beside the cooperative ORCA kernel.
//
// Loads.  Apart from the weight fragments and the out_sp rows, everything the chain reads -- the 16 envs' observation, hidden state, masks and
// noise, robot_linear's weights, every bias, the head's weights, the row offsets -- has an address that follows from the arguments, blockIdx and
// the lane.  It all leaves in ONE batch in front of the first wait (indices clamped, never guarded: a branch among the loads costs a wait at
// its join) and is read from LDS (the table) or from pinned registers afterwards; the chain behind it waits for weight fragments and out_sp
// rows only.  TAPS is a template parameter for the same reason: the tap stores sit behind the arithmetic of their phase, with no test of a
// pointer between two loads.
template <bool TAPS>
__global__ __launch_bounds__(512, 4) void rn_fused_kernel(int E, int H, RnFusedArgs a)
{
    const CnStampScope stamp_scope(a.stamp);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __builtin_amdgcn_s_setprio(3); // critical path of the step: win the issue arbitration against the side stream's simulator wavefronts
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int e0 = blockIdx.x * TE;
    float *R0 = smem + O_R0, *R1 = smem + O_R1, *R2 = smem + O_R2, *R3 = smem + O_R3, *R4 = smem + O_R4, *R5 = smem + O_R5, *T = smem + O_T;
    const int w4 = wave & 3, hi = wave >> 2; // two groups of four wavefronts run independent products side by side
    // ---- the batch ----
    // the row offsets of this wavefront's two envs (written by the human-human kernel in front of this one: the plan's offsets or its own scan)
    int r0q[2], r1q[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int e = e0 + 2 * wave + q < E ? e0 + 2 * wave + q : E - 1;
        r0q[q] = a.row_off[e]; r1q[q] = a.row_off[e + 1];
    }
    // robot_linear.0 (thread = feature n, the two thread halves split the envs): its weights, and the observation of the half's 8 envs spread
    // over the lanes: lane l < 16 temporal word l, lane l < 56 robot_node word l (env l / 7).  The tail workgroup repeats env E - 1.
    const int n = tid & 255;
    float w[9];
#pragma unroll
    for (int d = 0; d < 9; ++d) w[d] = a.rl_w[n * 9 + d];
    float bn = a.rl_b[n];
    float obs_t, obs_r;
    {
        const int lt = lane < 16 ? lane : 15, lr = lane < 56 ? lane : 55;
        const int it = e0 + 8 * hi + (lt >> 1), ir = e0 + 8 * hi + lr / 7;
        obs_t = a.temporal[(size_t)(it < E ? it : E - 1) * 2 + (lt & 1)];
        obs_r = a.robot_node[(size_t)(ir < E ? ir : E - 1) * 7 + lr % 7];
    }
    // h_in: 4 words per thread
    float hx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = (tid >> 7) + 4 * k;
        hx[k] = a.hxs_in[(size_t)(e0 + i < E ? e0 + i : E - 1) * 128 + (tid & 127)];
    }
    // the table's vectors: the table is the concatenation of nine arrays, 736 float4, two per thread.  Array and offset are selected per lane
    // from local copies of the pointers: ?: over locals compiles to selects, over the argument's members to a tree of branches
    f32x4 tv[2];
    {
        const float *const p_teb = a.te_b, *const p_edgeb = a.edge_b, *const p_bih = a.bih, *const p_bhh = a.bhh, *const p_ac0b = a.ac0_b;
        const float *const p_a2b = a.a2_b, *const p_c2b = a.c2_b, *const p_clw = a.cl_w, *const p_fmw = a.fm_w;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int j = 512 * r + tid < T_VEC4 ? 512 * r + tid : T_VEC4 - 1, f = 4 * j;
            const float *src = p_teb; int first = T_TEB;
            src = f >= T_EDGEB ? p_edgeb : src; first = f >= T_EDGEB ? T_EDGEB : first;
            src = f >= T_BIH ? p_bih : src; first = f >= T_BIH ? T_BIH : first;
            src = f >= T_BHH ? p_bhh : src; first = f >= T_BHH ? T_BHH : first;
            src = f >= T_AC0B ? p_ac0b : src; first = f >= T_AC0B ? T_AC0B : first;
            src = f >= T_A2B ? p_a2b : src; first = f >= T_A2B ? T_A2B : first;
            src = f >= T_C2B ? p_c2b : src; first = f >= T_C2B ? T_C2B : first;
            src = f >= T_CLW ? p_clw : src; first = f >= T_CLW ? T_CLW : first;
            src = f >= T_FMW ? p_fmw : src; first = f >= T_FMW ? T_FMW : first;
            tv[r] = *reinterpret_cast<const f32x4 *>(src + (f - first));
        }
    }
    // the small words: one per lane (without eps its lanes re-read the mask)
    float smw;
    {
        const float *const p_masks = a.masks, *const p_eps = a.eps, *const p_clb = a.cl_b, *const p_fmb = a.fm_b, *const p_ls = a.logstd;
        const bool has_eps = p_eps != nullptr;
        const int sl = lane < SM_USED ? lane : SM_USED - 1;
        const int i = sl < SM_EPS ? sl : (sl - SM_EPS) >> 1;
        const int e = e0 + i < E ? e0 + i : E - 1;
        const bool is_eps = sl >= SM_EPS && has_eps;
        const float *src = is_eps ? p_eps : p_masks; int off = is_eps ? 2 * e + (sl & 1) : e; // (lanes >= SM_CLB: i = 16 .. 18, clamped like any env)
        src = sl >= SM_CLB ? p_clb : src; off = sl >= SM_CLB ? 0 : off;
        src = sl >= SM_FMB ? p_fmb : src; off = sl >= SM_FMB ? sl - SM_FMB : off;
        src = sl >= SM_LS ? p_ls : src; off = sl >= SM_LS ? sl - SM_LS : off;
        smw = src[off];
    }
    // ---- the one wait ----
#pragma unroll
    for (int d = 0; d < 9; ++d) w[d] = held(w[d]);
    bn = held(bn); obs_t = held(obs_t); obs_r = held(obs_r); smw = held(smw);
#pragma unroll
    for (int k = 0; k < 4; ++k) hx[k] = held(hx[k]);
#pragma unroll
    for (int r = 0; r < 2; ++r) tv[r] = held(tv[r]);
#pragma unroll
    for (int q = 0; q < 2; ++q) { r0q[q] = held_uniform(r0q[q]); r1q[q] = held_uniform(r1q[q]); } // scalar from here
    *reinterpret_cast<f32x4 *>(T + 4 * tid) = tv[0];
    if (512 + tid < T_VEC4) *reinterpret_cast<f32x4 *>(T + 4 * (512 + tid)) = tv[1];
    if (wave == 0) T[T_SM + lane] = smw;
#pragma unroll
    for (int k = 0; k < 4; ++k) R4[((tid >> 7) + 4 * k) * S128 + (tid & 127)] = hx[k];
    // ---- robot_linear.0: relu(W [256,9] . [temporal_edges(2) | robot_node(7)] + b) ----
    {
        float rs[TE / 2];
#pragma unroll
        for (int ii = 0; ii < TE / 2; ++ii) {
            float acc = bn;
            acc += wv_readlane(obs_t, 2 * ii) * w[0];
            acc += wv_readlane(obs_t, 2 * ii + 1) * w[1];
#pragma unroll
            for (int d = 0; d < 7; ++d) acc += wv_readlane(obs_r, 7 * ii + d) * w[2 + d];
            rs[ii] = fmaxf(acc, 0.0f);
            R0[(8 * hi + ii) * S512 + n] = rs[ii];
        }
        if (TAPS) {
#pragma unroll
            for (int ii = 0; ii < TE / 2; ++ii) {
                const int i = 8 * hi + ii;
                if (e0 + i < E) a.tap_robot[(size_t)(e0 + i) * 256 + n] = rs[ii];
            }
        }
    }
    __syncthreads();
    // ---- z = [u (256) | relu(enc) (64)] = te_w [320,256] . robot_states + te_b ;  gh = W_hh [384,128] . h_in (unmasked, no bias) ----
    // 20 feature blocks of 8 k-steps and 24 of 4, dealt so that every wavefront runs 8 k-steps: five wavefronts take four te blocks each,
    // three take eight W_hh blocks each in two calls
    if (wave < 5) {
        stage<256, 4, A_RELU, true>(a.f_te, wave, 5, T + T_TEB, R0, S512, R1, S512, 0, 256, lane);
    } else {
        stage<128, 4, A_NONE, false>(a.f_whh, wave - 5, 3, nullptr, R4, S128, R2, S384, 0, 0, lane);
        stage<128, 4, A_NONE, false>(a.f_whh, wave - 5 + 12, 3, nullptr, R4, S128, R2, S384, 0, 0, lane);
    }
    __syncthreads();
    // ---- robot-human attention (rn_chain.h): wavefront w owns envs 2w, 2w+1 ----
    rn_hr_attention<2, TAPS, false>(a, r0q, r1q, R1, S512, R0, S512, 2 * wave, e0, E, H, (float)H / 8.0f, lane);
    __syncthreads();
    // ---- edge = relu(edge_attention_embed [64,256] . hr + b) -> z[320:384] ----
    if (hi == 0) stage<256, 1, A_RELU, true>(a.f_edge, w4, 4, T + T_EDGEB, R0, S512, R1, S512, 320, 0, lane);
    __syncthreads();
    // ---- gi = W_ih [384,128] . [enc | edge] + b_ih ----
    stage<128, 3, A_NONE, true>(a.f_wih, wave, 8, T + T_BIH, R1 + 256, S512, R3, S384, 0, 0, lane);
    __syncthreads();
    // ---- GRU cell, pointwise part (gate order r,z,n; h and gh masked by the done mask: srnn_model.py:43-46) ----
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = (tid >> 7) + 4 * k, c = tid & 127;
        const float *gie = R3 + i * S384, *ghe = R2 + i * S384, *bhh = T + T_BHH;
        const float hnew = rn_gru_cell(gie[c], gie[128 + c], gie[256 + c], ghe[c], ghe[128 + c], ghe[256 + c], bhh[c], bhh[128 + c], bhh[256 + c],
                                       T[T_SM + SM_MASK + i], R4[i * S128 + c]);
        R5[i * S128 + c] = hnew;
        if (e0 + i < E) a.hxs_out[(size_t)(e0 + i) * 128 + c] = hnew;
    }
    __syncthreads();
    // ---- actor / critic trunks: tanh((W0 Wo) h + ..) [512,128], then the two [256,256] second layers ----
    stage<128, 4, A_TANH, true>(a.f_ac0, wave, 8, T + T_AC0B, R5, S128, R0, S512, 0, 0, lane);
    __syncthreads();
    {
        const float *fw = hi == 0 ? a.f_a2 : a.f_c2, *fb = hi == 0 ? T + T_A2B : T + T_C2B;
        const float *src = hi == 0 ? R0 : R0 + 256;
        stage<256, 4, A_TANH, true>(fw, w4, 4, fb, src, S512, R1, S512, hi * 256, 0, lane);
    }
    __syncthreads();
    // ---- critic_linear + DiagGaussian head (model.py:64-72): wavefront w owns envs 2w, 2w+1; every operand is in LDS ----
    for (int q = 0; q < 2; ++q) {
        const int i = 2 * wave + q;
        if (e0 + i >= E) break;
        const int e = e0 + i;
        const float *av = R1 + i * S512, *cv = av + 256, *cl_w = T + T_CLW, *fm_w = T + T_FMW, *sm = T + T_SM;
        float sv = 0.f, s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int d = lane + 64 * k;
            sv += cv[d] * cl_w[d];
            s0 += av[d] * fm_w[d];
            s1 += av[d] * fm_w[256 + d];
        }
        sv = wv_sum(sv); s0 = wv_sum(s0); s1 = wv_sum(s1);
        if (lane == 0) {
            a.value[e] = sv + sm[SM_CLB];
            if (a.action) {
                float a0, a1;
                const bool noise = a.eps != nullptr; // (without noise the eps words hold the masks again: not read)
                const float lp = rn_gauss_sample(s0 + sm[SM_FMB], s1 + sm[SM_FMB + 1], sm[SM_LS], sm[SM_LS + 1], noise, noise ? sm[SM_EPS + 2 * i] : 0.0f,
                                                 noise ? sm[SM_EPS + 2 * i + 1] : 0.0f, a0, a1);
                a.action[2 * e] = a0; a.action[2 * e + 1] = a1;
                a.logp[e] = lp;
            }
        }
        if (TAPS) {
#pragma unroll
            for (int k = 0; k < 4; ++k) a.tap_actor[(size_t)e * 256 + lane + 64 * k] = av[lane + 64 * k];
        }
    }
}

// fp32 row-major W [N,K] -> [fb = N/16][K/32][plane hi,lo][64 lanes][8 bf16]: lane (f, kk) holds W[16 fb + f][32 ks + 8 kk .. +7]
__global__ void rn_bake_kernel(int N, int K, const float *__restrict__ w, __bf16 *__restrict__ out)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; // one weight
    if (idx >= (size_t)N * K) return;
    const int u = idx & 7, lane = (idx >> 3) & 63;
    const size_t rest = idx >> 9;
    const int KS = K / 32;
    const int ks = (int)(rest % KS), fb = (int)(rest / KS);
    const float x = w[(size_t)(fb * 16 + (lane & 15)) * K + 32 * ks + 8 * (lane >> 4) + u];
    const __bf16 hi = (__bf16)x;
    const size_t base = (((size_t)fb * KS + ks) * 2) * 512 + lane * 8 + u;
    out[base] = hi;
    out[base + 512] = (__bf16)(x - (float)hi);
}

} // namespace

int rn_fused_bake(int N, int K, const float *w, float *out, hipStream_t st)
{
    CN_REQUIRE(N % 16 == 0 && K % 32 == 0, "rn_fused_bake: N must be a multiple of 16, K of 32");
    const size_t n = (size_t)N * K;
    hipLaunchKernelGGL(rn_bake_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, N, K, w, reinterpret_cast<__bf16 *>(out));
    CN_CHECK_LAUNCH();
    return CN_OK;
}

template <bool TAPS>
static int rn_fused_launch(int E, int H, const RnFusedArgs &a, hipStream_t st)
{
    constexpr size_t lds = (size_t)LDS_FLOATS * sizeof(float);
    if (int rc = cn_lds_opt_in<&rn_fused_kernel<TAPS>>((int)lds)) return rc;
    hipLaunchKernelGGL(rn_fused_kernel<TAPS>, dim3((E + TE - 1) / TE), dim3(512), lds, st, E, H, a);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

int rn_fused_forward(int E, int H, const RnFusedArgs &args, hipStream_t st)
{
    CN_REQUIRE(E >= 1, "rn_fused_forward: E must be positive");
    if (int rc = rn_check_args(args, "rn_fused_forward")) return rc;
    RnFusedArgs a = args;
    a.stamp = cn_stamp_slot(CN_K_RN_FUSED);
    return args.tap_robot ? rn_fused_launch<true>(E, H, a, st) : rn_fused_launch<false>(E, H, a, st);
}
