// rn_sized.hip -- the robot-node half of the policy forward as ONE kernel on gfx950, for network sizes other than the reference's default
// (cn_policy_create_sized: R = human_node_rnn_size, M = human_node_embedding_size, O = human_node_output_size at run time).  The chain is
// rn_fused.hip's:
//   robot_linear -> [u = Ws^T temporal_edge_layer(.) | encoder_linear] -> robot-human attention over out_sp -> edge_attention_embed ->
//   GRU cell (with the done mask) -> actor / critic trunks (output_linear folded in) -> critic_linear + DiagGaussian head
// and so is the arithmetic (rn_chain.h holds what the two kernels share): products as bf16x3 splits on v_mfma_f32_16x16x32_bf16 from rn_fused_bake's fragment images ("transposed": A operand =
// weight fragment, B operand = the envs' activations from LDS, the C layout is a float4 of four consecutive features of one env), small operands
// in exact fp32, rn_fused's exp2-based tanh / sigmoid.  What the run-time sizes change:
//   * the LDS images are laid out from (R, M, O) (RnLayout below), and a workgroup owns 16 envs only where sixteen images fit -- else 8, the MFMA's
//     other eight columns then repeat them and are not stored;
//   * the feature-block counts (256 + M) / 16, 3R / 16, 2O / 16, O / 16 are not multiples of the eight wavefronts: wavefront w takes the blocks
//     w, w + 8, ... of a stage in groups of up to four accumulators, the last group of a wavefront may hold one to three;
//   * K / 32 is a run-time trip count.  Every K here is a multiple of 64, so the k loop runs in pairs over two statically indexed fragment buffers
//     (the next k-step's fragments are in flight behind the current one's MFMAs; a run-time index would send the buffers to scratch).
// The default sizes never come here: they keep rn_fused_kernel, whose fixed shapes buy the one-batch operand fetch and the hand-dealt stages.
#include "rn_sized.h"
#include "rn_chain.h"

namespace {

// ---- LDS ----
// Per env, in floats (each image row is K + 4 floats, so that the 16 lanes of a float4 read hit distinct banks):
//   R0  max(256, 2O)       robot_states (256) -> hr (256) -> ac1 (2O)
//   R1  max(256 + 2M, 2O)  z = [u 256 | enc M | edge M] -> ac2 (2O)
//   R2, R3  3R             gh, gi
//   R4, R5  R              h_in, h_new
// plus one table for the workgroup: every bias, the head weights (256 + 2M + 6R + 7O floats) and 64 small words (masks, noise, head biases).
// Envs per workgroup: 16 if 16 envs' images and the table fit into the 160 KB a workgroup may have, else 8.  Worked example, the default sizes
// (128, 64, 256): 516 + 516 + 388 + 388 + 132 + 132 = 2072 floats per env, 16 envs = 33 152, table 3008 -> 36 160 floats = 144 640 B: 16 envs (that is
// rn_fused_kernel's own figure).  Largest corner (256, 128, 512): 1028 + 1028 + 772 + 772 + 260 + 260 = 4120 per env; 16 envs would be 286 464 B, 8 envs
// are 32 960 + 5696 floats = 154 624 B: 8 envs.
constexpr int LDS_LIMIT_BYTES = 160 * 1024;

struct RnLayout {
    int S0, S1, S2, S4;                          // row strides of R0, R1, R2 / R3, R4 / R5
    int oR0, oR1, oR2, oR3, oR4, oR5, oT;        // image offsets
    int tTEB, tEDGEB, tBIH, tBHH, tAC0B, tA2B, tC2B, tCLW, tFMW, tSM; // table offsets
    int total;                                   // floats
};
__host__ __device__ inline RnLayout rn_layout(int R, int M, int O, int te)
{
    RnLayout L;
    const int w0 = 256 > 2 * O ? 256 : 2 * O, w1 = 256 + 2 * M > 2 * O ? 256 + 2 * M : 2 * O;
    L.S0 = w0 + 4; L.S1 = w1 + 4; L.S2 = 3 * R + 4; L.S4 = R + 4;
    L.oR0 = 0; L.oR1 = L.oR0 + te * L.S0; L.oR2 = L.oR1 + te * L.S1; L.oR3 = L.oR2 + te * L.S2; L.oR4 = L.oR3 + te * L.S2; L.oR5 = L.oR4 + te * L.S4;
    L.oT = L.oR5 + te * L.S4;
    L.tTEB = 0; L.tEDGEB = L.tTEB + 256 + M; L.tBIH = L.tEDGEB + M; L.tBHH = L.tBIH + 3 * R; L.tAC0B = L.tBHH + 3 * R; L.tA2B = L.tAC0B + 2 * O;
    L.tC2B = L.tA2B + O; L.tCLW = L.tC2B + O; L.tFMW = L.tCLW + O; L.tSM = L.tFMW + 2 * O;
    L.total = L.oT + L.tSM + SM_WORDS;
    return L;
}

// NB feature blocks fb0, fb0 + fb_step, ... of one product: acc = W[fb] . x over KS k-steps (KS even), then bias / activation / store.
// W: baked fragments [fb][KS][plane hi,lo][64 lanes][8 bf16]; xrow: this lane's env row + 8 * (lane >> 4); orow: this lane's output row + out_off,
// or nullptr for the lanes whose env column is a repeat (8 envs per workgroup)
template <int NB, int ACT, bool BIAS>
__device__ __forceinline__ void stage_group(const bf16x8 *__restrict__ W, int fb0, int fb_step, int KS, const float *bias, const float *xrow, float *orow,
                                            int relu_from, int lane)
{
    const int g = lane >> 4;
    f32x4 acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 a0h[NB], a0l[NB], a1h[NB], a1l[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int base = ((fb0 + j * fb_step) * KS) * 128 + lane;
        a0h[j] = W[base]; a0l[j] = W[base + 64];
    }
    for (int ks = 0; ks < KS; ks += 2) {
        bf16x8 bh, bl;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int base = ((fb0 + j * fb_step) * KS + ks + 1) * 128 + lane;
            a1h[j] = W[base]; a1l[j] = W[base + 64];
        }
        rn_split(xrow, ks, bh, bl);
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            acc[j] = mfma32(a0l[j], bh, acc[j]);
            acc[j] = mfma32(a0h[j], bl, acc[j]);
            acc[j] = mfma32(a0h[j], bh, acc[j]);
        }
        const int kn = ks + 2 < KS ? ks + 2 : KS - 1; // (the last pair re-reads the last k-step: loaded, never used)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int base = ((fb0 + j * fb_step) * KS + kn) * 128 + lane;
            a0h[j] = W[base]; a0l[j] = W[base + 64];
        }
        rn_split(xrow, ks + 1, bh, bl);
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            acc[j] = mfma32(a1l[j], bh, acc[j]);
            acc[j] = mfma32(a1h[j], bl, acc[j]);
            acc[j] = mfma32(a1h[j], bh, acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) rn_epilogue<ACT, BIAS>(acc[j], (fb0 + j * fb_step) * 16 + 4 * g, bias, relu_from, orow);
}

// out[env][out_off + f] = act(W . in[env] + bias) for all nfb feature blocks of 16: wavefront w takes the blocks (w + rot) % 8, + 8, + 16, ...
// (rot staggers two products that run back to back, so that their ragged tails do not land on the same wavefronts), in groups of four, the
// rest as one group of one to three.  wave and every count are wave-uniform: the branches are scalar.
template <int ACT, bool BIAS>
__device__ __forceinline__ void stage(const float *__restrict__ Wfrag, int nfb, int K, const float *bias, const float *in, int in_stride, float *out,
                                      int out_stride, int out_off, int relu_from, int te, int wave, int rot, int lane)
{
    const bf16x8 *__restrict__ W = reinterpret_cast<const bf16x8 *>(Wfrag);
    const int KS = K >> 5, i = lane & 15, g = lane >> 4;
    const float *xrow = in + (i & (te - 1)) * in_stride + 8 * g;
    float *orow = i < te ? out + i * out_stride + out_off : nullptr;
    int fb = (wave + rot) & 7;
    for (; fb + 24 < nfb; fb += 32) stage_group<4, ACT, BIAS>(W, fb, 8, KS, bias, xrow, orow, relu_from, lane);
    if (fb + 16 < nfb) stage_group<3, ACT, BIAS>(W, fb, 8, KS, bias, xrow, orow, relu_from, lane);
    else if (fb + 8 < nfb) stage_group<2, ACT, BIAS>(W, fb, 8, KS, bias, xrow, orow, relu_from, lane);
    else if (fb < nfb) stage_group<1, ACT, BIAS>(W, fb, 8, KS, bias, xrow, orow, relu_from, lane);
}

// the robot-human attention of this wavefront's PER envs: their row offsets (the tail workgroup repeats env E - 1), then the shared block
template <int PER, bool TAPS>
__device__ __forceinline__ void hr_attention(const RnFusedArgs &a, const float *R1, int S1, float *R0, int S0, int wave, int e0, int E, int H, float scale,
                                             int lane)
{
    int r0q[PER], r1q[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int e = e0 + PER * wave + q < E ? e0 + PER * wave + q : E - 1;
        r0q[q] = __builtin_amdgcn_readfirstlane(a.row_off[e]); r1q[q] = __builtin_amdgcn_readfirstlane(a.row_off[e + 1]);
    }
    rn_hr_attention<PER, TAPS, true>(a, r0q, r1q, R1, S1, R0, S0, PER * wave, e0, E, H, scale, lane);
}

// No register target: the LDS leaves one workgroup per CU, so its eight wavefronts may take 256 registers each.  The compiler's figures per
// instantiation are in DESIGN.md section 4; no scratch (every register array above is statically indexed).
template <bool TAPS>
__global__ __launch_bounds__(512) void rn_sized_kernel(int E, int H, RnFusedArgs a, RnSizedDims d)
{
    const CnStampScope stamp_scope(a.stamp);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int R = d.R, M = d.M, O = d.O, te = d.te;
    const RnLayout L = rn_layout(R, M, O, te);
    const int e0 = blockIdx.x * te;
    float *R0 = smem + L.oR0, *R1 = smem + L.oR1, *R2 = smem + L.oR2, *R3 = smem + L.oR3, *R4 = smem + L.oR4, *R5 = smem + L.oR5, *T = smem + L.oT;
    // ---- the table: nine arrays back to back (every length a multiple of 64 floats), then the small words ----
    for (int j = tid; 4 * j < L.tSM; j += 512) {
        const int f = 4 * j;
        const float *src = a.te_b; int first = L.tTEB;
        if (f >= L.tEDGEB) { src = a.edge_b; first = L.tEDGEB; }
        if (f >= L.tBIH) { src = a.bih; first = L.tBIH; }
        if (f >= L.tBHH) { src = a.bhh; first = L.tBHH; }
        if (f >= L.tAC0B) { src = a.ac0_b; first = L.tAC0B; }
        if (f >= L.tA2B) { src = a.a2_b; first = L.tA2B; }
        if (f >= L.tC2B) { src = a.c2_b; first = L.tC2B; }
        if (f >= L.tCLW) { src = a.cl_w; first = L.tCLW; }
        if (f >= L.tFMW) { src = a.fm_w; first = L.tFMW; }
        *reinterpret_cast<f32x4 *>(T + f) = *reinterpret_cast<const f32x4 *>(src + (f - first));
    }
    if (tid < SM_WORDS) { // masks (te) | eps (2 te, zero without noise) | cl_b | fm_b (2) | logstd (2); the tail workgroup repeats env E - 1
        float v = 0.0f;
        if (tid < te) v = a.masks[e0 + tid < E ? e0 + tid : E - 1];
        else if (tid >= SM_EPS && tid < SM_EPS + 2 * te) {
            const int i = (tid - SM_EPS) >> 1, e = e0 + i < E ? e0 + i : E - 1;
            if (a.eps) v = a.eps[2 * e + (tid & 1)];
        } else if (tid == SM_CLB) v = a.cl_b[0];
        else if (tid >= SM_FMB && tid < SM_FMB + 2) v = a.fm_b[tid - SM_FMB];
        else if (tid >= SM_LS && tid < SM_LS + 2) v = a.logstd[tid - SM_LS];
        T[L.tSM + tid] = v;
    }
    for (int idx = tid; idx < te * R; idx += 512) {
        const int i = idx / R, c = idx - i * R;
        R4[i * L.S4 + c] = a.hxs_in[(size_t)(e0 + i < E ? e0 + i : E - 1) * R + c];
    }
    // ---- robot_linear.0: relu(W [256,9] . [temporal_edges(2) | robot_node(7)] + b); thread = feature n, the two thread halves split the envs ----
    {
        const int n = tid & 255, half = tid >> 8, per = te >> 1;
        float w[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) w[k] = a.rl_w[n * 9 + k];
        const float bn = a.rl_b[n];
        for (int ii = 0; ii < per; ++ii) {
            const int i = half * per + ii, e = e0 + i < E ? e0 + i : E - 1;
            float acc = bn;
            acc += a.temporal[(size_t)e * 2] * w[0];
            acc += a.temporal[(size_t)e * 2 + 1] * w[1];
#pragma unroll
            for (int k = 0; k < 7; ++k) acc += a.robot_node[(size_t)e * 7 + k] * w[2 + k];
            const float rs = fmaxf(acc, 0.0f);
            R0[i * L.S0 + n] = rs;
            if (TAPS && e0 + i < E) a.tap_robot[(size_t)(e0 + i) * 256 + n] = rs;
        }
    }
    __syncthreads();
    // ---- z = [u (256) | relu(enc) (M)] = te_w [256 + M, 256] . robot_states + te_b ;  gh = W_hh [3R, R] . h_in (unmasked, no bias) ----
    stage<A_RELU, true>(a.f_te, (256 + M) >> 4, 256, T + L.tTEB, R0, L.S0, R1, L.S1, 0, 256, te, wave, 0, lane);
    stage<A_NONE, false>(a.f_whh, (3 * R) >> 4, R, nullptr, R4, L.S4, R2, L.S2, 0, 0, te, wave, ((256 + M) >> 4) & 7, lane);
    __syncthreads();
    // ---- robot-human attention (rn_chain.h): wavefront w owns te / 8 envs ----
    if (te == 16) hr_attention<2, TAPS>(a, R1, L.S1, R0, L.S0, wave, e0, E, H, d.scale, lane);
    else hr_attention<1, TAPS>(a, R1, L.S1, R0, L.S0, wave, e0, E, H, d.scale, lane);
    __syncthreads();
    // ---- edge = relu(edge_attention_embed [M,256] . hr + b) -> z[256 + M : 256 + 2M] ----
    stage<A_RELU, true>(a.f_edge, M >> 4, 256, T + L.tEDGEB, R0, L.S0, R1, L.S1, 256 + M, 0, te, wave, 0, lane);
    __syncthreads();
    // ---- gi = W_ih [3R, 2M] . [enc | edge] + b_ih ----
    stage<A_NONE, true>(a.f_wih, (3 * R) >> 4, 2 * M, T + L.tBIH, R1 + 256, L.S1, R3, L.S2, 0, 0, te, wave, 0, lane);
    __syncthreads();
    // ---- GRU cell, pointwise part (gate order r,z,n; h and gh masked by the done mask: srnn_model.py:43-46) ----
    for (int idx = tid; idx < te * R; idx += 512) {
        const int i = idx / R, c = idx - i * R;
        const float *gie = R3 + i * L.S2, *ghe = R2 + i * L.S2, *bhh = T + L.tBHH;
        const float hnew = rn_gru_cell(gie[c], gie[R + c], gie[2 * R + c], ghe[c], ghe[R + c], ghe[2 * R + c], bhh[c], bhh[R + c], bhh[2 * R + c],
                                       T[L.tSM + SM_MASK + i], R4[i * L.S4 + c]);
        R5[i * L.S4 + c] = hnew;
        if (e0 + i < E) a.hxs_out[(size_t)(e0 + i) * R + c] = hnew;
    }
    __syncthreads();
    // ---- actor / critic trunks: tanh((W0 Wo) h + ..) [2O, R], then the two [O, O] second layers ----
    stage<A_TANH, true>(a.f_ac0, (2 * O) >> 4, R, T + L.tAC0B, R5, L.S4, R0, L.S0, 0, 0, te, wave, 0, lane);
    __syncthreads();
    stage<A_TANH, true>(a.f_a2, O >> 4, O, T + L.tA2B, R0, L.S0, R1, L.S1, 0, 0, te, wave, 0, lane);
    stage<A_TANH, true>(a.f_c2, O >> 4, O, T + L.tC2B, R0 + O, L.S0, R1, L.S1, O, 0, te, wave, (O >> 4) & 7, lane);
    __syncthreads();
    // ---- critic_linear + DiagGaussian head (model.py:64-72): wavefront w owns te / 8 envs; every operand is in LDS ----
    {
        const int per = te >> 3;
        for (int q = 0; q < per; ++q) {
            const int i = per * wave + q;
            if (e0 + i >= E) break;
            const int e = e0 + i;
            const float *av = R1 + i * L.S1, *cv = av + O, *cl_w = T + L.tCLW, *fm_w = T + L.tFMW, *sm = T + L.tSM;
            float sv = 0.f, s0 = 0.f, s1 = 0.f;
            for (int c = lane; c < O; c += 64) {
                sv += cv[c] * cl_w[c];
                s0 += av[c] * fm_w[c];
                s1 += av[c] * fm_w[O + c];
            }
            sv = wv_sum(sv); s0 = wv_sum(s0); s1 = wv_sum(s1);
            if (lane == 0) {
                a.value[e] = sv + sm[SM_CLB];
                if (a.action) {
                    float a0, a1; // (the eps words are zero without noise)
                    const float lp = rn_gauss_sample(s0 + sm[SM_FMB], s1 + sm[SM_FMB + 1], sm[SM_LS], sm[SM_LS + 1], a.eps != nullptr, sm[SM_EPS + 2 * i],
                                                     sm[SM_EPS + 2 * i + 1], a0, a1);
                    a.action[2 * e] = a0; a.action[2 * e + 1] = a1;
                    a.logp[e] = lp;
                }
            }
            if (TAPS)
                for (int c = lane; c < O; c += 64) a.tap_actor[(size_t)e * O + c] = av[c];
        }
    }
}

bool sizes_in_box(int R, int M, int O) { return (R == 64 || R == 128 || R == 192 || R == 256) && (M == 64 || M == 128) && O >= 64 && O <= 512 && O % 64 == 0; }

} // namespace

int rn_sized_envs_per_group(int R, int M, int O)
{
    if (!sizes_in_box(R, M, O)) return 0;
    return (size_t)rn_layout(R, M, O, 16).total * sizeof(float) <= (size_t)LDS_LIMIT_BYTES ? 16 : 8;
}

size_t rn_sized_lds_bytes(int R, int M, int O, int te) { return (size_t)rn_layout(R, M, O, te).total * sizeof(float); }

template <bool TAPS>
static int rn_sized_launch(int E, int H, const RnFusedArgs &a, const RnSizedDims &d, size_t lds, hipStream_t st)
{
    if (int rc = cn_lds_opt_in<&rn_sized_kernel<TAPS>>(LDS_LIMIT_BYTES)) return rc;
    hipLaunchKernelGGL(rn_sized_kernel<TAPS>, dim3((E + d.te - 1) / d.te), dim3(512), lds, st, E, H, a, d);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

int rn_sized_forward(int E, int H, const RnFusedArgs &args, const RnSizedDims &dims, hipStream_t st)
{
    CN_REQUIRE(E >= 1 && H >= 1 && H <= CN_MAX_HUMANS, "rn_sized_forward: E must be positive, H in [1,%d]", CN_MAX_HUMANS);
    const int te = rn_sized_envs_per_group(dims.R, dims.M, dims.O);
    CN_REQUIRE(te != 0 && te == dims.te, "rn_sized_forward: sizes (%d, %d, %d) outside the box, or envs per workgroup %d not the layout's", dims.R, dims.M, dims.O, dims.te);
    const size_t lds = rn_sized_lds_bytes(dims.R, dims.M, dims.O, te);
    CN_REQUIRE(lds <= (size_t)LDS_LIMIT_BYTES, "rn_sized_forward: %zu B of LDS exceed the workgroup's 160 KB", lds);
    if (int rc = rn_check_args(args, "rn_sized_forward")) return rc;
    RnFusedArgs a = args;
    a.stamp = cn_stamp_slot(CN_K_RN_FUSED);
    return args.tap_robot ? rn_sized_launch<true>(E, H, a, dims, lds, st) : rn_sized_launch<false>(E, H, a, dims, lds, st);
}
