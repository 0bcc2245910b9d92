// policy.hip -- the attention-interaction-graph policy (selfAttn_merge_srnn + DiagGaussian) on gfx950, host side.  The file serves both
// the rollout (the cn_policy object: one forward per env step) and the PPO update (the stand-alone entry points that train_step.hip and
// the host mirror's autograd Functions call on whole minibatches).  It is ONE translation unit: its kernels live in headers that only
// this file includes, and the kernels both halves launch (hh_attention_kernel's four size classes, hr_attention_kernel,
// robot_embed_kernel, gemm_nt_kernel<64,64,ACT_RELU>) are compiled once.
// Reference: rl/networks/selfAttn_srnn_temp_node.py:360-449, rl/networks/model.py:56-90.
//
// Files:
//   policy_kernels.h  row compaction (row_offsets, compact_visible, scatter_rows), embed0 / robot_embed (K = D <= 16 and 9: VALU),
//                     gru_pointwise, gauss_head, the fp64 weight folds, align_up
//   attention.h       human-human attention per (env, head) in size classes of 8 / 16 / 32 / 64 humans with its VALU and MFMA backward
//                     kernels and launchers; robot-human attention forward and backward
//   rn_train.h        cn_rn_seq_*'s value / log-prob head on given actions, its backward, the row reduction, robot_linear.0's weight gradient
//   gemm.h            exact-fp32 MFMA GEMM (v_mfma_f32_32x32x2_f32): per-env layers, big layers in gemm mode 0
//   gemm3.h           bf16x3 split-precision NT GEMM of the big layers in gemm mode 1 (arithmetic: split_bf16.h) and the weight split
//   hh_fused.h, rn_fused.h   interfaces of the two fused kernels of gemm mode 2 (hh_fused.hip, rn_fused.hip: objects of their own)
//   rn_sized.h        interface of the robot-node kernel with run-time network sizes (rn_sized.hip): gemm mode 2 of a cn_policy_create_sized handle
//   rn_chain.h        the robot-node chain's arithmetic, stated once for rn_fused.hip and rn_sized.hip; here (through policy_kernels.h and
//                     rn_train.h) for the DiagGaussian sample / log-prob of gauss_head_kernel and rn_head_fwd_kernel
//   policy.hip        part 1, rollout: cn_policy, cn_policy_set_weights (copies, folds, splits, fragment images), policy_forward, taps, profiling
//                     part 2, training: cn_hh_block_fwd, cn_obs_compact_visible, cn_hh_attention_*, cn_hr_attention_*, cn_rn_seq_* and the
//                     rn_seq_*_impl / rn_seq_prep_jobs that train_internal.h declares.  Its big products go to linear.hip (cn_linear_*).
//
// Rollout pipeline per call (E envs, H humans, M = E*H rows), all on the caller's stream, no host sync; in the default gemm mode 2 the
// human-human lines are ONE launch (hh_fused.hip) and the robot-node lines another (rn_fused.hip), in modes 0 / 1 each line is a launch:
//   embed0        [M,D]   -> [M,128]  ReLU                      (K = 2 or 12: VALU)
//   gemm          [M,128] -> [M,512]  ReLU                      embedding_layer.2
//   gemm          [M,512] -> [M,1536]                           folded (q|k|v)_linear ∘ in_proj, 1/sqrt(64) folded into q
//   hh_attention  per (env, head): softmax(QK^T + key padding mask) V  -> [M,512]
//   gemm          [M,512] -> [M,256]  ReLU                      folded out_proj ∘ spatial_linear
//   robot_embed   [E,9]   -> [E,256]  ReLU ; gemm -> [E,256]    robot_linear, u = spatial_edge_layer^T temporal_edge_layer(.)
//   hr_attention  per env: scores u . out_sp_j, masked softmax over humans, weighted sum of [H,256]
//   gemms + gru_pointwise + gemms(tanh) + gauss_head            EndRNN, actor/critic, DiagGaussian
// The reference computes in fp32 and the parity bar is 1e-4, which plain bf16 inputs cannot hold at K = 512.  The three
// large products (embedding_layer.2, q|k|v, out_proj∘spatial_linear) therefore run as bf16x3 split-precision MFMA
// (split_bf16.h: hi/lo bf16 pairs, three v_mfma_f32_32x32x16_bf16 per term, fp32 accumulate, ~2e-5 from fp32; default) or as
// exact fp32 MFMA (cn_policy_set_gemm_mode(p, 0)); every other product is exact fp32 on v_mfma_f32_32x32x2_f32 (gemm.h).
// The rows of the human-human block are the compacted "live" (env, human) rows only, the robot-node launches run on a side
// stream beside that block.
// The two affine pairs without a nonlinearity in between are folded once per weight snapshot (fp64 accumulation),
// which removes 4 of the 9 [M,512]x[512,512] products (83.65 -> 52.2 MFLOP per env-step at H = 20).
#include "common.h"
#include "gemm.h"
#include "gemm3.h"
#include "policy_kernels.h"
#include "attention.h"
#include "rn_train.h"
#include "hh_fused.h"
#include "rn_fused.h"
#include "rn_sized.h"
#include "row_plan.h"
#include "train_internal.h"

#include <cmath>
#include <cstddef>
#include <new>
#include <vector>

// =================================================================================================================================
// Part 1 -- rollout: the cn_policy object
// =================================================================================================================================
struct cn_policy {
    int H, D, maxE;
    // cn_policy_dims: R = human_node_rnn_size, Mb = human_node_embedding_size, A = attention_size, O = human_node_output_size (128 / 64 / 64 / 256)
    int R, Mb, A, O;
    bool sized;       // any of them off its default: the robot-node half of gemm mode 2 runs on rn_sized.hip
    int rn_te;        // ... with this many envs per workgroup (rn_sized_envs_per_group)
    float hr_scale;   // robot-human score scale (float)((double)H / sqrt((double)A)): H / 8 at the default
    bool weights_set;
    char *blob;
    // weight snapshot (device)
    float *emb0_w, *emb0_b, *emb2_w, *emb2_b;
    float *qkv_w, *qkv_b;   // folded [1536,512], [1536]
    float *os_w, *os_b;     // folded out_proj∘spatial_linear [256,512], [256]
    float *as_w, *as_b;     // attn.spatial_edge_layer [A,256]
    float *at_w, *at_b;     // attn.temporal_edge_layer [A,256]
    float *rl_w, *rl_b;     // robot_linear [256,9]
    float *enc_w, *enc_b, *edge_w, *edge_b; // [Mb,256] each
    float *wih, *whh, *bih, *bhh;           // GRU [3R,2Mb], [3R,R]
    float *out_w, *out_b;                   // [O,R]
    float *ac0_w, *ac0_b;                   // concat(actor.0, critic.0) [2O,O]
    float *a2_w, *a2_b, *c2_w, *c2_b;       // [O,O]
    float *cl_w, *cl_b, *fm_w, *fm_b, *logstd;
    float *te_w, *te_b;       // [spatial_edge_layer^T * temporal_edge_layer (u, 256 rows) ; encoder_linear (Mb rows)] stacked [256 + Mb,256]
    float *ac0f_w, *ac0f_b;   // (actor.0 ; critic.0) folded with output_linear [2O,R]
    float *z;                 // [E,256 + 2Mb] = [u | relu(enc) | relu(edge)]
    // activations
    float *emb1, *emb2, *qkv, *attn, *out_sp;
    __bf16 *emb2_hi, *emb2_lo, *qkv_hi, *qkv_lo, *os_hi, *os_lo; // split copies of the three big weight matrices
    float *r_te, *r_whh, *r_edge, *r_wih, *r_ac0, *r_a2, *r_c2; // MFMA-fragment images of the robot-node weights (rn_fused.hip)
    bool self_attn = true;       // args.use_self_attn: false = spatial_linear is a two-layer MLP on the spatial edges (cn_policy_set_self_attention)
    bool taps_on;                // fused mode: write the test taps (robot_emb, hr_attn, hr_out, actor_feat) of every forward
    void *f_emb2, *f_qkv, *f_os; // MFMA-fragment images of the three big weight matrices for the fused human-human kernel
    int gemm_mode; // 0 = exact fp32 MFMA, 1 = bf16x3 split as separate launches, 2 = bf16x3 split, fused human-human kernel (default)
    unsigned long long *live_total; // device counter: sum of live rows over the profiled forwards
    int *row_off; // [maxE + 1]
    int *cls_cnt, *cls_list; // big attention size classes: [2] counts, [2][E] env lists exclusive prefix of live humans per env; row_off[E] = live rows
    float *robot_states, *t_emb, *hr_out, *hr_attn, *x, *gi, *gh, *hnew, *rnn_out, *ac1, *ac2;
    // robot-side launches that do not depend on the human-human block run on this stream, beside the big GEMMs
    hipStream_t side;
    hipEvent_t ev_fork, ev_join;
    // profiling of the dominant kernel: every prof_every-th forward is bracketed by a pair of events (an event record on the
    // critical stream costs a few microseconds of dispatch gap, so the bracket is sampled, not put around every launch)
    bool profiling;       // THIS forward is bracketed
    int prof_every;       // 0 = off
    long long prof_tick;
    static constexpr int PROF_RING = 64;
    hipEvent_t ev[PROF_RING][2]; // ring of (start, stop) pairs around the QKV projection launch
    int ev_head, ev_tail;        // [tail, head) are recorded but not yet harvested
    double prof_ms[8];
    int64_t prof_n[8];
    std::vector<float> prof_samples; // the harvested brackets one by one [ms], in launch order (cn_policy_get_profile_samples)
    // called right behind the launch of the human-human kernel (cn_policy_set_post_hh_hook): side work that must not reach the CUs before it
    int (*post_hh_hook)(void *arg, void *stream);
    void *post_hh_arg;
};

// big-M GEMMs (rows = live humans): 128-row tiles
template <int BN, int ACT>
static int launch_gemm(int M, int N, int K, const float *A, int lda, const float *W, const float *bias, float *C, int ldc, hipStream_t st,
                       const int *m_dev = nullptr)
{
    return launch_gemm_t<128, BN, ACT>(M, N, K, A, lda, W, bias, C, ldc, st, m_dev, 1, GemmBatch{0, 0, 0, 0}, 1 << 30);
}
// per-env GEMMs (rows = envs, a few thousand): 64 x 64 tiles so that the launch still fills the 256 CUs
template <int ACT>
static int launch_gemm_env(int M, int N, int K, const float *A, int lda, const float *W, const float *bias, float *C, int ldc, hipStream_t st,
                           int nbatch = 1, GemmBatch gb = GemmBatch{0, 0, 0, 0}, int relu_from = 1 << 30)
{
    return launch_gemm_t<64, 64, ACT>(M, N, K, A, lda, W, bias, C, ldc, st, nullptr, nbatch, gb, relu_from);
}

// The sizes are checked by the callers: cn_policy_create passes the default, cn_policy_create_sized its box.
static int policy_create(int human_num, int edge_width, int max_envs, int dR, int dM, int dA, int dO, cn_policy **out)
{
    if (int rc = cn_require_device()) return rc;
    CN_REQUIRE(out, "cn_policy_create: null out");
    CN_REQUIRE(human_num >= 1 && human_num <= CN_MAX_HUMANS, "cn_policy_create: human_num must be in [1,%d]", CN_MAX_HUMANS);
    CN_REQUIRE(edge_width >= 1 && edge_width <= 16, "cn_policy_create: edge_width must be in [1,16]");
    CN_REQUIRE(max_envs >= 1, "cn_policy_create: max_envs must be positive");
    cn_policy *p = new (std::nothrow) cn_policy{};
    CN_REQUIRE(p, "cn_policy_create: out of host memory");
    p->H = human_num; p->D = edge_width; p->maxE = max_envs;
    p->R = dR; p->Mb = dM; p->A = dA; p->O = dO;
    p->sized = !(dR == 128 && dM == 64 && dA == 64 && dO == 256);
    p->rn_te = p->sized ? rn_sized_envs_per_group(dR, dM, dO) : 16;
    p->hr_scale = (float)((double)human_num / sqrt((double)dA)); // the reference forms it in double and multiplies a float32 tensor by it
    const size_t E = max_envs, M = E * human_num, D = edge_width;
    const size_t R = dR, Mb = dM, A = dA, O = dO; // at the default every size below is the literal it used to be
    size_t off = 0;
    auto carve = [&](size_t nfloat) { size_t o = off; off += align_up(nfloat * sizeof(float)); return o; };
    const size_t o_emb0w = carve(128 * D), o_emb0b = carve(128), o_emb2w = carve(512 * 128), o_emb2b = carve(512);
    const size_t o_qkvw = carve(1536 * 512), o_qkvb = carve(1536), o_osw = carve(256 * 512), o_osb = carve(256);
    const size_t o_asw = carve(A * 256), o_asb = carve(A), o_atw = carve(A * 256), o_atb = carve(A);
    const size_t o_rlw = carve(256 * 9), o_rlb = carve(256);
    const size_t o_encw = carve(Mb * 256), o_encb = carve(Mb), o_edgew = carve(Mb * 256), o_edgeb = carve(Mb);
    const size_t o_wih = carve(3 * R * 2 * Mb), o_whh = carve(3 * R * R), o_bih = carve(3 * R), o_bhh = carve(3 * R);
    const size_t o_outw = carve(O * R), o_outb = carve(O);
    const size_t o_ac0w = carve(2 * O * O), o_ac0b = carve(2 * O);
    const size_t o_a2w = carve(O * O), o_a2b = carve(O), o_c2w = carve(O * O), o_c2b = carve(O);
    const size_t o_clw = carve(O), o_clb = carve(1), o_fmw = carve(2 * O), o_fmb = carve(2), o_ls = carve(2);
    const size_t o_emb1 = carve(M * 128), o_emb2 = carve(M * 512), o_qkv = carve(M * 1536), o_attn = carve(M * 512);
    const size_t o_outsp = carve(M * 256);
    const size_t o_rs = carve(E * 256), o_temb = carve(E * A), o_hr = carve(E * 256), o_hra = carve(M), o_x = carve(E * 2 * Mb);
    const size_t o_gi = carve(E * 3 * R), o_gh = carve(E * 3 * R), o_hn = carve(E * R), o_ro = carve(E * O);
    const size_t o_ac1 = carve(E * 2 * O), o_ac2 = carve(E * 2 * O);
    const size_t o_roff = carve(E + 1);
    const size_t o_live = carve(2);
    const size_t o_ccnt = carve(2), o_clist = carve(2 * E);
    const size_t o_tew = carve((256 + Mb) * 256), o_teb = carve(256 + Mb), o_acfw = carve(2 * O * R), o_acfb = carve(2 * O), o_z = carve(E * (256 + 2 * Mb));
    const size_t o_e2h = carve(512 * 128 / 2), o_e2l = carve(512 * 128 / 2), o_qh = carve(1536 * 512 / 2), o_ql = carve(1536 * 512 / 2);
    const size_t o_osh = carve(256 * 512 / 2), o_osl = carve(256 * 512 / 2);
    const size_t o_rte = carve((256 + Mb) * 256), o_rwhh = carve(3 * R * R), o_redge = carve(Mb * 256), o_rwih = carve(3 * R * 2 * Mb), o_rac0 = carve(2 * O * R);
    const size_t o_ra2 = carve(O * O), o_rc2 = carve(O * O);
    const size_t o_fe2 = carve(HH_EMB2_FRAG_BYTES / 4), o_fqkv = carve(HH_QKV_FRAG_BYTES / 4), o_fos = carve(HH_OS_FRAG_BYTES / 4);
    char *base = nullptr;
    hipError_t herr = hipMalloc((void **)&base, off);
    if (herr != hipSuccess) { delete p; cn_set_error("cn_policy_create: hipMalloc(%zu) failed: %s", off, hipGetErrorString(herr)); return CN_ERR_HIP; }
    p->blob = base;
    auto F = [&](size_t o) { return (float *)(base + o); };
    p->emb0_w = F(o_emb0w); p->emb0_b = F(o_emb0b); p->emb2_w = F(o_emb2w); p->emb2_b = F(o_emb2b);
    p->qkv_w = F(o_qkvw); p->qkv_b = F(o_qkvb); p->os_w = F(o_osw); p->os_b = F(o_osb);
    p->as_w = F(o_asw); p->as_b = F(o_asb); p->at_w = F(o_atw); p->at_b = F(o_atb);
    p->rl_w = F(o_rlw); p->rl_b = F(o_rlb); p->enc_w = F(o_encw); p->enc_b = F(o_encb); p->edge_w = F(o_edgew); p->edge_b = F(o_edgeb);
    p->wih = F(o_wih); p->whh = F(o_whh); p->bih = F(o_bih); p->bhh = F(o_bhh); p->out_w = F(o_outw); p->out_b = F(o_outb);
    p->ac0_w = F(o_ac0w); p->ac0_b = F(o_ac0b); p->a2_w = F(o_a2w); p->a2_b = F(o_a2b); p->c2_w = F(o_c2w); p->c2_b = F(o_c2b);
    p->cl_w = F(o_clw); p->cl_b = F(o_clb); p->fm_w = F(o_fmw); p->fm_b = F(o_fmb); p->logstd = F(o_ls);
    p->emb1 = F(o_emb1); p->emb2 = F(o_emb2); p->qkv = F(o_qkv); p->attn = F(o_attn); p->out_sp = F(o_outsp);
    p->robot_states = F(o_rs); p->t_emb = F(o_temb); p->hr_out = F(o_hr); p->hr_attn = F(o_hra); p->x = F(o_x);
    p->gi = F(o_gi); p->gh = F(o_gh); p->hnew = F(o_hn); p->rnn_out = F(o_ro); p->ac1 = F(o_ac1); p->ac2 = F(o_ac2);
    p->row_off = (int *)(base + o_roff);
    p->live_total = (unsigned long long *)(base + o_live);
    p->cls_cnt = (int *)(base + o_ccnt); p->cls_list = (int *)(base + o_clist);
    (void)hipMemset(p->live_total, 0, 8);
    p->emb2_hi = (__bf16 *)(base + o_e2h); p->emb2_lo = (__bf16 *)(base + o_e2l); p->qkv_hi = (__bf16 *)(base + o_qh); p->qkv_lo = (__bf16 *)(base + o_ql);
    p->os_hi = (__bf16 *)(base + o_osh); p->os_lo = (__bf16 *)(base + o_osl);
    p->r_te = F(o_rte); p->r_whh = F(o_rwhh); p->r_edge = F(o_redge); p->r_wih = F(o_rwih); p->r_ac0 = F(o_rac0); p->r_a2 = F(o_ra2); p->r_c2 = F(o_rc2);
    p->taps_on = true;
    p->f_emb2 = base + o_fe2; p->f_qkv = base + o_fqkv; p->f_os = base + o_fos;
    p->gemm_mode = 2;
    p->te_w = F(o_tew); p->te_b = F(o_teb); p->ac0f_w = F(o_acfw); p->ac0f_b = F(o_acfb); p->z = F(o_z);
    p->weights_set = false;
    p->profiling = false; p->prof_every = 0; p->prof_tick = 0;
    p->ev_head = p->ev_tail = 0;
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest); // side work yields to the caller's stream (critical path)
    if (hipStreamCreateWithPriority(&p->side, hipStreamNonBlocking, prio_least) != hipSuccess || hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming) != hipSuccess) {
        (void)hipFree(base); delete p; cn_set_error("cn_policy_create: side stream / event creation failed"); return CN_ERR_HIP;
    }
    for (int i = 0; i < cn_policy::PROF_RING; ++i)
        if (hipEventCreate(&p->ev[i][0]) != hipSuccess || hipEventCreate(&p->ev[i][1]) != hipSuccess) {
            (void)hipFree(base); delete p; cn_set_error("cn_policy_create: hipEventCreate failed"); return CN_ERR_HIP;
        }
    *out = p;
    return CN_OK;
}

extern "C" int cn_policy_create(int human_num, int edge_width, int max_envs, cn_policy **out)
{
    return policy_create(human_num, edge_width, max_envs, 128, 64, 64, 256, out);
}

extern "C" int cn_policy_create_sized(int human_num, int edge_width, int max_envs, const cn_policy_dims *dims, cn_policy **out)
{
    if (!dims) return cn_policy_create(human_num, edge_width, max_envs, out);
    const int R = dims->rnn_size, M = dims->embedding_size, A = dims->attention_size, O = dims->output_size;
    // multiples of 64: launch_gemm_env needs N % 64, rn_fused_bake N % 16 and K % 32 (and the sized kernel pairs its k-steps: K % 64)
    CN_REQUIRE((R == 64 || R == 128 || R == 192 || R == 256) && (M == 64 || M == 128) && O >= 64 && O <= 512 && O % 64 == 0 && A >= 1 && A <= 256,
               "cn_policy_create_sized: (rnn_size %d, embedding_size %d, attention_size %d, output_size %d) outside the device box: rnn_size in "
               "{64,128,192,256}, embedding_size in {64,128}, output_size a multiple of 64 in [64,512], attention_size in [1,256]", R, M, A, O);
    return policy_create(human_num, edge_width, max_envs, R, M, A, O, out);
}

extern "C" int cn_policy_destroy(cn_policy *p)
{
    if (!p) return CN_OK;
    for (int i = 0; i < cn_policy::PROF_RING; ++i) { (void)hipEventDestroy(p->ev[i][0]); (void)hipEventDestroy(p->ev[i][1]); }
    (void)hipEventDestroy(p->ev_fork); (void)hipEventDestroy(p->ev_join); (void)hipStreamDestroy(p->side);
    if (p->blob) CN_HIP(hipFree(p->blob));
    delete p;
    return CN_OK;
}

#define CN_D2D(dst, src, n) CN_HIP(hipMemcpyAsync((dst), (src), (size_t)(n) * sizeof(float), hipMemcpyDeviceToDevice, st))

extern "C" int cn_policy_set_weights(cn_policy *p, const cn_policy_weights *w, void *stream)
{
    CN_REQUIRE(p && w, "cn_policy_set_weights: null argument");
    const float *const *ptrs = reinterpret_cast<const float *const *>(w);
    const size_t attn_first = offsetof(cn_policy_weights, emb2_w) / sizeof(const float *), attn_last = offsetof(cn_policy_weights, out_proj_b) / sizeof(const float *);
    for (size_t i = 0; i < sizeof(cn_policy_weights) / sizeof(const float *); ++i) {
        if (!p->self_attn && i >= attn_first && i <= attn_last) continue; // no human-human attention: those layers do not exist
        CN_REQUIRE(ptrs[i] != nullptr, "cn_policy_set_weights: weight pointer #%zu is null", i);
    }
    hipStream_t st = (hipStream_t)stream;
    const int D = p->D;
    CN_D2D(p->emb0_w, w->emb0_w, 128 * D); CN_D2D(p->emb0_b, w->emb0_b, 128);
    if (!p->self_attn) {
        // use_self_attn = False: out_sp = relu(W2 relu(W0 x + b0) + b2); W2 = spatial_linear.2 [256,128] takes the place of the folded
        // out_proj o spatial_linear image (fp32 + bf16 hi / lo planes)
        CN_D2D(p->os_w, w->spatial_linear_w, 256 * 128); CN_D2D(p->os_b, w->spatial_linear_b, 256);
        const size_t n = 256 * 128;
        hipLaunchKernelGGL(split_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, p->os_w, p->os_hi, p->os_lo);
        CN_CHECK_LAUNCH();
    } else {
    CN_D2D(p->emb2_w, w->emb2_w, 512 * 128); CN_D2D(p->emb2_b, w->emb2_b, 512);
    // fold (q|k|v)_linear into in_proj:  y = W_in (W_x e + b_x) + b_in ; q additionally scaled by 1/sqrt(head_dim) = 0.125
    const float *xw[3] = {w->q_w, w->k_w, w->v_w}, *xb[3] = {w->q_b, w->k_b, w->v_b};
    for (int s = 0; s < 3; ++s) {
        const float scale = s == 0 ? 0.125f : 1.0f;
        hipLaunchKernelGGL(fold_mm_kernel, dim3(2, 512), dim3(256), 0, st, 512, 512, 512, w->in_proj_w + (size_t)s * 512 * 512, xw[s], scale,
                           p->qkv_w + (size_t)s * 512 * 512);
        CN_CHECK_LAUNCH();
        hipLaunchKernelGGL(fold_bias_kernel, dim3(2), dim3(256), 0, st, 512, 512, w->in_proj_w + (size_t)s * 512 * 512, xb[s],
                           w->in_proj_b + s * 512, scale, p->qkv_b + s * 512);
        CN_CHECK_LAUNCH();
    }
    // fold out_proj into spatial_linear: y = W_sl (W_o a + b_o) + b_sl
    hipLaunchKernelGGL(fold_mm_kernel, dim3(2, 256), dim3(256), 0, st, 256, 512, 512, w->spatial_linear_w, w->out_proj_w, 1.0f, p->os_w);
    CN_CHECK_LAUNCH();
    hipLaunchKernelGGL(fold_bias_kernel, dim3(1), dim3(256), 0, st, 256, 512, w->spatial_linear_w, w->out_proj_b, w->spatial_linear_b, 1.0f, p->os_b);
    CN_CHECK_LAUNCH();
    {
        struct { const float *w; __bf16 *hi, *lo; size_t n; } sp[3] = {{p->emb2_w, p->emb2_hi, p->emb2_lo, 512 * 128},
                                                                       {p->qkv_w, p->qkv_hi, p->qkv_lo, 1536 * 512},
                                                                       {p->os_w, p->os_hi, p->os_lo, 256 * 512}};
        for (auto &x : sp) {
            hipLaunchKernelGGL(split_bf16_kernel, dim3((unsigned)((x.n + 255) / 256)), dim3(256), 0, st, x.n, x.w, x.hi, x.lo);
            CN_CHECK_LAUNCH();
        }
    }
    if (int rc = hh_fused_bake(p->emb2_w, p->qkv_w, p->os_w, p->f_emb2, p->f_qkv, p->f_os, st)) return rc;
    } // self_attn
    const int R = p->R, Mb = p->Mb, A = p->A, O = p->O; // cn_policy_dims: 128 / 64 / 64 / 256 by default
    CN_D2D(p->as_w, w->attn_spatial_w, A * 256); CN_D2D(p->as_b, w->attn_spatial_b, A);
    CN_D2D(p->at_w, w->attn_temporal_w, A * 256); CN_D2D(p->at_b, w->attn_temporal_b, A);
    CN_D2D(p->rl_w, w->robot_linear_w, 256 * 9); CN_D2D(p->rl_b, w->robot_linear_b, 256);
    CN_D2D(p->enc_w, w->enc_w, Mb * 256); CN_D2D(p->enc_b, w->enc_b, Mb);
    CN_D2D(p->edge_w, w->edge_embed_w, Mb * 256); CN_D2D(p->edge_b, w->edge_embed_b, Mb);
    CN_D2D(p->wih, w->gru_w_ih, 3 * R * 2 * Mb); CN_D2D(p->whh, w->gru_w_hh, 3 * R * R);
    CN_D2D(p->bih, w->gru_b_ih, 3 * R); CN_D2D(p->bhh, w->gru_b_hh, 3 * R);
    CN_D2D(p->out_w, w->out_w, O * R); CN_D2D(p->out_b, w->out_b, O);
    CN_D2D(p->ac0_w, w->actor0_w, O * O); CN_D2D(p->ac0_w + O * O, w->critic0_w, O * O);
    CN_D2D(p->ac0_b, w->actor0_b, O); CN_D2D(p->ac0_b + O, w->critic0_b, O);
    CN_D2D(p->a2_w, w->actor2_w, O * O); CN_D2D(p->a2_b, w->actor2_b, O);
    CN_D2D(p->c2_w, w->critic2_w, O * O); CN_D2D(p->c2_b, w->critic2_b, O);
    // u = Ws^T (Wt r + bt): the robot-human scores become u . o_j (see hr_attention_kernel); the attention size A is summed away here
    hipLaunchKernelGGL(fold_mm_tn_kernel, dim3(1, 256), dim3(256), 0, st, 256, A, 256, w->attn_spatial_w, w->attn_temporal_w, p->te_w);
    CN_CHECK_LAUNCH();
    hipLaunchKernelGGL(fold_bias_tn_kernel, dim3(1), dim3(256), 0, st, 256, A, w->attn_spatial_w, w->attn_temporal_b, p->te_b);
    CN_CHECK_LAUNCH();
    CN_D2D(p->te_w + 256 * 256, w->enc_w, Mb * 256);
    CN_D2D(p->te_b + 256, w->enc_b, Mb);
    // fold output_linear into the first actor / critic layers: tanh(W0 (Wo h + bo) + b0) = tanh((W0 Wo) h + (W0 bo + b0))
    hipLaunchKernelGGL(fold_mm_kernel, dim3(1, 2 * O), dim3(R), 0, st, 2 * O, O, R, p->ac0_w, w->out_w, 1.0f, p->ac0f_w);
    CN_CHECK_LAUNCH();
    hipLaunchKernelGGL(fold_bias_kernel, dim3((2 * O + 255) / 256), dim3(256), 0, st, 2 * O, O, p->ac0_w, w->out_b, p->ac0_b, 1.0f, p->ac0f_b);
    CN_CHECK_LAUNCH();
    {
        struct { int N, K; const float *w; float *out; } bk[7] = {{256 + Mb, 256, p->te_w, p->r_te}, {3 * R, R, p->whh, p->r_whh}, {Mb, 256, p->edge_w, p->r_edge},
                                                                  {3 * R, 2 * Mb, p->wih, p->r_wih}, {2 * O, R, p->ac0f_w, p->r_ac0}, {O, O, p->a2_w, p->r_a2},
                                                                  {O, O, p->c2_w, p->r_c2}};
        for (auto &b : bk)
            if (int rc = rn_fused_bake(b.N, b.K, b.w, b.out, st)) return rc;
    }
    CN_D2D(p->cl_w, w->critic_linear_w, O); CN_D2D(p->cl_b, w->critic_linear_b, 1);
    CN_D2D(p->fm_w, w->fc_mean_w, 2 * O); CN_D2D(p->fm_b, w->fc_mean_b, 2); CN_D2D(p->logstd, w->logstd, 2);
    p->weights_set = true;
    return CN_OK;
}

// Collect finished (start, stop) pairs.  `all` waits for everything recorded; otherwise only the oldest slot is waited
// for, and only when the ring is full (it finished long ago: the host is at most a few launches ahead of the device).
static int harvest_profile(cn_policy *p, bool all)
{
    constexpr int R = cn_policy::PROF_RING;
    while (p->ev_tail != p->ev_head) {
        const bool full = ((p->ev_head + 1) % R) == p->ev_tail;
        if (!all && !full) break;
        CN_HIP(hipEventSynchronize(p->ev[p->ev_tail][1]));
        float ms = 0.f;
        CN_HIP(hipEventElapsedTime(&ms, p->ev[p->ev_tail][0], p->ev[p->ev_tail][1]));
        p->prof_ms[0] += ms; p->prof_n[0] += 1;
        if (p->prof_samples.size() < (size_t)1 << 20) p->prof_samples.push_back(ms);
        p->ev_tail = (p->ev_tail + 1) % R;
    }
    return CN_OK;
}

// use_self_attn = False (selfAttn_srnn_temp_node.py:342-345, :404-408): out_sp = relu(W2 relu(W0 x + b0) + b2) on the live rows
// (row offsets already built).  Two launches: the D -> 128 layer (embed0_kernel, exact fp32) and the 128 -> 256 layer on the large-GEMM
// kernels in the policy's arithmetic mode (bf16x3 split, or exact fp32 MFMA in mode 0).
static int spatial_mlp_forward(cn_policy *p, int E, const cn_obs *obs, hipStream_t st)
{
    const int H = p->H, D = p->D, M = E * H;
    const int *m_dev = p->row_off + E;
    const int blocks = E < 4096 ? E : 4096;
    hipLaunchKernelGGL(embed0_kernel, dim3(blocks), dim3(128), 0, st, E, H, D, obs->spatial_edges, p->emb0_w, p->emb0_b, p->row_off, p->emb1);
    CN_CHECK_LAUNCH();
    if (p->gemm_mode != 0) return launch_gemm3<128, ACT_RELU>(M, 256, 128, p->emb1, 128, p->os_hi, p->os_lo, p->os_b, p->out_sp, 256, st, m_dev);
    return launch_gemm<128, ACT_RELU>(M, 256, 128, p->emb1, 128, p->os_w, p->os_b, p->out_sp, 256, st, m_dev);
}

static int policy_forward(cn_policy *p, int E, const cn_obs *obs, const float *hxs_in, const float *masks, const float *eps,
                          float *value, float *action, float *logp, float *hxs_out, hipStream_t st)
{
    CN_REQUIRE(p, "policy: null handle");
    if (!p->weights_set) { cn_set_error("policy: call cn_policy_set_weights first"); return CN_ERR_STATE; }
    CN_REQUIRE(E >= 1 && E <= p->maxE, "policy: E=%d outside [1,%d]", E, p->maxE);
    CN_REQUIRE(obs && obs->robot_node && obs->temporal_edges && obs->spatial_edges && obs->detected_human_num, "policy: null observation pointer");
    CN_REQUIRE(hxs_in && masks && value, "policy: null pointer");
    const int H = p->H, D = p->D, M = E * H;
    int rc;
    p->profiling = p->prof_every > 0 && (p->prof_tick++ % p->prof_every) == 0;
    if (p->gemm_mode == 2) {
        // fused mode: two launches -- the human-human kernel (which also builds the row offsets) and the robot-node kernel
        if (p->profiling) { if ((rc = harvest_profile(p, false))) return rc; CN_HIP(hipEventRecord(p->ev[p->ev_head][0], st)); }
        HhFusedWeights fw{p->f_emb2, p->f_qkv, p->f_os, p->emb0_w, p->emb0_b, p->emb2_b, p->qkv_b, p->os_b, 1, 1.0f, nullptr, nullptr, nullptr, nullptr};
        if (!p->self_attn) {
            hipLaunchKernelGGL(row_offsets_kernel, dim3(1), dim3(1024), 0, st, E, H, obs->detected_human_num, p->row_off,
                               p->profiling ? p->live_total : (unsigned long long *)nullptr, p->cls_cnt, p->cls_list);
            CN_CHECK_LAUNCH();
            if ((rc = spatial_mlp_forward(p, E, obs, st))) return rc;
        } else
        if ((rc = hh_fused_forward(E, H, D, obs->spatial_edges, obs->detected_human_num, p->row_off,
                                   p->profiling ? p->live_total : (unsigned long long *)nullptr, fw, p->out_sp, st, obs->row_plan))) return rc;
        if (p->profiling) { CN_HIP(hipEventRecord(p->ev[p->ev_head][1], st)); p->ev_head = (p->ev_head + 1) % cn_policy::PROF_RING; }
        if (p->post_hh_hook) { if ((rc = p->post_hh_hook(p->post_hh_arg, (void *)st))) return rc; }
        RnFusedArgs ra{};
        ra.temporal = obs->temporal_edges; ra.robot_node = obs->robot_node; ra.hxs_in = hxs_in; ra.masks = masks; ra.eps = eps;
        ra.out_sp = p->out_sp; ra.row_off = p->row_off;

        ra.rl_w = p->rl_w; ra.rl_b = p->rl_b; ra.f_te = p->r_te; ra.te_b = p->te_b; ra.f_whh = p->r_whh; ra.bhh = p->bhh;
        ra.f_edge = p->r_edge; ra.edge_b = p->edge_b; ra.f_wih = p->r_wih; ra.bih = p->bih; ra.f_ac0 = p->r_ac0; ra.ac0_b = p->ac0f_b;
        ra.f_a2 = p->r_a2; ra.a2_b = p->a2_b; ra.f_c2 = p->r_c2; ra.c2_b = p->c2_b;
        ra.cl_w = p->cl_w; ra.cl_b = p->cl_b; ra.fm_w = p->fm_w; ra.fm_b = p->fm_b; ra.logstd = p->logstd;
        ra.value = value; ra.action = action; ra.logp = logp; ra.hxs_out = hxs_out ? hxs_out : p->hnew;
        if (p->taps_on) { ra.tap_robot = p->robot_states; ra.tap_attn = p->hr_attn; ra.tap_hr = p->hr_out; ra.tap_actor = p->ac2; }
        if (p->sized) return rn_sized_forward(E, H, ra, RnSizedDims{p->R, p->Mb, p->O, p->rn_te, p->hr_scale}, st);
        return rn_fused_forward(E, H, ra, st);
    }
    // ---- robot node: nothing here depends on the human-human block, so it runs beside it on the side stream ----
    CN_HIP(hipEventRecord(p->ev_fork, st)); // inputs (and the previous forward's readers of z / gh) are ordered before this point
    CN_HIP(hipStreamWaitEvent(p->side, p->ev_fork, 0));
    {
        int blocks = E < 2048 ? E : 2048;
        hipLaunchKernelGGL(robot_embed_kernel, dim3(blocks), dim3(256), 0, p->side, E, obs->temporal_edges, obs->robot_node, p->rl_w, p->rl_b, p->robot_states);
        CN_CHECK_LAUNCH();
    }
    // [u | relu(enc)] in one launch (both read robot_states); z = [u (256) | enc (Mb) | edge (Mb)], GRU input x = z + 256
    const int R = p->R, Mb = p->Mb, O = p->O, ZW = 256 + 2 * Mb; // 128, 64, 256, 384 by default
    if ((rc = launch_gemm_env<ACT_NONE>(E, 256 + Mb, 256, p->robot_states, 256, p->te_w, p->te_b, p->z, ZW, p->side, 1, GemmBatch{0, 0, 0, 0}, 256))) return rc;
    if ((rc = launch_gemm_env<ACT_NONE>(E, 3 * R, R, hxs_in, R, p->whh, nullptr, p->gh, 3 * R, p->side))) return rc; // GRU hidden-side gates
    CN_HIP(hipEventRecord(p->ev_join, p->side));
    // ---- human-human block on the compacted live rows (row_off[E] rows, known only on the device) ----
    const int *m_dev = p->row_off + E;
    // (without the human-human block no launch of this path is bracketed by a profiling event pair: the live rows are not counted either,
    // so that cn_policy_get_profile never reports rows without a matching device time)
    hipLaunchKernelGGL(row_offsets_kernel, dim3(1), dim3(1024), 0, st, E, H, obs->detected_human_num, p->row_off,
                           p->profiling && p->self_attn ? p->live_total : (unsigned long long *)nullptr, p->cls_cnt, p->cls_list);
    CN_CHECK_LAUNCH();
    if (!p->self_attn) {
        if ((rc = spatial_mlp_forward(p, E, obs, st))) return rc;
    } else {
    {
        int blocks = E < 4096 ? E : 4096;
        hipLaunchKernelGGL(embed0_kernel, dim3(blocks), dim3(128), 0, st, E, H, D, obs->spatial_edges, p->emb0_w, p->emb0_b, p->row_off, p->emb1);
        CN_CHECK_LAUNCH();
    }
    const bool split = p->gemm_mode == 1;
    if (split) rc = launch_gemm3<128, ACT_RELU>(M, 512, 128, p->emb1, 128, p->emb2_hi, p->emb2_lo, p->emb2_b, p->emb2, 512, st, m_dev);
    else rc = launch_gemm<128, ACT_RELU>(M, 512, 128, p->emb1, 128, p->emb2_w, p->emb2_b, p->emb2, 512, st, m_dev);
    if (rc) return rc;
    if (p->profiling) { if ((rc = harvest_profile(p, false))) return rc; CN_HIP(hipEventRecord(p->ev[p->ev_head][0], st)); }
    if (split) rc = launch_gemm3<128, ACT_NONE>(M, 1536, 512, p->emb2, 512, p->qkv_hi, p->qkv_lo, p->qkv_b, p->qkv, 1536, st, m_dev);
    else rc = launch_gemm<128, ACT_NONE>(M, 1536, 512, p->emb2, 512, p->qkv_w, p->qkv_b, p->qkv, 1536, st, m_dev);
    if (rc) return rc;
    if (p->profiling) { CN_HIP(hipEventRecord(p->ev[p->ev_head][1], st)); p->ev_head = (p->ev_head + 1) % cn_policy::PROF_RING; }
    {
        if ((rc = launch_hh_attention<8>(E, 0, p->qkv, p->row_off, p->attn, st))) return rc;
        if (H > 8 && (rc = launch_hh_attention<16>(E, 8, p->qkv, p->row_off, p->attn, st))) return rc;
        if (H > 16 && (rc = launch_hh_attention<32>(E, 16, p->qkv, p->row_off, p->attn, st, 1.0f, p->cls_cnt, p->cls_list))) return rc;
        if (H > 32 && (rc = launch_hh_attention<64>(E, 32, p->qkv, p->row_off, p->attn, st, 1.0f, p->cls_cnt + 1, p->cls_list + (size_t)E))) return rc;
    }
    if (split) rc = launch_gemm3<128, ACT_RELU>(M, 256, 512, p->attn, 512, p->os_hi, p->os_lo, p->os_b, p->out_sp, 256, st, m_dev);
    else rc = launch_gemm<128, ACT_RELU>(M, 256, 512, p->attn, 512, p->os_w, p->os_b, p->out_sp, 256, st, m_dev);
    if (rc) return rc;
    }
    // ---- robot-human attention (robot node embeddings arrive from the side stream) ----
    CN_HIP(hipStreamWaitEvent(st, p->ev_join, 0));
    {
        hipLaunchKernelGGL(hr_attention_kernel, dim3((E + 3) / 4), dim3(256), 0, st, E, H, p->hr_scale, p->z, ZW, p->out_sp, p->row_off, p->hr_out, p->hr_attn);
        CN_CHECK_LAUNCH();
    }
    // ---- EndRNN: edge encoder -> GRU (output_linear is folded into the actor / critic trunks) ----
    if ((rc = launch_gemm_env<ACT_RELU>(E, Mb, 256, p->hr_out, 256, p->edge_w, p->edge_b, p->z + 256 + Mb, ZW, st))) return rc;
    if ((rc = launch_gemm_env<ACT_NONE>(E, 3 * R, 2 * Mb, p->z + 256, ZW, p->wih, p->bih, p->gi, 3 * R, st))) return rc;
    float *hdst = hxs_out ? hxs_out : p->hnew;
    hipLaunchKernelGGL(gru_pointwise_kernel, dim3(E), dim3(R), 0, st, E, R, p->gi, p->gh, p->bhh, hxs_in, masks, hdst);
    CN_CHECK_LAUNCH();
    // ---- actor / critic trunks: first layers stacked (+ folded output_linear), second layers as one batched launch ----
    if ((rc = launch_gemm_env<ACT_TANH>(E, 2 * O, R, hdst, R, p->ac0f_w, p->ac0f_b, p->ac1, 2 * O, st))) return rc;
    if ((rc = launch_gemm_env<ACT_TANH>(E, O, O, p->ac1, 2 * O, p->a2_w, p->a2_b, p->ac2, 2 * O, st, 2,
                                        GemmBatch{O, (long long)(p->c2_w - p->a2_w), (long long)(p->c2_b - p->a2_b), O}))) return rc;
    hipLaunchKernelGGL(gauss_head_kernel, dim3((E + 3) / 4), dim3(256), 0, st, E, O, p->ac2, 2 * O, p->cl_w, p->cl_b, p->fm_w, p->fm_b, p->logstd, eps,
                       value, action, logp);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_policy_act(cn_policy *p, int E, const cn_obs *obs, const float *hxs_in, const float *masks, const float *eps,
                             float *value, float *action, float *logp, float *hxs_out, void *stream)
{
    CN_REQUIRE(action && logp && hxs_out, "cn_policy_act: null output pointer");
    CN_REQUIRE(hxs_out != hxs_in, "cn_policy_act: hxs_out must not alias hxs_in");
    return policy_forward(p, E, obs, hxs_in, masks, eps, value, action, logp, hxs_out, (hipStream_t)stream);
}

extern "C" int cn_policy_get_value(cn_policy *p, int E, const cn_obs *obs, const float *hxs_in, const float *masks, float *value, void *stream)
{
    return policy_forward(p, E, obs, hxs_in, masks, nullptr, value, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int cn_policy_get_taps(cn_policy *p, int E, float *spatial_lin, float *hr_attn, float *hr_out, float *robot_emb, float *actor_feat, void *stream)
{
    CN_REQUIRE(p && E >= 1 && E <= p->maxE, "cn_policy_get_taps: bad argument");
    if (p->gemm_mode == 2 && !p->taps_on) { cn_set_error("cn_policy_get_taps: taps are switched off (cn_policy_set_taps)"); return CN_ERR_STATE; }
    hipStream_t st = (hipStream_t)stream;
    const size_t M = (size_t)E * p->H;
    (void)M;
    if (spatial_lin) {
        hipLaunchKernelGGL(scatter_rows_kernel, dim3(E), dim3(256), 0, st, E, p->H, p->out_sp, p->row_off, spatial_lin);
        CN_CHECK_LAUNCH();
    }
    if (hr_attn) CN_D2D(hr_attn, p->hr_attn, M);
    if (hr_out) CN_D2D(hr_out, p->hr_out, (size_t)E * 256);
    if (robot_emb) CN_D2D(robot_emb, p->robot_states, (size_t)E * 256);
    const size_t O = p->O;
    if (actor_feat && p->gemm_mode == 2) CN_D2D(actor_feat, p->ac2, (size_t)E * O); // the fused robot-node kernel taps [E,O] directly
    else if (actor_feat) CN_HIP(hipMemcpy2DAsync(actor_feat, O * sizeof(float), p->ac2, 2 * O * sizeof(float), O * sizeof(float), E, hipMemcpyDeviceToDevice, st));
    return CN_OK;
}

extern "C" int cn_policy_set_gemm_mode(cn_policy *p, int mode)
{
    CN_REQUIRE(p && mode >= 0 && mode <= 2, "cn_policy_set_gemm_mode: mode must be 0 (fp32 MFMA), 1 (bf16x3 split, separate launches) or 2 (bf16x3 split, fused)");
    p->gemm_mode = mode;
    return CN_OK;
}

extern "C" int cn_policy_set_self_attention(cn_policy *p, int enabled)
{
    CN_REQUIRE(p, "cn_policy_set_self_attention: null handle");
    if (p->self_attn != (enabled != 0)) { p->self_attn = enabled != 0; p->weights_set = false; }
    return CN_OK;
}

extern "C" int cn_policy_set_post_hh_hook(cn_policy *p, int (*fn)(void *arg, void *stream), void *arg)
{
    CN_REQUIRE(p, "cn_policy_set_post_hh_hook: null handle");
    p->post_hh_hook = fn; p->post_hh_arg = fn ? arg : nullptr;
    return CN_OK;
}

extern "C" int cn_policy_set_taps(cn_policy *p, int enabled)
{
    CN_REQUIRE(p, "cn_policy_set_taps: null handle");
    p->taps_on = enabled != 0;
    return CN_OK;
}

extern "C" int cn_policy_set_profiling(cn_policy *p, int enabled)
{
    CN_REQUIRE(p && enabled >= 0, "cn_policy_set_profiling: null handle or negative stride");
    p->prof_every = enabled; p->prof_tick = 0; p->profiling = false;
    return CN_OK;
}

extern "C" int cn_policy_get_profile_samples(cn_policy *p, float *ms_out, int cap)
{
    CN_REQUIRE(p && (ms_out || cap == 0) && cap >= 0, "cn_policy_get_profile_samples: null argument");
    if (int rc = harvest_profile(p, true)) return rc;
    const int n = (int)p->prof_samples.size();
    for (int i = 0; i < n && i < cap; ++i) ms_out[i] = p->prof_samples[i];
    return n;
}

extern "C" int cn_policy_reset_profile(cn_policy *p)
{
    CN_REQUIRE(p, "cn_policy_reset_profile: null handle");
    if (int rc = harvest_profile(p, true)) return rc;
    for (int i = 0; i < 8; ++i) { p->prof_ms[i] = 0.0; p->prof_n[i] = 0; }
    p->prof_samples.clear();
    p->prof_tick = 0;
    CN_HIP(hipMemset(p->live_total, 0, 8));
    return CN_OK;
}

extern "C" int cn_policy_get_profile(cn_policy *p, double *ms_out, int64_t *launches_out)
{
    CN_REQUIRE(p && ms_out && launches_out, "cn_policy_get_profile: null argument");
    if (int rc = harvest_profile(p, true)) return rc;
    unsigned long long live = 0;
    CN_HIP(hipMemcpy(&live, p->live_total, 8, hipMemcpyDeviceToHost)); // synchronising: measurement aid only
    p->prof_n[1] = (int64_t)live;                                        // [1] = live (env, human) rows summed over the profiled forwards
    for (int i = 0; i < 8; ++i) { ms_out[i] = p->prof_ms[i]; launches_out[i] = p->prof_n[i]; }
    return CN_OK;
}

// =================================================================================================================================
// Part 2 -- training: stand-alone entry points over whole minibatches (no cn_policy; weights and workspaces come from the caller)
// =================================================================================================================================

// ---- the human-human block of the TRAINING forward as one launch (the rollout's fused kernel + the activations the backward needs) ----
extern "C" int64_t cn_hh_block_workspace_bytes(void) { return (int64_t)(HH_EMB2_FRAG_BYTES + HH_QKV_FRAG_BYTES + HH_OS_FRAG_BYTES); }

extern "C" int cn_hh_block_fwd(int B, int H, int D, const float *spatial_edges, const int *row_off, const float *emb0_w, const float *emb0_b,
                               const float *emb2_w, const float *emb2_b, const float *qkv_w, const float *qkv_b, const float *os_w, const float *os_b,
                               float q_scale, void *workspace, float *e0, float *x, float *qkv, float *attn, float *out_sp, void *stream)
{
    CN_REQUIRE(B >= 1 && H >= 1 && H <= 48 && D >= 1 && D <= 16, "cn_hh_block_fwd: B=%d H=%d D=%d outside B >= 1, 1 <= H <= 48, 1 <= D <= 16", B, H, D);
    CN_REQUIRE(spatial_edges && row_off && emb0_w && emb0_b && emb2_w && emb2_b && qkv_w && qkv_b && os_w && os_b && workspace && e0 && x && qkv && attn && out_sp,
               "cn_hh_block_fwd: null pointer");
    CN_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)emb2_b & 15) == 0 && ((uintptr_t)qkv_b & 15) == 0 && ((uintptr_t)os_b & 15) == 0 &&
               ((uintptr_t)e0 & 15) == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)qkv & 15) == 0 && ((uintptr_t)attn & 15) == 0 && ((uintptr_t)out_sp & 15) == 0,
               "cn_hh_block_fwd: workspace, bias vectors and outputs must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    void *f_emb2 = ws, *f_qkv = ws + HH_EMB2_FRAG_BYTES, *f_os = ws + HH_EMB2_FRAG_BYTES + HH_QKV_FRAG_BYTES;
    if (int rc = hh_fused_bake(emb2_w, qkv_w, os_w, f_emb2, f_qkv, f_os, st)) return rc;
    HhFusedWeights fw{f_emb2, f_qkv, f_os, emb0_w, emb0_b, emb2_b, qkv_b, os_b, 0, q_scale, e0, x, qkv, attn};
    return hh_fused_forward(B, H, D, spatial_edges, nullptr, const_cast<int *>(row_off), nullptr, fw, out_sp, st);
}

// ---- stand-alone attention core (training path: autograd Function in the host mirror) ----
extern "C" int cn_obs_compact_visible(int B, int H, int D, const float *spatial_edges, const uint8_t *visible_masks, float *out_edges, float *out_detected,
                                      void *stream)
{
    if (int rc = cn_require_device()) return rc;
    CN_REQUIRE(B >= 1 && H >= 1 && H <= CN_MAX_HUMANS && D >= 1 && spatial_edges && visible_masks && out_edges && out_detected,
               "cn_obs_compact_visible: bad argument");
    CN_REQUIRE(out_edges != spatial_edges, "cn_obs_compact_visible: out_edges must not alias spatial_edges");
    hipLaunchKernelGGL(compact_visible_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, B, H, D, spatial_edges, visible_masks, out_edges, out_detected);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int64_t cn_hh_attention_workspace_ints(int B) { return B > 0 ? 4 + 4 * (int64_t)B : 0; }

// cls (optional, cn_hh_attention_workspace_ints(B) ints): when given, the size-class lists are built here and each class launch walks
// only its own units; cn_hh_attention_bwd can reuse the same lists (pass the buffer back, unchanged).
extern "C" int cn_hh_attention_fwd(int B, int H, const float *qkv, const int *row_off, float scale, float *out, int *cls, void *stream)
{
    if (int rc = cn_require_device()) return rc;
    CN_REQUIRE(B >= 1 && H >= 1 && H <= CN_MAX_HUMANS && qkv && row_off && out, "cn_hh_attention_fwd: bad argument");
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (cls) {
        CN_HIP(hipMemsetAsync(cls, 0, 4 * sizeof(int), st));
        hipLaunchKernelGGL(hh_classify_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, row_off, cls);
        CN_CHECK_LAUNCH();
    }
    const int *cc = cls, *cl = cls ? cls + 4 : nullptr;
    if ((rc = launch_hh_attention<8>(B, 0, qkv, row_off, out, st, scale, cc, cl))) return rc;
    if (H > 8 && (rc = launch_hh_attention<16>(B, 8, qkv, row_off, out, st, scale, cc ? cc + 1 : nullptr, cl ? cl + (size_t)B : nullptr))) return rc;
    if (H > 16 && (rc = launch_hh_attention<32>(B, 16, qkv, row_off, out, st, scale, cc ? cc + 2 : nullptr, cl ? cl + 2 * (size_t)B : nullptr))) return rc;
    if (H > 32 && (rc = launch_hh_attention<64>(B, 32, qkv, row_off, out, st, scale, cc ? cc + 3 : nullptr, cl ? cl + 3 * (size_t)B : nullptr))) return rc;
    return CN_OK;
}

extern "C" int cn_hr_attention_fwd(int B, int H, const float *u, const float *out_sp, const int *row_off, float *hr_out, float *attn, void *stream)
{
    if (int rc = cn_require_device()) return rc;
    CN_REQUIRE(B >= 1 && H >= 1 && H <= CN_MAX_HUMANS && u && out_sp && row_off && hr_out && attn, "cn_hr_attention_fwd: bad argument");
    hipLaunchKernelGGL(hr_attention_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, B, H, (float)H / 8.0f, u, 256, out_sp, row_off, hr_out, attn);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_hr_attention_bwd(int B, int H, const float *u, const float *out_sp, const int *row_off, const float *attn, const float *d_hr,
                                   float *d_u, float *d_o, void *stream)
{
    if (int rc = cn_require_device()) return rc;
    CN_REQUIRE(B >= 1 && H >= 1 && H <= CN_MAX_HUMANS && u && out_sp && row_off && attn && d_hr && d_u && d_o, "cn_hr_attention_bwd: bad argument");
    hipLaunchKernelGGL(hr_attention_bwd_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, B, H, u, out_sp, row_off, attn, d_hr, d_u, d_o, 256, 256, (float)H / 8.0f);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_hh_attention_bwd(int B, int H, const float *qkv, const int *row_off, const float *d_out, float scale, float *d_qkv, int *cls,
                                   int cls_ready, void *stream)
{
    if (int rc = cn_require_device()) return rc;
    CN_REQUIRE(B >= 1 && H >= 1 && H <= CN_MAX_HUMANS && qkv && row_off && d_out && d_qkv && cls, "cn_hh_attention_bwd: bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (!cls_ready) { // lists not built by a preceding cn_hh_attention_fwd on the same row_off
        CN_HIP(hipMemsetAsync(cls, 0, 4 * sizeof(int), st));
        hipLaunchKernelGGL(hh_classify_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, row_off, cls);
        CN_CHECK_LAUNCH();
    }
    int rc;
    if ((rc = launch_hh_attention_bwd<8>(B, qkv, row_off, cls, 0, d_out, d_qkv, scale, st))) return rc;
    if (H > 8 && (rc = launch_hh_attention_bwd<16>(B, qkv, row_off, cls, 1, d_out, d_qkv, scale, st))) return rc;
    if (H > 16 && (rc = launch_hh_attention_bwd<32>(B, qkv, row_off, cls, 2, d_out, d_qkv, scale, st))) return rc;
    if (H > 32 && (rc = launch_hh_attention_bwd<64>(B, qkv, row_off, cls, 3, d_out, d_qkv, scale, st))) return rc;
    return CN_OK;
}


// ---------------------------------------------------------------------------------------------------------------------------------
// cn_rn_seq_fwd / cn_rn_seq_bwd: the robot-node sequence of evaluate_actions (see include/crowdnav_hip.h).  A sequence of the kernels of
// the separate-launch rollout forward run over all B = T * N samples at once (every layer but the GRU is independent across samples), the
// GRU as ONE launch per direction (cn_gru_seq_*), and their backward counterparts: products on the split-precision NT kernel of the big
// layers (activation or activation derivative in the epilogue), weight gradients on the split-K TN kernel (cn_linear_wgrad), small
// reductions in fixed order.
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {
// The sizes of the sequence: cn_policy_dims checked against the device box (the default when dims == NULL).
struct RnDims {
    int R, M, A, O; // rnn_size, embedding_size, attention_size, output_size
    int ZW;         // row of saved z: u (256) | relu(enc) (M) | relu(edge) (M)
    int TE;         // rows of te_w: 256 + M
    bool ok;
};
constexpr int rn_pad128(int n) { return (n + 127) & ~127; }
RnDims rn_dims(const cn_policy_dims *d)
{
    RnDims q{128, 64, 64, 256, 0, 0, true};
    if (d) { q.R = d->rnn_size; q.M = d->embedding_size; q.A = d->attention_size; q.O = d->output_size; }
    q.ok = (q.R == 64 || q.R == 128 || q.R == 192 || q.R == 256) && (q.M == 64 || q.M == 128) && q.O >= 64 && q.O <= 512 && q.O % 64 == 0 && q.A >= 1 && q.A <= 256;
    q.ZW = 256 + 2 * q.M; q.TE = 256 + q.M;
    return q;
}
#define RN_REQUIRE_BOX(D, WHO)                                                                                                                      \
    CN_REQUIRE((D).ok, WHO ": (rnn_size %d, embedding_size %d, attention_size %d, output_size %d) outside the device box: rnn_size in {64, 128, 192, " \
               "256}, embedding_size in {64, 128}, output_size a multiple of 64 in [64, 512], attention_size in [1, 256]", (D).R, (D).M, (D).A, (D).O)

struct RnWs { // carve-up of the backward workspace (floats)
    size_t d2, d1, dhs, dgi, dgh, dz, dhr, drs, a2T, c2T, ac0T, wihT, edgeT, teT, part, dbp, small, gru, total;
    int small_rows;
};
RnWs rn_ws(int T, int N, const RnDims &D)
{
    const size_t B = (size_t)T * N;
    const int R = D.R, M = D.M, O = D.O;
    RnWs w{};
    size_t off = 0;
    auto carve = [&](size_t n) { size_t o = off; off += (n + 63) & ~size_t(63); return o; };
    w.d2 = carve(B * 2 * O); w.d1 = carve(B * 2 * O); w.dhs = carve(B * R); w.dgi = carve(B * 3 * R); w.dgh = carve(B * 3 * R); w.dz = carve(B * D.ZW);
    w.dhr = carve(B * 256); w.drs = carve(B * 256);
    // transposed planes of the dX products; a product with N % 128 != 0 output columns gets planes zero-padded to the next multiple of 128
    w.a2T = carve((size_t)rn_pad128(O) * O); w.c2T = carve((size_t)rn_pad128(O) * O); w.ac0T = carve((size_t)rn_pad128(R) * 2 * O);
    w.wihT = carve((size_t)2 * M * 3 * R); w.edgeT = carve((size_t)256 * M); w.teT = carve((size_t)256 * D.TE);
    // weight-gradient partials: the largest of the seven products (splits <= 66 by construction of cn_linear_wgrad_splits)
    size_t pmax = 0, bmax = 0;
    const int shp[7][2] = {{O, O}, {O, O}, {2 * O, R}, {3 * R, R}, {3 * R, 2 * M}, {M, 256}, {D.TE, 256}};
    for (auto &q : shp) {
        const size_t sp = (size_t)cn_linear_wgrad_splits((int)B, q[0], q[1]);
        pmax = pmax > sp * q[0] * q[1] ? pmax : sp * q[0] * q[1];
        bmax = bmax > sp * q[0] ? bmax : sp * q[0];
    }
    if (bmax < (size_t)rn_head_cols(O)) bmax = rn_head_cols(O); // dbp also receives the reduced head gradients (cn_rn_seq_bwd): with one split per product
                                                                // (a few samples) 512 floats would let them run into `small`, which that reduction is reading
    w.part = carve(pmax); w.dbp = carve(bmax);
    w.small_rows = 1024;
    w.small = carve((size_t)w.small_rows * 2560); // head partials [1024, 3 O + 8 <= 1544] / robot_linear partials [1024, 256, 10]
    w.gru = carve(R <= 128 ? 0 : (size_t)3 * R * R); // fragment image of W_hh for cn_gru_seq_bwd_sized (R = 64 / 128 keep the weights in registers)
    w.total = off;
    return w;
}
int rn_wgrad(int M, int N, int K, const float *dY, int ldy, const float *X, int ldx, float *ws, const RnWs &L, float *dW, float *db, hipStream_t st)
{
    const int splits = cn_linear_wgrad_splits(M, N, K);
    CN_REQUIRE(splits >= 1, "cn_rn_seq_bwd: no split-K plan for a %d x %d weight gradient over %d rows", N, K, M);
    return cn_linear_wgrad(M, N, K, dY, ldy, nullptr, X, ldx, splits, ws + L.part, ws + L.dbp, dW, db, (void *)st);
}
template <int ACT>
int rn_gemm(int M, int N, int K, const float *A, int lda, const float *W, const float *bias, float *C, int ldc, hipStream_t st)
{
    return launch_gemm_t<64, 64, ACT>(M, N, K, A, lda, W, bias, C, ldc, st, nullptr, 1, GemmBatch{0, 0, 0, 0}, 1 << 30);
}
// The products with K % 64 == 0 -- all but edge_attention_embed's forward -- run on the split-precision kernel of the update's big layers
// (cn_linear_fwd_act, gemm3p.h): three bf16 MFMA products per term at ~5x the rate of the exact-fp32 instruction.  `planes` = hi plane followed by
// lo plane (Np * K bf16 each = the Np * K floats of the slot) in that kernel's fragment order, Np = N rounded up to a multiple of 128 with zero rows
// behind the real ones: the kernel computes Np columns and stores the N real ones (a guarded store: no output or bias has padded columns).
int rn_gemm3(int act, int M, int N, int K, const float *A, int lda, const float *planes, const float *bias, float *C, int ldc, hipStream_t st,
             const float *aux = nullptr, int ldaux = 0, int relu_from = 1 << 30)
{
    const int Np = rn_pad128(N);
    return cn_linear_fwd_act_cols(M, Np, N, K, A, lda, planes, reinterpret_cast<const uint16_t *>(planes) + (size_t)Np * K, bias, act, aux, ldaux, relu_from, C,
                                  ldc, (void *)st);
}
struct RnFwdWs { size_t te, teb, wih, ac0, a2, c2, gru, total; }; // forward workspace (floats): split planes of the five weights + the padded te bias
RnFwdWs rn_fwd_ws(const RnDims &D)
{
    const int R = D.R, M = D.M, O = D.O;
    RnFwdWs w{};
    size_t off = 0;
    auto carve = [&](size_t n) { size_t o = off; off += (n + 63) & ~size_t(63); return o; };
    w.te = carve((size_t)rn_pad128(D.TE) * 256); w.teb = carve(rn_pad128(D.TE)); w.wih = carve((size_t)rn_pad128(3 * R) * 2 * M); w.ac0 = carve((size_t)2 * O * R);
    w.a2 = carve((size_t)rn_pad128(O) * O); w.c2 = carve((size_t)rn_pad128(O) * O);
    w.gru = carve(R <= 128 ? 0 : (size_t)3 * R * R); // fragment image of W_hh for cn_gru_seq_fwd_sized (streamed R only)
    w.total = off;
    return w;
}
} // namespace

extern "C" int64_t cn_rn_seq_workspace_floats_sized(int T, int N, const cn_policy_dims *dims)
{
    const RnDims D = rn_dims(dims);
    return (T > 0 && N > 0 && D.ok) ? (int64_t)rn_ws(T, N, D).total : 0;
}
extern "C" int64_t cn_rn_seq_fwd_workspace_floats_sized(const cn_policy_dims *dims)
{
    const RnDims D = rn_dims(dims);
    return D.ok ? (int64_t)rn_fwd_ws(D).total : 0;
}
extern "C" int64_t cn_rn_seq_workspace_floats(int T, int N) { return cn_rn_seq_workspace_floats_sized(T, N, nullptr); }
extern "C" int64_t cn_rn_seq_fwd_workspace_floats(void) { return cn_rn_seq_fwd_workspace_floats_sized(nullptr); }

static int rn_check(int T, int N, int H, const void *a, const void *b, const void *c, const void *d, const cn_rn_weights *w, const cn_rn_saved *sv)
{
    CN_REQUIRE(T >= 1 && N >= 1 && H >= 1 && H <= CN_MAX_HUMANS, "cn_rn_seq: bad shape T=%d N=%d H=%d", T, N, H);
    CN_REQUIRE(a && b && c && d && w && sv, "cn_rn_seq: null argument");
    const void *const *wp = reinterpret_cast<const void *const *>(w);
    for (size_t i = 0; i < sizeof(cn_rn_weights) / sizeof(void *); ++i) CN_REQUIRE(wp[i], "cn_rn_seq: weight pointer #%zu is null", i);
    const void *const *sp = reinterpret_cast<const void *const *>(sv);
    for (size_t i = 0; i < sizeof(cn_rn_saved) / sizeof(void *); ++i) CN_REQUIRE(sp[i], "cn_rn_seq: saved-activation pointer #%zu is null", i);
    return CN_OK;
}

// The weight preparation of one optimiser step's sequence as jobs of ONE grouped launch (cn_split_group_launch): forward planes (rows padded to
// whole 128-column tiles, e.g. te: 320 rows -> 384; its bias padded with zeros) and the transposed planes of the backward's dX products.
int rn_seq_prep_jobs(const cn_rn_weights *w, float *fwd_ws, float *bwd_ws, int T, int N, CnSplitJob *out, const cn_policy_dims *dims)
{
    const RnDims D = rn_dims(dims);
    const int R = D.R, M = D.M, O = D.O;
    auto padded = [](int n) { return n % 128 ? rn_pad128(n) : 0; };
    int n = 0;
    if (fwd_ws) {
        const RnFwdWs F = rn_fwd_ws(D);
        out[n++] = cn_split_job(w->te_w, D.TE, 256, 0, padded(D.TE), fwd_ws + F.te);
        out[n++] = cn_split_job(w->wih, 3 * R, 2 * M, 0, padded(3 * R), fwd_ws + F.wih);
        out[n++] = cn_split_job(w->ac0_w, 2 * O, R, 0, 0, fwd_ws + F.ac0);
        out[n++] = cn_split_job(w->a2_w, O, O, 0, padded(O), fwd_ws + F.a2);
        out[n++] = cn_split_job(w->c2_w, O, O, 0, padded(O), fwd_ws + F.c2);
        out[n++] = CnSplitJob{w->te_b, fwd_ws + F.teb, nullptr, rn_pad128(D.TE), 0, 0, D.TE, 0};
    }
    if (bwd_ws) {
        const RnWs L = rn_ws(T, N, D);
        out[n++] = cn_split_job(w->a2_w, O, O, 1, padded(O), bwd_ws + L.a2T);
        out[n++] = cn_split_job(w->c2_w, O, O, 1, padded(O), bwd_ws + L.c2T);
        out[n++] = cn_split_job(w->ac0_w, 2 * O, R, 1, padded(R), bwd_ws + L.ac0T);
        out[n++] = cn_split_job(w->wih, 3 * R, 2 * M, 1, 0, bwd_ws + L.wihT);
        out[n++] = cn_split_job(w->edge_w, M, 256, 1, 0, bwd_ws + L.edgeT);
        out[n++] = cn_split_job(w->te_w, D.TE, 256, 1, 0, bwd_ws + L.teT);
    }
    return n;
}

extern "C" int cn_rn_seq_fwd(int T, int N, int H, const float *robot_node, const float *temporal, const float *out_sp, const int *row_off, const float *h0,
                             const float *masks, const float *actions, const cn_rn_weights *w, const cn_rn_saved *sv, float *ws, float *value, float *logp,
                             void *stream)
{
    return rn_seq_fwd_impl(T, N, H, robot_node, temporal, out_sp, row_off, h0, masks, actions, w, sv, ws, value, logp, stream, false, nullptr);
}

extern "C" int cn_rn_seq_fwd_sized(int T, int N, int H, const float *robot_node, const float *temporal, const float *out_sp, const int *row_off,
                                   const float *h0, const float *masks, const float *actions, const cn_rn_weights *w, const cn_rn_saved *sv, float *ws,
                                   float *value, float *logp, const cn_policy_dims *dims, void *stream)
{
    return rn_seq_fwd_impl(T, N, H, robot_node, temporal, out_sp, row_off, h0, masks, actions, w, sv, ws, value, logp, stream, false, dims);
}

int rn_seq_fwd_impl(int T, int N, int H, const float *robot_node, const float *temporal, const float *out_sp, const int *row_off, const float *h0,
                    const float *masks, const float *actions, const cn_rn_weights *w, const cn_rn_saved *sv, float *ws, float *value, float *logp,
                    void *stream, bool prepared, const cn_policy_dims *dims)
{
    const RnDims D = rn_dims(dims);
    RN_REQUIRE_BOX(D, "cn_rn_seq_fwd");
    if (int rc = cn_require_device()) return rc;
    if (int rc = rn_check(T, N, H, robot_node, temporal, out_sp, row_off, w, sv)) return rc;
    CN_REQUIRE(h0 && masks && actions && ws && value && logp, "cn_rn_seq_fwd: null argument");
    hipStream_t st = (hipStream_t)stream;
    const int B = T * N, R = D.R, M = D.M, O = D.O, ZW = D.ZW;
    const RnFwdWs F = rn_fwd_ws(D);
    // the temperature num_edges / sqrt(attention_size) of the robot-human scores, as the rollout kernels form it (H / 8 at attention_size = 64)
    const float temp = (float)((double)H / sqrt((double)D.A));
    int rc;
    if (!prepared) { // split planes of this optimiser step's weights, one grouped launch
        CnSplitJob jobs[8];
        const int nj = rn_seq_prep_jobs(w, ws, nullptr, T, N, jobs, dims);
        if ((rc = cn_split_group_launch(jobs, nj, st))) return rc;
    }
    hipLaunchKernelGGL(robot_embed_kernel, dim3(B < 2048 ? B : 2048), dim3(256), 0, st, B, temporal, robot_node, w->rl_w, w->rl_b, sv->rs);
    CN_CHECK_LAUNCH();
    // z = [u (256) | relu(enc) (M) | .] in one product (both read robot_states), then the attention over the compacted rows, then edge -> z[256+M:]
    if ((rc = rn_gemm3(ACT_NONE, B, D.TE, 256, sv->rs, 256, ws + F.te, ws + F.teb, sv->z, ZW, st, nullptr, 0, 256))) return rc;
    hipLaunchKernelGGL(hr_attention_kernel, dim3((B + 3) / 4), dim3(256), 0, st, B, H, temp, sv->z, ZW, out_sp, row_off, sv->hr, sv->attn);
    CN_CHECK_LAUNCH();
    if ((rc = rn_gemm<ACT_RELU>(B, M, 256, sv->hr, 256, w->edge_w, w->edge_b, sv->z + D.TE, ZW, st))) return rc;
    if ((rc = rn_gemm3(ACT_NONE, B, 3 * R, 2 * M, sv->z + 256, ZW, ws + F.wih, w->bih, sv->gi, 3 * R, st))) return rc;
    if ((rc = cn_gru_seq_fwd_sized(T, N, R, sv->gi, h0, masks, w->whh, w->bhh, sv->hs, sv->hms, sv->gates, ws + F.gru, stream))) return rc;
    if ((rc = rn_gemm3(ACT_TANH, B, 2 * O, R, sv->hs, R, ws + F.ac0, w->ac0_b, sv->a1, 2 * O, st))) return rc;
    if ((rc = rn_gemm3(ACT_TANH, B, O, O, sv->a1, 2 * O, ws + F.a2, w->a2_b, sv->a2, 2 * O, st))) return rc;
    if ((rc = rn_gemm3(ACT_TANH, B, O, O, sv->a1 + O, 2 * O, ws + F.c2, w->c2_b, sv->a2 + O, 2 * O, st))) return rc;
    RN_HEAD_DISPATCH(O / 64, hipLaunchKernelGGL(rn_head_fwd_kernel<NS>, dim3((B + 3) / 4), dim3(256), 0, st, B, sv->a2, w->cl_w, w->cl_b, w->fm_w, w->fm_b,
                                                w->logstd, actions, value, logp));
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_rn_seq_bwd(int T, int N, int H, const float *robot_node, const float *temporal, const float *out_sp, const int *row_off, const float *masks,
                             const float *actions, const cn_rn_weights *w, const cn_rn_saved *sv, const float *d_value, const float *d_logp, float *ws,
                             float *d_out_sp, float *d_h0, const cn_rn_grads *g, void *stream)
{
    return rn_seq_bwd_impl(T, N, H, robot_node, temporal, out_sp, row_off, masks, actions, w, sv, d_value, d_logp, ws, d_out_sp, d_h0, g, stream, false, nullptr,
                           nullptr);
}

extern "C" int cn_rn_seq_bwd_sized(int T, int N, int H, const float *robot_node, const float *temporal, const float *out_sp, const int *row_off,
                                   const float *masks, const float *actions, const cn_rn_weights *w, const cn_rn_saved *sv, const float *d_value,
                                   const float *d_logp, float *ws, float *d_out_sp, float *d_h0, const cn_rn_grads *g, const cn_policy_dims *dims, void *stream)
{
    return rn_seq_bwd_impl(T, N, H, robot_node, temporal, out_sp, row_off, masks, actions, w, sv, d_value, d_logp, ws, d_out_sp, d_h0, g, stream, false, nullptr,
                           dims);
}

int rn_seq_bwd_impl(int T, int N, int H, const float *robot_node, const float *temporal, const float *out_sp, const int *row_off, const float *masks,
                    const float *actions, const cn_rn_weights *w, const cn_rn_saved *sv, const float *d_value, const float *d_logp, float *ws,
                    float *d_out_sp, float *d_h0, const cn_rn_grads *g, void *stream, bool prepared, float **packed_heads, const cn_policy_dims *dims)
{
    const RnDims D = rn_dims(dims);
    RN_REQUIRE_BOX(D, "cn_rn_seq_bwd");
    if (int rc = cn_require_device()) return rc;
    if (int rc = rn_check(T, N, H, robot_node, temporal, out_sp, row_off, w, sv)) return rc;
    CN_REQUIRE(masks && actions && d_value && d_logp && ws && d_out_sp && d_h0 && g, "cn_rn_seq_bwd: null argument");
    {
        const void *const *gp = reinterpret_cast<const void *const *>(g);
        for (size_t i = 0; i < sizeof(cn_rn_grads) / sizeof(void *); ++i) CN_REQUIRE(gp[i], "cn_rn_seq_bwd: gradient pointer #%zu is null", i);
    }
    hipStream_t st = (hipStream_t)stream;
    const int B = T * N, R = D.R, M = D.M, O = D.O, ZW = D.ZW, HC = rn_head_cols(O);
    const float temp = (float)((double)H / sqrt((double)D.A));
    const RnWs L = rn_ws(T, N, D);
    float *d2 = ws + L.d2, *d1 = ws + L.d1, *dhs = ws + L.dhs, *dgi = ws + L.dgi, *dgh = ws + L.dgh, *dz = ws + L.dz, *dhr = ws + L.dhr, *drs = ws + L.drs;
    int rc;
    // ---- heads + the tanh of the second trunk layers; the heads' own weight gradients ----
    {
        const int blocks = B < 4 * L.small_rows ? (B + 3) / 4 : L.small_rows;
        RN_HEAD_DISPATCH(O / 64, hipLaunchKernelGGL(rn_head_bwd_kernel<NS>, dim3(blocks), dim3(256), 0, st, B, sv->a2, w->cl_w, w->fm_w, w->fm_b, w->logstd, actions,
                                                    d_value, d_logp, d2, ws + L.small));
        CN_CHECK_LAUNCH();
        // the reduced head gradients: 3 O + 8 floats in the bias-partial region (free until the first weight gradient below) -- or, for a
        // caller that scatters them itself (packed_heads), at the end of the head partials' region, which nothing writes before robot_linear's
        // partials at the very end of this call
        float *red = packed_heads ? ws + L.small + (size_t)(L.small_rows - 1) * 2560 + (HC <= 1536 ? 1024 : 2560 - HC) : ws + L.dbp;
        hipLaunchKernelGGL(rn_reduce_rows_kernel, dim3((HC + 15) / 16), dim3(256), 0, st, blocks, HC, ws + L.small, red, nullptr, 0);
        CN_CHECK_LAUNCH();
        if (packed_heads) *packed_heads = red;
        else {
            CN_HIP(hipMemcpyAsync(g->fm_w, red, 2 * O * sizeof(float), hipMemcpyDeviceToDevice, st));
            CN_HIP(hipMemcpyAsync(g->cl_w, red + 2 * O, O * sizeof(float), hipMemcpyDeviceToDevice, st));
            CN_HIP(hipMemcpyAsync(g->fm_b, red + 3 * O, 2 * sizeof(float), hipMemcpyDeviceToDevice, st));
            CN_HIP(hipMemcpyAsync(g->cl_b, red + 3 * O + 2, 1 * sizeof(float), hipMemcpyDeviceToDevice, st));
            CN_HIP(hipMemcpyAsync(g->logstd, red + 3 * O + 3, 2 * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
    }
    // ---- split planes of the transposed weights for the dX products (dX = dY W as an NT product with W^T), one grouped launch ----
    if (!prepared) {
        CnSplitJob jobs[8];
        const int nj = rn_seq_prep_jobs(w, nullptr, ws, T, N, jobs, dims);
        if ((rc = cn_split_group_launch(jobs, nj, st))) return rc;
    }
    // ---- second trunk layers: weight gradients, then d1 = (d2 W2) (1 - a1^2) ----
    if ((rc = rn_wgrad(B, O, O, d2, 2 * O, sv->a1, 2 * O, ws, L, g->a2_w, g->a2_b, st))) return rc;
    if ((rc = rn_wgrad(B, O, O, d2 + O, 2 * O, sv->a1 + O, 2 * O, ws, L, g->c2_w, g->c2_b, st))) return rc;
    if ((rc = rn_gemm3(ACT_MUL_DTANH, B, O, O, d2, 2 * O, ws + L.a2T, nullptr, d1, 2 * O, st, sv->a1, 2 * O))) return rc;
    if ((rc = rn_gemm3(ACT_MUL_DTANH, B, O, O, d2 + O, 2 * O, ws + L.c2T, nullptr, d1 + O, 2 * O, st, sv->a1 + O, 2 * O))) return rc;
    // ---- first trunk layers (output_linear folded in) ----
    if ((rc = rn_wgrad(B, 2 * O, R, d1, 2 * O, sv->hs, R, ws, L, g->ac0_w, g->ac0_b, st))) return rc;
    if ((rc = rn_gemm3(ACT_NONE, B, R, 2 * O, d1, 2 * O, ws + L.ac0T, nullptr, dhs, R, st))) return rc;
    // ---- GRU over the sequence ----
    if ((rc = cn_gru_seq_bwd_sized(T, N, R, sv->gates, sv->hms, masks, w->whh, dhs, dgi, dgh, d_h0, ws + L.gru, stream))) return rc;
    if ((rc = rn_wgrad(B, 3 * R, R, dgh, 3 * R, sv->hms, R, ws, L, g->whh, g->bhh, st))) return rc;
    if ((rc = rn_wgrad(B, 3 * R, 2 * M, dgi, 3 * R, sv->z + 256, ZW, ws, L, g->wih, g->bih, st))) return rc;
    // ---- d[enc | edge] = (dgi W_ih) relu'(.) -> dz[:, 256:]; d hr = d edge W_e; attention backward; d u -> dz[:, 0:256] ----
    if ((rc = rn_gemm3(ACT_MUL_DRELU, B, 2 * M, 3 * R, dgi, 3 * R, ws + L.wihT, nullptr, dz + 256, ZW, st, sv->z + 256, ZW))) return rc;
    if ((rc = rn_wgrad(B, M, 256, dz + D.TE, ZW, sv->hr, 256, ws, L, g->edge_w, g->edge_b, st))) return rc;
    if ((rc = rn_gemm3(ACT_NONE, B, 256, M, dz + D.TE, ZW, ws + L.edgeT, nullptr, dhr, 256, st))) return rc;
    hipLaunchKernelGGL(hr_attention_bwd_kernel, dim3((B + 3) / 4), dim3(256), 0, st, B, H, sv->z, out_sp, row_off, sv->attn, dhr, dz, d_out_sp, ZW, ZW, temp);
    CN_CHECK_LAUNCH();
    // ---- [u | enc] layer and robot_linear ----
    if ((rc = rn_wgrad(B, D.TE, 256, dz, ZW, sv->rs, 256, ws, L, g->te_w, g->te_b, st))) return rc;
    if ((rc = rn_gemm3(ACT_MUL_DRELU, B, 256, D.TE, dz, ZW, ws + L.teT, nullptr, drs, 256, st, sv->rs, 256))) return rc;
    {
        const int blocks = B < 512 ? B : 512;
        hipLaunchKernelGGL(rn_rl_wgrad_kernel, dim3(blocks), dim3(256), 0, st, B, drs, temporal, robot_node, ws + L.small);
        CN_CHECK_LAUNCH();
        hipLaunchKernelGGL(rn_reduce_rows_kernel, dim3(2560 / 16), dim3(256), 0, st, blocks, 2560, ws + L.small, g->rl_w, g->rl_b, 1);
        CN_CHECK_LAUNCH();
    }
    return CN_OK;
}
