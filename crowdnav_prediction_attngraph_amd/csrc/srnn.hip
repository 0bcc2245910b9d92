// srnn.hip -- the cn_srnn handle: rollout-time forward of the DS-RNN baseline (Policy(base='srnn'), rl/networks/srnn_model.py) as TWO launches,
// whatever E and H: srnn_edge_gru_kernel (both edge GRUs) and srnn_node_kernel (attention, node GRU, trunks, heads, sampling).  No framework
// kernel between the observation and the outputs, no atomics on data, the same arguments give the same bits.
#include <new>

#include "srnn_kernels.h"

namespace {
constexpr size_t sr_align(size_t x) { return (x + 255) & ~size_t(255); }
} // namespace

namespace {

// number of floats of each cn_srnn_weights field, in field order
void srnn_counts(int D, size_t *n)
{
    const size_t c[SR_NW] = {
        (size_t)64 * D, 64, 768 * 64, 768 * 256, 768, 768,      // spatial edge RNN: encoder, GRU
        64 * 2, 64, 768 * 64, 768 * 256, 768, 768,              // temporal edge RNN
        64 * 256, 64, 64 * 256, 64,                             // attention
        64 * 3, 64, 64 * 512, 64, 384 * 128, 384 * 128, 384, 384, 256 * 128, 256,   // node RNN
        256 * 256, 256, 256 * 256, 256, 256 * 256, 256, 256 * 256, 256,             // actor, critic
        256, 1, 3 * 7, 3, 2 * 256, 2, 2};                       // critic_linear, robot_linear, fc_mean, logstd
    for (int i = 0; i < SR_NW; ++i) n[i] = c[i];
}

int srnn_forward(cn_srnn *p, int E, const cn_obs *obs, const float *node_in, const float *edge_in, const float *masks, const float *eps, float *value,
                 float *action, float *logp, float *node_out, float *edge_out, hipStream_t st)
{
    const int H = p->H;
    const SrnnEdgeW ws = srnn_edge_weights(p, 1), wt = srnn_edge_weights(p, 0);
    const int tiles_t = (E + SR_TILE - 1) / SR_TILE;
    const long long tiles_s = ((long long)E * H + SR_TILE - 1) / SR_TILE;
    CN_REQUIRE(tiles_t + tiles_s < (1ll << 31), "cn_srnn: too many edge rows");
    const dim3 grid((unsigned)(tiles_t + tiles_s));
    if (int rc = cn_lds_opt_in<&srnn_edge_gru_kernel<1>>((int)SR_EDGE_LDS)) return rc;
    if (int rc = cn_lds_opt_in<&srnn_edge_gru_kernel<0>>((int)SR_EDGE_LDS)) return rc;
    if (p->mode)
        hipLaunchKernelGGL(srnn_edge_gru_kernel<1>, grid, dim3(SR_EDGE_THREADS), SR_EDGE_LDS, st, E, H, tiles_t, wt, ws, obs->temporal_edges, obs->spatial_edges,
                           edge_in, masks, edge_out);
    else
        hipLaunchKernelGGL(srnn_edge_gru_kernel<0>, grid, dim3(SR_EDGE_THREADS), SR_EDGE_LDS, st, E, H, tiles_t, wt, ws, obs->temporal_edges, obs->spatial_edges,
                           edge_in, masks, edge_out);
    CN_CHECK_LAUNCH();
    SrnnNodeW nw;
    nw.at_w = p->w[W_ATTN]; nw.at_b = p->w[W_ATTN + 1]; nw.as_w = p->w[W_ATTN + 2]; nw.as_b = p->w[W_ATTN + 3];
    nw.enc_w = p->w[W_NODE]; nw.enc_b = p->w[W_NODE + 1]; nw.eae_w = p->w[W_NODE + 2]; nw.eae_b = p->w[W_NODE + 3];
    nw.w_ih = p->w[W_NODE + 4]; nw.w_hh = p->w[W_NODE + 5]; nw.b_ih = p->w[W_NODE + 6]; nw.b_hh = p->w[W_NODE + 7];
    nw.out_w = p->w[W_NODE + 8]; nw.out_b = p->w[W_NODE + 9];
    nw.a0_w = p->w[W_TRUNK]; nw.a0_b = p->w[W_TRUNK + 1]; nw.a2_w = p->w[W_TRUNK + 2]; nw.a2_b = p->w[W_TRUNK + 3];
    nw.c0_w = p->w[W_TRUNK + 4]; nw.c0_b = p->w[W_TRUNK + 5]; nw.c2_w = p->w[W_TRUNK + 6]; nw.c2_b = p->w[W_TRUNK + 7];
    nw.cl_w = p->w[W_HEADS]; nw.cl_b = p->w[W_HEADS + 1]; nw.rl_w = p->w[W_HEADS + 2]; nw.rl_b = p->w[W_HEADS + 3];
    nw.fm_w = p->w[W_HEADS + 4]; nw.fm_b = p->w[W_HEADS + 5]; nw.logstd = p->w[W_HEADS + 6];
    SrnnNodeIO io;
    io.robot_node = obs->robot_node; io.edge = edge_out; io.node_in = node_in; io.masks = masks; io.eps = eps;
    io.value = value; io.action = action; io.logp = logp; io.node_out = node_out;
    io.tap_attn = p->tap_attn; io.tap_weighted = p->tap_weighted; io.tap_node = p->tap_node; io.tap_feat = p->tap_feat;
    hipLaunchKernelGGL(srnn_node_kernel, dim3((E + SR_G - 1) / SR_G), dim3(SR_NODE_THREADS), 0, st, E, H, nw, io);
    CN_CHECK_LAUNCH();
    p->last_edge = edge_out;
    p->lastE = E;
    return CN_OK;
}

int srnn_check_call(cn_srnn *p, int E, const cn_obs *obs, const float *node_in, const float *edge_in, const float *masks, const char *who)
{
    CN_REQUIRE(p, "%s: null handle", who);
    CN_REQUIRE(p->have_weights, "%s: cn_srnn_set_weights has not been called", who);
    CN_REQUIRE(E >= 1 && E <= p->maxE, "%s: E = %d outside [1, max_envs = %d]", who, E, p->maxE);
    CN_REQUIRE(obs && obs->robot_node && obs->temporal_edges && obs->spatial_edges, "%s: null observation tensor", who);
    CN_REQUIRE(node_in && edge_in && masks, "%s: null hidden state / mask", who);
    return CN_OK;
}

} // namespace

extern "C" int cn_srnn_create(int human_num, int edge_width, int max_envs, cn_srnn **out)
{
    if (int rc = cn_require_device()) return rc;
    CN_REQUIRE(out, "cn_srnn_create: null out");
    CN_REQUIRE(human_num >= 1 && human_num <= CN_MAX_HUMANS, "cn_srnn_create: human_num must be in [1,%d]", CN_MAX_HUMANS);
    CN_REQUIRE(edge_width >= 1 && edge_width <= 64, "cn_srnn_create: edge_width must be in [1,64]");
    CN_REQUIRE(max_envs >= 1, "cn_srnn_create: max_envs must be positive");
    cn_srnn *p = new (std::nothrow) cn_srnn{};
    CN_REQUIRE(p, "cn_srnn_create: out of host memory");
    p->H = human_num; p->D = edge_width; p->maxE = max_envs; p->mode = 1;
    size_t n[SR_NW], off[SR_NW], total = 0;
    srnn_counts(edge_width, n);
    for (int i = 0; i < SR_NW; ++i) { off[i] = total; total += sr_align(n[i] * sizeof(float)); }
    size_t plane_off[8];            // W_hh planes, then W_hh^T planes
    for (int i = 0; i < 8; ++i) {
        plane_off[i] = total;
        total += sr_align((size_t)768 * 256 * sizeof(__bf16));
    }
    const size_t E = max_envs;
    const size_t o_attn = total; total += sr_align(E * human_num * sizeof(float));
    const size_t o_wgt = total; total += sr_align(E * 256 * sizeof(float));
    const size_t o_node = total; total += sr_align(E * 256 * sizeof(float));
    const size_t o_feat = total; total += sr_align(E * 256 * sizeof(float));
    hipError_t e = hipMalloc((void **)&p->pool, total);
    if (e != hipSuccess) {
        cn_set_error("cn_srnn_create: hipMalloc(%zu) failed: %s", total, hipGetErrorString(e));
        delete p;
        return CN_ERR_HIP;
    }
    for (int i = 0; i < SR_NW; ++i) p->w[i] = reinterpret_cast<const float *>(p->pool + off[i]);
    for (int i = 0; i < 4; ++i) p->planes[i] = reinterpret_cast<__bf16 *>(p->pool + plane_off[i]);
    for (int i = 0; i < 4; ++i) p->planes_t[i] = reinterpret_cast<__bf16 *>(p->pool + plane_off[4 + i]);
    p->tap_attn = reinterpret_cast<float *>(p->pool + o_attn);
    p->tap_weighted = reinterpret_cast<float *>(p->pool + o_wgt);
    p->tap_node = reinterpret_cast<float *>(p->pool + o_node);
    p->tap_feat = reinterpret_cast<float *>(p->pool + o_feat);
    *out = p;
    return CN_OK;
}

extern "C" int cn_srnn_destroy(cn_srnn *p)
{
    if (!p) return CN_OK;
    if (p->edge_ws) (void)hipFree(p->edge_ws);
    if (p->pool) (void)hipFree(p->pool);
    delete p;
    return CN_OK;
}

extern "C" int cn_srnn_set_weights(cn_srnn *p, const cn_srnn_weights *w, void *stream)
{
    if (int rc = cn_require_device()) return rc;
    CN_REQUIRE(p && w, "cn_srnn_set_weights: null argument");
    hipStream_t st = (hipStream_t)stream;
    const float *const *src = reinterpret_cast<const float *const *>(w);
    size_t n[SR_NW];
    srnn_counts(p->D, n);
    for (int i = 0; i < SR_NW; ++i) CN_REQUIRE(src[i], "cn_srnn_set_weights: weight pointer #%d is null", i);
    for (int i = 0; i < SR_NW; ++i) CN_HIP(hipMemcpyAsync(const_cast<float *>(p->w[i]), src[i], n[i] * sizeof(float), hipMemcpyDeviceToDevice, st));
    const int gru[2] = {W_GRU_S, W_GRU_T};
    for (int s = 0; s < 2; ++s) {          // W_hh of both edge GRUs as bf16 hi / lo planes
        const int cnt = 768 * 256;
        hipLaunchKernelGGL(srnn_split_kernel, dim3((cnt + 255) / 256), dim3(256), 0, st, cnt, p->w[gru[s] + 1], p->planes[s * 2], p->planes[s * 2 + 1]);
        CN_CHECK_LAUNCH();
        hipLaunchKernelGGL(srnn_split_t_kernel, dim3((cnt + 255) / 256), dim3(256), 0, st, p->w[gru[s] + 1], p->planes_t[s * 2], p->planes_t[s * 2 + 1]);
        CN_CHECK_LAUNCH();
    }
    p->have_weights = 1;
    return CN_OK;
}

extern "C" int cn_srnn_act(cn_srnn *p, int E, const cn_obs *obs, const float *node_hxs_in, const float *edge_hxs_in, const float *masks, const float *eps,
                           float *value, float *action, float *logp, float *node_hxs_out, float *edge_hxs_out, void *stream)
{
    if (int rc = cn_require_device()) return rc;
    if (int rc = srnn_check_call(p, E, obs, node_hxs_in, edge_hxs_in, masks, "cn_srnn_act")) return rc;
    CN_REQUIRE(value && action && logp && node_hxs_out && edge_hxs_out, "cn_srnn_act: null output");
    return srnn_forward(p, E, obs, node_hxs_in, edge_hxs_in, masks, eps, value, action, logp, node_hxs_out, edge_hxs_out, (hipStream_t)stream);
}

extern "C" int cn_srnn_get_value(cn_srnn *p, int E, const cn_obs *obs, const float *node_hxs_in, const float *edge_hxs_in, const float *masks, float *value,
                                 void *stream)
{
    if (int rc = cn_require_device()) return rc;
    if (int rc = srnn_check_call(p, E, obs, node_hxs_in, edge_hxs_in, masks, "cn_srnn_get_value")) return rc;
    CN_REQUIRE(value, "cn_srnn_get_value: null output");
    if (!p->edge_ws) CN_HIP(hipMalloc((void **)&p->edge_ws, (size_t)p->maxE * (p->H + 1) * 256 * sizeof(float)));
    return srnn_forward(p, E, obs, node_hxs_in, edge_hxs_in, masks, nullptr, value, nullptr, nullptr, nullptr, p->edge_ws, (hipStream_t)stream);
}

extern "C" int cn_srnn_get_taps(cn_srnn *p, int E, float *edge_out, float *attn, float *weighted, float *node_out, float *actor_feat, void *stream)
{
    if (int rc = cn_require_device()) return rc;
    CN_REQUIRE(p, "cn_srnn_get_taps: null handle");
    CN_REQUIRE(p->last_edge && E >= 1 && E <= p->lastE, "cn_srnn_get_taps: E = %d, the last forward had %d envs", E, p->lastE);
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)E;
    if (edge_out && edge_out != p->last_edge) CN_HIP(hipMemcpyAsync(edge_out, p->last_edge, n * (p->H + 1) * 256 * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (attn) CN_HIP(hipMemcpyAsync(attn, p->tap_attn, n * p->H * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (weighted) CN_HIP(hipMemcpyAsync(weighted, p->tap_weighted, n * 256 * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (node_out) CN_HIP(hipMemcpyAsync(node_out, p->tap_node, n * 256 * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (actor_feat) CN_HIP(hipMemcpyAsync(actor_feat, p->tap_feat, n * 256 * sizeof(float), hipMemcpyDeviceToDevice, st));
    return CN_OK;
}

extern "C" int cn_srnn_set_gemm_mode(cn_srnn *p, int mode)
{
    CN_REQUIRE(p, "cn_srnn_set_gemm_mode: null handle");
    CN_REQUIRE(mode == 0 || mode == 1, "cn_srnn_set_gemm_mode: mode must be 0 (exact fp32) or 1 (bf16x3)");
    p->mode = mode;
    return CN_OK;
}
