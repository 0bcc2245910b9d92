// srnn_train.hip -- the edge-GRU sequence of the DS-RNN baseline's PPO update on the cn_srnn handle: cn_srnn_seq_fwd (T launches of the rollout's
// edge kernel, which also leaves the gates and the embedding in the workspace) and cn_srnn_seq_bwd (T BPTT launches, then the weight gradients
// of each set as range partials added in range order).  No host synchronisation, no framework kernel and no atomics on data inside a call.
#include "srnn_train_kernels.h"

namespace {

struct SeqLayout {                      // the workspace, in floats; per-set blocks are [T, rows of the set, ...]
    size_t rows_t, rows_s;              // rows of a step: N temporal, N * H spatial
    size_t gates_t, gates_s, emb_t, emb_s, de_t, de_s, carry, total;
};

// 0 = refused shape
bool seq_layout(int T, int N, int H, int D, SeqLayout *L)
{
    if (T < 1 || N < 1 || H < 1 || H > 64 || D < 1 || D > 64) return false;
    const unsigned long long R = (unsigned long long)N * (H + 1), TR = R * (unsigned long long)T;
    if (TR * 1024ull > 0xffffffffull) return false;       // the saved gates stay inside 32-bit element offsets
    L->rows_t = N; L->rows_s = (size_t)N * H;
    const size_t tt = (size_t)T * L->rows_t, ts = (size_t)T * L->rows_s;
    size_t o = 0;
    L->gates_t = o; o += tt * 1024;
    L->gates_s = o; o += ts * 1024;
    L->emb_t = o; o += tt * 64;
    L->emb_s = o; o += ts * 64;
    L->de_t = o; o += tt * 64;
    L->de_s = o; o += ts * 64;
    L->carry = o; o += (size_t)R * 256;
    L->total = o;
    return true;
}

int seq_check(const cn_srnn *p, int T, int N, const float *temporal, const float *spatial, const float *edge_h0, const float *masks, const void *workspace,
              int64_t workspace_bytes, SeqLayout *L, const char *who)
{
    CN_REQUIRE(p, "%s: null handle", who);
    CN_REQUIRE(p->have_weights, "%s: cn_srnn_set_weights has not been called", who);
    CN_REQUIRE(seq_layout(T, N, p->H, p->D, L), "%s: unsupported shape T = %d, N = %d, H = %d, D = %d (cn_srnn_seq_workspace_bytes returns 0)", who, T, N,
               p->H, p->D);
    CN_REQUIRE(temporal && spatial, "%s: null observation tensor", who);
    CN_REQUIRE(edge_h0 && masks, "%s: null hidden state / mask", who);
    CN_REQUIRE(workspace, "%s: null workspace", who);
    CN_REQUIRE(workspace_bytes >= (int64_t)(L->total * sizeof(float)), "%s: T * N = %d * %d needs a workspace of %zu bytes, the caller's has %lld", who, T, N,
               L->total * sizeof(float), (long long)workspace_bytes);
    return CN_OK;
}

SrnnBwdW bwd_weights(const cn_srnn *p, int spatial)
{
    const int gru = spatial ? W_GRU_S : W_GRU_T, plane = spatial ? 0 : 2;
    SrnnBwdW w;
    w.w_ih = p->w[gru]; w.w_hh = p->w[gru + 1];
    w.hht_hi = p->planes_t[plane]; w.hht_lo = p->planes_t[plane + 1];
    return w;
}

int reduce(hipStream_t st, int n, int cols, float *dst, const float *P, int chunks, size_t chunk_stride, int ldp, int col_off, int row_split, int row_add)
{
    hipLaunchKernelGGL(srnn_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, cols, dst, P, chunks, chunk_stride, ldp, col_off, row_split, row_add);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

// the six gradients of one weight set, from its [M, ...] blocks of the workspace
int set_wgrads(hipStream_t st, int T, int N, int H, int is_t, int din, const float *x, const float *gates, const float *emb, const float *de,
               const float *h_all, const float *edge_h0, const float *masks, float *partials, float *const *g /* enc_w, enc_b, w_ih, w_hh, b_ih, b_hh */)
{
    const int rows_set = is_t ? N : N * H, M = T * rows_set;
    int rpc = (M + CN_SRNN_SEQ_CHUNKS - 1) / CN_SRNN_SEQ_CHUNKS;
    rpc = (rpc + SW_ROWS - 1) / SW_ROWS * SW_ROWS;
    if (rpc < 256) rpc = 256;
    const int chunks = (M + rpc - 1) / rpc;
    float *p_hh = partials, *p_ih = p_hh + (size_t)CN_SRNN_SEQ_CHUNKS * 768 * 256, *p_enc = p_ih + (size_t)CN_SRNN_SEQ_CHUNKS * 1024 * 80;
    SrnnWgradArgs a{};
    a.M = M; a.rows_per_chunk = rpc; a.N = N; a.H = H; a.is_t = is_t; a.rows_set = rows_set;
    // dW_hh = d_gh^T . (mask * h_prev): planes 0, 1, 3 of the gradients
    a.D = gates; a.ldd = 1024; a.ncols = 768; a.skip = 256; a.h_all = h_all; a.edge_h0 = edge_h0; a.masks = masks; a.P = p_hh;
    hipLaunchKernelGGL((srnn_wgrad_kernel<16, SW_A_HP>), dim3(6, chunks), dim3(SW_THREADS), 0, st, a);
    CN_CHECK_LAUNCH();
    // [dW_ih | db] = [dr, dz, dn, dn r]^T . [e | 1]
    a.ncols = 1024; a.skip = 0; a.A = emb; a.lda = 64; a.ka = 64; a.P = p_ih;
    hipLaunchKernelGGL((srnn_wgrad_kernel<5, SW_A_PLAIN>), dim3(8, chunks), dim3(SW_THREADS), 0, st, a);
    CN_CHECK_LAUNCH();
    // [d enc_w | d enc_b] = d_e^T . [x | 1]
    const int kb = din + 1 <= 16 ? 1 : 5;
    a.D = de; a.ldd = 64; a.ncols = 64; a.A = x; a.lda = din; a.ka = din; a.P = p_enc;
    if (kb == 1)
        hipLaunchKernelGGL((srnn_wgrad_kernel<1, SW_A_PLAIN>), dim3(1, chunks), dim3(SW_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL((srnn_wgrad_kernel<5, SW_A_PLAIN>), dim3(1, chunks), dim3(SW_THREADS), 0, st, a);
    CN_CHECK_LAUNCH();
    const int none = 1 << 30;
    if (int rc = reduce(st, 64 * din, din, g[0], p_enc, chunks, (size_t)64 * kb * 16, kb * 16, 0, none, 0)) return rc;
    if (int rc = reduce(st, 64, 1, g[1], p_enc, chunks, (size_t)64 * kb * 16, kb * 16, din, none, 0)) return rc;
    if (int rc = reduce(st, 768 * 64, 64, g[2], p_ih, chunks, (size_t)1024 * 80, 80, 0, none, 0)) return rc;
    if (int rc = reduce(st, 768 * 256, 256, g[3], p_hh, chunks, (size_t)768 * 256, 256, 0, none, 0)) return rc;
    if (int rc = reduce(st, 768, 1, g[4], p_ih, chunks, (size_t)1024 * 80, 80, 64, none, 0)) return rc;
    return reduce(st, 768, 1, g[5], p_ih, chunks, (size_t)1024 * 80, 80, 64, 512, 256);      // b_hh's n gate: the dn * r plane
}

} // namespace

extern "C" int64_t cn_srnn_seq_workspace_bytes(int T, int N, int H, int D)
{
    SeqLayout L;
    return seq_layout(T, N, H, D, &L) ? (int64_t)(L.total * sizeof(float)) : 0;
}

extern "C" int cn_srnn_seq_fwd(cn_srnn *p, int T, int N, const float *temporal_edges, const float *spatial_edges, const float *edge_h0, const float *masks,
                               float *h_all, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (int rc = cn_require_device()) return rc;
    SeqLayout L;
    if (int rc = seq_check(p, T, N, temporal_edges, spatial_edges, edge_h0, masks, workspace, workspace_bytes, &L, "cn_srnn_seq_fwd")) return rc;
    CN_REQUIRE(h_all, "cn_srnn_seq_fwd: null output");
    hipStream_t st = (hipStream_t)stream;
    const int H = p->H;
    if (int rc = cn_lds_opt_in<&srnn_edge_gru_kernel<1, 1>>((int)SR_EDGE_LDS)) return rc;
    if (int rc = cn_lds_opt_in<&srnn_edge_gru_kernel<0, 1>>((int)SR_EDGE_LDS)) return rc;
    const SrnnEdgeW ws = srnn_edge_weights(p, 1), wt = srnn_edge_weights(p, 0);
    const int tiles_t = (N + SR_TILE - 1) / SR_TILE;
    const int tiles_s = (int)((L.rows_s + SR_TILE - 1) / SR_TILE);
    const dim3 grid((unsigned)(tiles_t + tiles_s));
    const size_t R = (size_t)N * (H + 1);
    float *wsf = static_cast<float *>(workspace);
    for (int t = 0; t < T; ++t) {
        SrnnEdgeSave sv;
        sv.gates_t = wsf + L.gates_t + (size_t)t * L.rows_t * 1024; sv.gates_s = wsf + L.gates_s + (size_t)t * L.rows_s * 1024;
        sv.emb_t = wsf + L.emb_t + (size_t)t * L.rows_t * 64; sv.emb_s = wsf + L.emb_s + (size_t)t * L.rows_s * 64;
        const float *tin = temporal_edges + (size_t)t * N * 2, *sin = spatial_edges + (size_t)t * L.rows_s * p->D;
        const float *hin = t ? h_all + (size_t)(t - 1) * R * SR_HID : edge_h0;
        float *hout = h_all + (size_t)t * R * SR_HID;
        if (p->mode)
            hipLaunchKernelGGL((srnn_edge_gru_kernel<1, 1>), grid, dim3(SR_EDGE_THREADS), SR_EDGE_LDS, st, N, H, tiles_t, wt, ws, tin, sin, hin, masks + (size_t)t * N,
                               hout, sv);
        else
            hipLaunchKernelGGL((srnn_edge_gru_kernel<0, 1>), grid, dim3(SR_EDGE_THREADS), SR_EDGE_LDS, st, N, H, tiles_t, wt, ws, tin, sin, hin, masks + (size_t)t * N,
                               hout, sv);
        CN_CHECK_LAUNCH();
    }
    return CN_OK;
}

extern "C" int cn_srnn_seq_bwd(cn_srnn *p, int T, int N, const float *temporal_edges, const float *spatial_edges, const float *edge_h0, const float *masks,
                               const float *h_all, const float *d_h_all, void *workspace, int64_t workspace_bytes, const cn_srnn_edge_grads *grads,
                               float *d_edge_h0, void *partials, void *stream)
{
    if (int rc = cn_require_device()) return rc;
    SeqLayout L;
    if (int rc = seq_check(p, T, N, temporal_edges, spatial_edges, edge_h0, masks, workspace, workspace_bytes, &L, "cn_srnn_seq_bwd")) return rc;
    CN_REQUIRE(h_all && d_h_all, "cn_srnn_seq_bwd: null h_all / d_h_all");
    CN_REQUIRE(grads && partials, "cn_srnn_seq_bwd: null grads / partials");
    float *const *gp = reinterpret_cast<float *const *>(grads);
    for (int i = 0; i < 12; ++i) CN_REQUIRE(gp[i], "cn_srnn_seq_bwd: gradient pointer #%d is null", i);
    hipStream_t st = (hipStream_t)stream;
    const int H = p->H;
    if (int rc = cn_lds_opt_in<&srnn_edge_bwd_kernel<1>>((int)SR_BWD_LDS)) return rc;
    if (int rc = cn_lds_opt_in<&srnn_edge_bwd_kernel<0>>((int)SR_BWD_LDS)) return rc;
    const SrnnBwdW ws = bwd_weights(p, 1), wt = bwd_weights(p, 0);
    const int tiles_t = (N + SR_TILE - 1) / SR_TILE;
    const int tiles_s = (int)((L.rows_s + SR_TILE - 1) / SR_TILE);
    const dim3 grid((unsigned)(tiles_t + tiles_s));
    const size_t R = (size_t)N * (H + 1);
    float *wsf = static_cast<float *>(workspace);
    for (int t = T - 1; t >= 0; --t) {
        SrnnBwdStep s;
        s.d_h = d_h_all + (size_t)t * R * SR_HID;
        s.h_prev = t ? h_all + (size_t)(t - 1) * R * SR_HID : edge_h0;
        s.masks = masks + (size_t)t * N;
        s.gates_t = wsf + L.gates_t + (size_t)t * L.rows_t * 1024; s.gates_s = wsf + L.gates_s + (size_t)t * L.rows_s * 1024;
        s.emb_t = wsf + L.emb_t + (size_t)t * L.rows_t * 64; s.emb_s = wsf + L.emb_s + (size_t)t * L.rows_s * 64;
        s.de_t = wsf + L.de_t + (size_t)t * L.rows_t * 64; s.de_s = wsf + L.de_s + (size_t)t * L.rows_s * 64;
        s.carry = wsf + L.carry;
        s.carry_out = (t == 0 && d_edge_h0) ? d_edge_h0 : s.carry;
        s.last = t == T - 1;
        if (p->mode)
            hipLaunchKernelGGL(srnn_edge_bwd_kernel<1>, grid, dim3(SR_EDGE_THREADS), SR_BWD_LDS, st, N, H, tiles_t, wt, ws, s);
        else
            hipLaunchKernelGGL(srnn_edge_bwd_kernel<0>, grid, dim3(SR_EDGE_THREADS), SR_BWD_LDS, st, N, H, tiles_t, wt, ws, s);
        CN_CHECK_LAUNCH();
    }
    // spatial set (fields 0 .. 5 of the grads), then temporal (6 .. 11): the partials buffer serves one set at a time, in stream order
    if (int rc = set_wgrads(st, T, N, H, 0, p->D, spatial_edges, wsf + L.gates_s, wsf + L.emb_s, wsf + L.de_s, h_all, edge_h0, masks,
                            static_cast<float *>(partials), gp))
        return rc;
    return set_wgrads(st, T, N, H, 1, 2, temporal_edges, wsf + L.gates_t, wsf + L.emb_t, wsf + L.de_t, h_all, edge_h0, masks, static_cast<float *>(partials),
                      gp + 6);
}
