// gst_eval.hip -- evaluation of the GST trajectory predictor on gfx950 (cn_gst_eval_step): validation (decode on the mean) and the sampled
// test protocol (S decodes per sequence with the Gaussian sampled and fed back).
//
// Reference: gst_updated/scripts/experiments/eval.py:56-157 (`inference`, modes 'val' and 'test') over st_model.py:271-455 (forward with
// sampling = False / True, dropout off), :62-112 (negative_log_likelihood_full_partial), :232-243 (sample_gaussian) and mgnn/utils.py:8-28
// (average / final offset error).  The same forward as gst_train.hip without the reverse pass.
//
// Mapping.  Nothing is kept for a reverse pass, so a sequence's activations live in LDS: seven [N,64] slots (h, c, two temporaries and
// the q|k|v block, each reused along the layer) -- 112 KB at 64 pedestrians, 35 KB at 20, and 133 KB with everything else at 64 pedestrians and
// P = 8, inside the CU's 160 KiB (asserted below); the attention probabilities are never stored
// (each (row, head) thread makes two passes over the keys: maximum, then the exponentials with their sums); the 67 k weights stream
// from L2.  Two launches: gst_eval_encode_kernel, one workgroup per SEQUENCE, runs the five observed encoder passes and LSTM steps --
// they do not depend on the draws -- and leaves (h, c) in the workspace; gst_eval_decode_kernel, one workgroup per (sequence, sample),
// starts from that state and runs the P decode steps (P = pred_seq_len in 1 .. 8, the kernels' template parameter GP), the loss and the offset errors.  Plain fp32 FMA arithmetic with the training
// kernel's summation orders; every reduction has a fixed order (no atomics), so equal arguments give equal bits.
#include "common.h"
#include "gst_model.h"

#include <cmath>

namespace {

using namespace gst_model;

constexpr int MAXN = 64, MAXS = 64;
constexpr int RB = 4; // rows per thread in the matrix products: one weight load serves four pedestrians

// ---- LDS layout (floats) ----
struct Lds {
    float *H, *C, *T0, *T1, *Q, *X2, *MK, *MFP, *LM, *XS5, *RAW, *RED;
};
__host__ __device__ constexpr int eval_lds_floats(int N, int GP) { return 7 * N * 64 + ((N * 2 + 3) & ~3) + 64 + 64 + N * seq_steps(GP) + GP * N * 2 + GP * N * 5 + 8; }
static_assert(eval_lds_floats(MAXN, GP_MAX) * sizeof(float) <= 160 * 1024, "the largest (N, P) fits gfx950's 160 KiB of LDS per CU");
template <int GP>
__device__ inline Lds carve(float *p, int N)
{
    constexpr int TT = seq_steps(GP);
    Lds L;
    const int slot = N * 64;
    L.H = p; p += slot;
    L.C = p; p += slot;
    L.T0 = p; p += slot;      // T0 | T1 are contiguous: together they hold the FFN's hidden layer [N,128]
    L.T1 = p; p += slot;
    L.Q = p; p += 3 * slot;   // q|k|v [N,192]; after the attention its three thirds hold x1, LayerNorm1(x1) and the layer's output
    L.X2 = p; p += (N * 2 + 3) & ~3;
    L.MK = p; p += 64;
    L.MFP = p; p += 64;
    L.LM = p; p += N * TT;
    L.XS5 = p; p += GP * N * 2;
    L.RAW = p; p += GP * N * 5;
    L.RED = p;
    return L;
}

// y[r][f] = (res[r][f] + b[f] + sum_k W[f][k] x[r][k]) (relu) (* rowmask[r]);  x, y, res in LDS, W from global memory (16-byte aligned rows)
template <int K, int F, bool RELU>
__device__ void lin_lds(int N, const float *x, const float *__restrict__ W, const float *__restrict__ b, const float *res, const float *rowmask, float *y)
{
    const int groups = (N + RB - 1) / RB;
    for (int idx = threadIdx.x; idx < groups * F; idx += NT) {
        const int g = idx / F, f = idx - g * F, r0 = g * RB;
        const float4 *w4 = reinterpret_cast<const float4 *>(W + (size_t)f * K);
        const float4 *x4[RB];
        float acc[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int r = min(r0 + i, N - 1);
            x4[i] = reinterpret_cast<const float4 *>(x + r * K);
            acc[i] = b[f];
        }
        for (int k = 0; k < K / 4; ++k) {
            const float4 w = w4[k];
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                const float4 v = x4[i][k];
                acc[i] += w.x * v.x; acc[i] += w.y * v.y; acc[i] += w.z * v.z; acc[i] += w.w * v.w;
            }
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int r = r0 + i;
            if (r < N) {
                float v = acc[i];
                if (RELU) v = fmaxf(v, 0.0f);
                if (res) v = res[r * F + f] + v;
                if (rowmask) v *= rowmask[r];
                y[r * F + f] = v;
            }
        }
    }
}

// LayerNorm over 64 features of the value each lane holds (one wavefront per row, lane = feature)
__device__ __forceinline__ float ln_lane(float v, float g, float b)
{
    const float m = wv_sum(v) * (1.0f / 64.0f);
    const float d = v - m;
    const float var = wv_sum(d * d) * (1.0f / 64.0f);
    return d * (1.0f / sqrtf(var + 1e-5f)) * g + b;
}

// NodeEncoderLayer (dropout off) on the N rows of L.X2 with the 0/1 presence vector m: the output times m lands in the last third of L.Q
__device__ void layer_eval(const Lds &L, int N, const Wts &W, const float *m)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, slot = N * 64;
    float *N0 = L.T1, *O = L.T0, *QKV = L.Q, *X1 = L.Q, *N1 = L.Q + slot, *Ff = L.T0, *XS = L.Q + 2 * slot;
    // node_embedding (2 -> 64), LayerNorm(norm_node) * ped -> N0
    for (int r = wave; r < N; r += NT / 64) {
        const float e = W.p[P_EW][2 * lane] * L.X2[2 * r] + W.p[P_EW][2 * lane + 1] * L.X2[2 * r + 1] + W.p[P_EB][lane];
        N0[r * 64 + lane] = ln_lane(e, W.p[P_NW][lane], W.p[P_NB][lane]) * m[r];
    }
    __syncthreads();
    lin_lds<64, 192, false>(N, N0, W.p[P_INW], W.p[P_INB], nullptr, nullptr, QKV);
    __syncthreads();
    // attention per (row i, head h): softmax over all j, times the mask m_i m_j, renormalised (mha.py:236-242), times v
    for (int ih = threadIdx.x; ih < N * 8; ih += NT) {
        const int i = ih >> 3, h = ih & 7;
        const float *q = QKV + i * 192 + h * 8;
        float qs[8];
#pragma unroll
        for (int d = 0; d < 8; ++d) qs[d] = q[d] * 0.35355339059327373f;
        float mx = -INFINITY;
        for (int j = 0; j < N; ++j) {
            const float *k = QKV + j * 192 + 64 + h * 8;
            float s = 0.0f;
#pragma unroll
            for (int d = 0; d < 8; ++d) s += qs[d] * k[d];
            mx = fmaxf(mx, s);
        }
        float Z = 0.0f, Zm = 0.0f;
        float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < N; ++j) {
            const float *k = QKV + j * 192 + 64 + h * 8, *v = k + 64;
            float s = 0.0f;
#pragma unroll
            for (int d = 0; d < 8; ++d) s += qs[d] * k[d];
            const float e = expf(s - mx);
            Z += e;
            const float em = e * (m[i] * m[j]);
            Zm += em;
#pragma unroll
            for (int d = 0; d < 8; ++d) o[d] += em * v[d];
        }
        // p_j = e_j / Z; masked sum S = Zm / Z; output sum_j p_j mask_ij v_j / (S + 1e-10)
        const float inv = 1.0f / Z, sc = inv / (Zm * inv + 1e-10f);
#pragma unroll
        for (int d = 0; d < 8; ++d) O[i * 64 + h * 8 + d] = o[d] * sc;
    }
    __syncthreads();
    lin_lds<64, 64, false>(N, O, W.p[P_OW], W.p[P_OB], N0, nullptr, X1);                 // x1 = n0 + out_proj(o)   (q|k|v is dead)
    __syncthreads();
    for (int r = wave; r < N; r += NT / 64) N1[r * 64 + lane] = ln_lane(X1[r * 64 + lane], W.p[P_N1W][lane], W.p[P_N1B][lane]);
    __syncthreads();
    lin_lds<64, 128, true>(N, N1, W.p[P_L1W], W.p[P_L1B], nullptr, nullptr, Ff);         // (o and n0 are dead: the hidden layer takes T0 | T1)
    __syncthreads();
    lin_lds<128, 64, false>(N, Ff, W.p[P_L2W], W.p[P_L2B], X1, m, XS);                   // (x1 + linear2(f)) * m: the LSTM's input
    __syncthreads();
}

// LSTM cell (PyTorch gate order i, f, g, o) on x = last third of L.Q: (h, c) <- blend ? mk (h', c') + (1 - mk) (h, c) : (h', c')
__device__ void lstm_eval(const Lds &L, int N, const Wts &W, const float *blend)
{
    const float *x = L.Q + 2 * N * 64;
    float *Hn = L.T0;
    const int groups = (N + RB - 1) / RB;
    for (int idx = threadIdx.x; idx < groups * 64; idx += NT) {
        const int g = idx >> 6, d = idx & 63, r0 = g * RB;
        float acc[4][RB];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int i = 0; i < RB; ++i) acc[q][i] = W.p[P_BIH][q * 64 + d] + W.p[P_BHH][q * 64 + d];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const float *in = half ? L.H : x;
            const float *Wm = half ? W.p[P_WHH] : W.p[P_WIH];
            for (int k = 0; k < 16; ++k) {
                float4 w[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) w[q] = reinterpret_cast<const float4 *>(Wm + (size_t)(q * 64 + d) * 64)[k];
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    const float4 v = reinterpret_cast<const float4 *>(in + min(r0 + i, N - 1) * 64)[k];
#pragma unroll
                    for (int q = 0; q < 4; ++q) { acc[q][i] += w[q].x * v.x; acc[q][i] += w[q].y * v.y; acc[q][i] += w[q].z * v.z; acc[q][i] += w[q].w * v.w; }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int r = r0 + i;
            if (r < N) {
                const float gi = sigm(acc[0][i]), gf = sigm(acc[1][i]), gg = tanhf(acc[2][i]), go = sigm(acc[3][i]);
                const float c_old = L.C[r * 64 + d];
                const float cn = gf * c_old + gi * gg;
                const float hn = go * tanhf(cn);
                if (blend) {
                    const float mk = blend[r];
                    L.C[r * 64 + d] = cn * mk + c_old * (1.0f - mk);
                    Hn[r * 64 + d] = hn * mk + L.H[r * 64 + d] * (1.0f - mk);
                } else {
                    L.C[r * 64 + d] = cn;
                    Hn[r * 64 + d] = hn;
                }
            }
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < N * 64; idx += NT) L.H[idx] = Hn[idx];
    __syncthreads();
}

// sum over the workgroup in a fixed order (every thread calls it); the total is returned to all threads
__device__ float block_sum(float v, float *red)
{
    v = wv_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// observed period of one sequence: five encoder passes and LSTM steps -> (h, c) times lm_fp into state [B][2][N,64]
template <int GP>
__global__ __launch_bounds__(NT) void gst_eval_encode_kernel(int N, const float *__restrict__ v_obs, const float *__restrict__ lm_all, Wts W, float *__restrict__ state)
{
    constexpr int TT = seq_steps(GP);
    extern __shared__ __align__(16) float lds_eval[];
    const Lds L = carve<GP>(lds_eval, N);
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < N * TT; i += NT) L.LM[i] = lm_all[(size_t)b * N * TT + i];
    for (int idx = threadIdx.x; idx < N * 64; idx += NT) { L.H[idx] = 0.0f; L.C[idx] = 0.0f; }
    __syncthreads();
    for (int t = 0; t < GT; ++t) {
        for (int r = threadIdx.x; r < N; r += NT) L.MK[r] = L.LM[r * TT + t];
        for (int i = threadIdx.x; i < N * 2; i += NT) L.X2[i] = v_obs[((size_t)b * GT + t) * N * 2 + i];
        __syncthreads();
        layer_eval(L, N, W, L.MK);
        lstm_eval(L, N, W, nullptr);
    }
    float *st = state + (size_t)b * 2 * N * 64;
    for (int idx = threadIdx.x; idx < N * 64; idx += NT) {
        const float mk = L.LM[(idx >> 6) * TT + GT - 1];
        st[idx] = L.H[idx] * mk;
        st[N * 64 + idx] = L.C[idx] * mk;
    }
}

// prediction period of one (sequence, sample): head, sample (or mean), GP - 1 encoder passes + LSTM steps on what was fed back, loss, offset errors
template <int GP>
__global__ __launch_bounds__(NT) void gst_eval_decode_kernel(int N, int S1, const float *__restrict__ v_pred, const float *__restrict__ lm_all, Wts W,
                                                              const float *__restrict__ noise, const float *__restrict__ state, float *__restrict__ seq_out,
                                                              float *__restrict__ ped_out, float *__restrict__ gauss_out)
{
    constexpr int TT = seq_steps(GP);
    extern __shared__ __align__(16) float lds_eval[];
    const Lds L = carve<GP>(lds_eval, N);
    const int bs = blockIdx.x, b = bs / S1;
    const float *st = state + (size_t)b * 2 * N * 64;
    for (int i = threadIdx.x; i < N * TT; i += NT) L.LM[i] = lm_all[(size_t)b * N * TT + i];
    for (int idx = threadIdx.x; idx < N * 64; idx += NT) { L.H[idx] = st[idx]; L.C[idx] = st[N * 64 + idx]; }
    __syncthreads();
    for (int r = threadIdx.x; r < N; r += NT) L.MFP[r] = L.LM[r * TT + GT - 1];
    __syncthreads();
    for (int tt = 0; tt < GP; ++tt) {
        if (tt > 0) {
            layer_eval(L, N, W, L.MFP);
            lstm_eval(L, N, W, L.MFP);
        }
        float *RAW = L.RAW + tt * N * 5;
        for (int idx = threadIdx.x; idx < N * 5; idx += NT) {
            const int r = idx / 5, f = idx - r * 5;
            const float *w = W.p[P_HW] + f * 64, *hr = L.H + r * 64;
            float acc = W.p[P_HB][f];
            for (int k = 0; k < 64; ++k) acc += w[k] * hr[k];
            RAW[idx] = acc;
        }
        __syncthreads();
        // raw2gaussian (st_model.py:188-209) and sample_gaussian (:232-243) with the caller's draws; the fed-back value is masked with lm_fp (:377, :420)
        for (int n = threadIdx.x; n < N; n += NT) {
            const float *raw = RAW + n * 5;
            const float mux = raw[0], muy = raw[1], sx = expf(raw[2]), sy = expf(raw[3]), rho = tanhf(raw[4]);
            if (gauss_out) {
                float *go = gauss_out + (((size_t)bs * GP + tt) * N + n) * 5;
                go[0] = mux; go[1] = muy; go[2] = sx; go[3] = sy; go[4] = rho;
            }
            float x = mux, y = muy;
            if (noise) {
                const float *e = noise + (((size_t)bs * GP + tt) * N + n) * 2;
                x = mux + sx * e[0];
                y = muy + (rho * sy * e[0] + sqrtf(1.0f - rho * rho) * sy * e[1]);
            }
            x *= L.MFP[n]; y *= L.MFP[n];
            L.X2[2 * n] = x; L.X2[2 * n + 1] = y;
            L.XS5[(tt * N + n) * 2] = x; L.XS5[(tt * N + n) * 2 + 1] = y;
        }
        __syncthreads();
    }
    // masked negative log-likelihood (st_model.py:62-112): sum and number of valid (step, pedestrian) pairs
    float lsum = 0.0f, cnt = 0.0f;
    for (int idx = threadIdx.x; idx < GP * N; idx += NT) {
        const int tt = idx / N, n = idx - tt * N;
        const float M = L.LM[n * TT + GT + tt] * L.MFP[n];
        if (M > 0.0f) {
            const float *raw = L.RAW + idx * 5;
            const float mux = raw[0], muy = raw[1], sx = expf(raw[2]), sy = expf(raw[3]), rho = tanhf(raw[4]);
            const float *xt = v_pred + (((size_t)b * GP + tt) * N + n) * 2;
            const float nx = (xt[0] - mux) / sx, ny = (xt[1] - muy) / sy;
            const float a = 1.0f - rho * rho;
            const float Q = nx * nx - 2.0f * rho * nx * ny + ny * ny;
            lsum += 0.5f * logf(a) + logf(sx) + logf(sy) + Q / (2.0f * a);
            cnt += 1.0f;
        }
    }
    // average / final offset error (mgnn/utils.py:8-28) of the fed-back values, for the pedestrians present at all TT steps; everyone else: exactly 0
    for (int n = threadIdx.x; n < N; n += NT) {
        float present = 0.0f;
        for (int t = 0; t < TT; ++t) present += L.LM[n * TT + t];
        const float pp = present == (float)TT ? 1.0f : 0.0f;
        float a = 0.0f, f = 0.0f;
        if (pp > 0.0f) {
            float px = 0.0f, py = 0.0f, gx = 0.0f, gy = 0.0f, es = 0.0f;
            for (int tt = 0; tt < GP; ++tt) {
                const float *xt = v_pred + (((size_t)b * GP + tt) * N + n) * 2;
                px += L.XS5[(tt * N + n) * 2]; py += L.XS5[(tt * N + n) * 2 + 1];
                gx += xt[0]; gy += xt[1];
                const float dx = px - gx, dy = py - gy;
                f = sqrtf(dx * dx + dy * dy);
                es += f;
            }
            a = es / (float)GP;
        }
        if (ped_out) {
            float *po = ped_out + ((size_t)bs * N + n) * 3;
            po[0] = a; po[1] = f; po[2] = pp;
        }
        L.X2[2 * n] = a; L.X2[2 * n + 1] = f;      // (the fed-back value's buffer is free by now)
    }
    lsum = block_sum(lsum, L.RED);
    cnt = block_sum(cnt, L.RED + 4);
    if (threadIdx.x == 0) {
        // the sums over at most 64 pedestrians in float64, pedestrian order: they are compared with sums of a few tens at a few 1e-5
        double aoe = 0.0, foe = 0.0;
        for (int n = 0; n < N; ++n) { aoe += (double)L.X2[2 * n]; foe += (double)L.X2[2 * n + 1]; }
        float *so = seq_out + (size_t)bs * 4;
        so[0] = lsum; so[1] = cnt; so[2] = (float)aoe; so[3] = (float)foe;
    }
}

size_t eval_ws_bytes(int B, int N) { return ((size_t)B * 2 * N * 64 * sizeof(float) + 255) & ~size_t(255); }

} // namespace

extern "C" int64_t cn_gst_eval_workspace_bytes_horizon(int B, int N, int S, int P)
{
    if (B < 1 || N < 4 || N > MAXN || S < 0 || S > MAXS || P < 1 || P > GP_MAX) return 0;
    return (int64_t)eval_ws_bytes(B, N);
}
extern "C" int64_t cn_gst_eval_workspace_bytes(int B, int N, int S) { return cn_gst_eval_workspace_bytes_horizon(B, N, S, GP_DEFAULT); }

extern "C" int cn_gst_eval_step(int B, int N, int S, const float *v_obs, const float *v_pred, const float *loss_mask_rel, const cn_gst_weights *w, const float *noise,
                                void *workspace, int64_t workspace_bytes, float *seq_out, float *ped_out, float *gauss_out, void *stream)
{
    return cn_gst_eval_step_horizon(B, N, S, GP_DEFAULT, v_obs, v_pred, loss_mask_rel, w, noise, workspace, workspace_bytes, seq_out, ped_out, gauss_out, stream);
}

extern "C" int cn_gst_eval_step_horizon(int B, int N, int S, int P, const float *v_obs, const float *v_pred, const float *loss_mask_rel, const cn_gst_weights *w, const float *noise,
                                void *workspace, int64_t workspace_bytes, float *seq_out, float *ped_out, float *gauss_out, void *stream)
{
    if (int rc = cn_require_device()) return rc;
    CN_REQUIRE(B >= 1 && N >= 4 && N <= MAXN, "cn_gst_eval_step: B=%d sequences of N=%d pedestrians outside B >= 1, 4 <= N <= 64 (pad small crowds with absent pedestrians)", B, N);
    CN_REQUIRE(S >= 0 && S <= MAXS, "cn_gst_eval_step: S=%d samples per sequence outside 0 (validation: decode on the mean) .. 64", S);
    CN_REQUIRE(P >= 1 && P <= GP_MAX, "cn_gst_eval_step: P=%d predicted steps outside [1, %d]", P, GP_MAX);
    CN_REQUIRE(v_obs && v_pred && loss_mask_rel && w && workspace && seq_out, "cn_gst_eval_step: null argument (v_obs, v_pred, loss_mask_rel, w, workspace, seq_out are required)");
    CN_REQUIRE(S == 0 || noise, "cn_gst_eval_step: noise is NULL with S=%d samples: the caller supplies the [B,S,P,N,2] standard-normal draws", S);
    CN_REQUIRE(S > 0 || !noise, "cn_gst_eval_step: noise given with S=0 (validation decodes on the mean; pass NULL)");
    const size_t need = eval_ws_bytes(B, N);
    CN_REQUIRE(workspace_bytes >= (int64_t)need && ((uintptr_t)workspace & 15) == 0, "cn_gst_eval_step: workspace of %lld bytes (16-byte aligned) needed, got %lld",
               (long long)need, (long long)workspace_bytes);
    Wts W;
    const float *const *wp = reinterpret_cast<const float *const *>(w);
    for (int i = 0; i < NPARAM; ++i) {
        CN_REQUIRE(wp[i] && ((uintptr_t)wp[i] & 15) == 0, "cn_gst_eval_step: weight pointer #%d is null or not 16-byte aligned", i);
        W.p[i] = wp[i];
    }
    const int S1 = S > 0 ? S : 1;
    const size_t lds = (size_t)eval_lds_floats(N, P) * sizeof(float);
    CN_REQUIRE(lds <= 160 * 1024, "cn_gst_eval_step: N=%d pedestrians at P=%d predicted steps need %zu bytes of LDS, a CU has 160 KiB", N, P, lds);
    hipStream_t st = (hipStream_t)stream;
    float *state = (float *)workspace;
    return for_horizon(P, [&](auto gp) -> int {
        constexpr int GP = decltype(gp)::value;
        constexpr int max_lds = eval_lds_floats(MAXN, GP) * (int)sizeof(float);
        if (int rc = cn_lds_opt_in<&gst_eval_encode_kernel<GP>>(max_lds)) return rc;
        if (int rc = cn_lds_opt_in<&gst_eval_decode_kernel<GP>>(max_lds)) return rc;
        hipLaunchKernelGGL(gst_eval_encode_kernel<GP>, dim3(B), dim3(NT), lds, st, N, v_obs, loss_mask_rel, W, state);
        CN_CHECK_LAUNCH();
        hipLaunchKernelGGL(gst_eval_decode_kernel<GP>, dim3(B * S1), dim3(NT), lds, st, N, S1, v_pred, loss_mask_rel, W, noise, state, seq_out, ped_out, gauss_out);
        CN_CHECK_LAUNCH();
        return CN_OK;
    });
}
