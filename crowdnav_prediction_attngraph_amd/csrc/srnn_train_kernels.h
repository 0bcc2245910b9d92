// srnn_train_kernels.h -- the backward of the DS-RNN baseline's edge-GRU sequence (the forward is srnn_edge_gru_kernel<., SAVE = 1> of
// srnn_kernels.h, once per step), launched by srnn_train.hip:
//   srnn_edge_bwd_kernel   one BPTT step of both edge GRUs: gate gradients, the carry product d_gh . W_hh and d_e = (d_gi . W_ih) [e > 0]
//   srnn_wgrad_kernel      partial weight gradients D^T . A of one weight set over a range of its rows (exact fp32 MFMA)
//   srnn_reduce_kernel     adds the ranges' partials in range order and lays the sums out as the parameter's gradient
// The rules of srnn_edge_gru_kernel hold: no atomics on data, fixed summation orders, equal arguments give equal bits.
#pragma once
#define SRNN_EDGE_KERNEL_ONLY
#include "srnn_kernels.h"

namespace {

constexpr int SB_LDF = SR_HID + 4;      // fp32 row stride of one gate's d_gi (and, exact mode, d_gh) plane in LDS
// split mode: fp32 d_gi plane (66 560 B) + hi / lo planes of d_gh (2 x 64 x 264 x 2 = 67 584 B); exact mode: two fp32 planes (133 120 B)
constexpr size_t SR_BWD_LDS = (size_t)SR_TILE * SB_LDF * sizeof(float) + (size_t)2 * SR_TILE * SR_LDH * sizeof(__bf16);

struct SrnnBwdW {                       // what the backward reads of one weight set
    const float *w_ih, *w_hh;           // [768,64], [768,256]
    const __bf16 *hht_hi, *hht_lo;      // split planes of W_hh^T [256,768]
};

struct SrnnBwdStep {
    const float *d_h;                   // gradient of h_all[t], [N * (H+1), 256]
    const float *h_prev;                // h_all[t-1], or edge_h0 at t = 0
    const float *masks;                 // masks[t], [N]
    float *gates_t, *gates_s;           // step t of the saved gates [rows of the set, 4, 256]: r, z, n, hn in; dr, dz, dn, dn * r out
    const float *emb_t, *emb_s;         // step t of the saved embedding [rows of the set, 64]
    float *de_t, *de_s;                 // step t of d_e [rows of the set, 64]
    float *carry;                       // [N * (H+1), 256]: the carry into step t (not read when `last`), then g * z
    float *carry_out;                   // the carry into step t - 1 (carry itself, or d_edge_h0 at t = 0)
    int last;                           // t == T - 1: no carry comes in
};

// One BPTT step for a tile of 64 rows of one weight set (the gathering of srnn_edge_gru_kernel).  With g = d_h + carry and hp = mask * h_prev:
//   dn = g (1 - z)(1 - n^2), dz = g (hp - n) z (1 - z), dr = dn hn r (1 - r);  d_gi = [dr, dz, dn], d_gh = [dr, dz, dn r]
//   carry' = mask (g z + d_gh . W_hh)   K = 768, split bf16x3 on v_mfma_f32_16x16x32_bf16 (SPLIT) or v_mfma_f32_16x16x4_f32
//   d_e    = (d_gi . W_ih) [e > 0]      K = 768, exact fp32 MFMA in both modes
// Phase 0 is elementwise: each thread overwrites the saved gates of its elements with the four gradients and leaves g z in `carry`.  The 768
// columns of d_gh as hi / lo planes do not fit the LDS beside anything else, so the two products run gate by gate: a gate's 256 columns are
// staged (read back from where phase 0 wrote them, by the same workgroup), the accumulators -- per wavefront two 16-column blocks of the
// carry for all 64 rows and two 16 x 16 blocks of d_e -- live in registers across the three gates.  A row's result does not depend on the
// other rows of its tile.
template <int SPLIT>
__global__ __launch_bounds__(SR_EDGE_THREADS) void srnn_edge_bwd_kernel(int E, int H, int tiles_t, SrnnBwdW wt, SrnnBwdW ws, SrnnBwdStep s)
{
    extern __shared__ __attribute__((aligned(16))) char sb_smem[];
    float *fi = reinterpret_cast<float *>(sb_smem);                          // d_gi of the gate, fp32
    float *fh = fi + SR_TILE * SB_LDF;                                       // exact mode: d_gh of the gate, fp32
    __bf16 *xh = reinterpret_cast<__bf16 *>(fi + SR_TILE * SB_LDF);          // split mode: d_gh of the gate, hi and lo planes
    __bf16 *xl = xh + SR_TILE * SR_LDH;
    const bool is_t = (int)blockIdx.x < tiles_t;
    const SrnnBwdW w = is_t ? wt : ws;
    const long long nrows = is_t ? (long long)E : (long long)E * H;
    const long long r0 = (long long)(is_t ? blockIdx.x : blockIdx.x - tiles_t) * SR_TILE;
    const int tid = threadIdx.x;
    auto env_of = [&](long long r) { return is_t ? r : r / H; };
    auto edge_row = [&](long long r) { return is_t ? r * (H + 1) : (r / H) * (H + 1) + 1 + r % H; };
    float *gates = is_t ? s.gates_t : s.gates_s;
    const float *emb = is_t ? s.emb_t : s.emb_s;
    float *de = is_t ? s.de_t : s.de_s;

    // ---- phase 0: the gate gradients, in place ----
    for (int idx = tid; idx < SR_TILE * (SR_HID / 4); idx += SR_EDGE_THREADS) {
        const int row = idx >> 6, c4 = (idx & 63) * 4;
        const long long r = r0 + row;
        if (r < nrows) {
            const size_t o = (size_t)edge_row(r) * SR_HID + c4;
            sr_f4 g = *reinterpret_cast<const sr_f4 *>(s.d_h + o);
            if (!s.last) g += *reinterpret_cast<const sr_f4 *>(s.carry + o);
            const sr_f4 hp = *reinterpret_cast<const sr_f4 *>(s.h_prev + o) * s.masks[env_of(r)];
            float *gp = gates + (size_t)r * (4 * SR_HID) + c4;
            const sr_f4 rg = *reinterpret_cast<const sr_f4 *>(gp), zg = *reinterpret_cast<const sr_f4 *>(gp + SR_HID);
            const sr_f4 ng = *reinterpret_cast<const sr_f4 *>(gp + 2 * SR_HID), hn = *reinterpret_cast<const sr_f4 *>(gp + 3 * SR_HID);
            const sr_f4 dn = g * (1.0f - zg) * (1.0f - ng * ng);
            const sr_f4 dz = g * (hp - ng) * zg * (1.0f - zg);
            const sr_f4 dr = dn * hn * rg * (1.0f - rg);
            *reinterpret_cast<sr_f4 *>(gp) = dr;
            *reinterpret_cast<sr_f4 *>(gp + SR_HID) = dz;
            *reinterpret_cast<sr_f4 *>(gp + 2 * SR_HID) = dn;
            *reinterpret_cast<sr_f4 *>(gp + 3 * SR_HID) = dn * rg;
            *reinterpret_cast<sr_f4 *>(s.carry + o) = g * zg;
        }
    }
    __syncthreads();       // the workgroup's own global writes are visible to all its threads from here

    const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    sr_f4 ac[2][4], ae[2];
#pragma unroll
    for (int cbi = 0; cbi < 2; ++cbi)
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) ac[cbi][rb] = sr_f4{0.f, 0.f, 0.f, 0.f};
    ae[0] = ae[1] = sr_f4{0.f, 0.f, 0.f, 0.f};
    const int ecol = (wave & 3) * 16 + li;         // d_e: this wavefront's 16 columns of the embedding ...
    const int erb = (wave >> 2) * 2;               // ... and its two 16-row blocks

    for (int gate = 0; gate < 3; ++gate) {
        // ---- stage the gate's 256 columns of d_gi (fp32) and d_gh (planes 0, 1, 3 of the gradients); rows past the end are zero ----
        for (int idx = tid; idx < SR_TILE * (SR_HID / 4); idx += SR_EDGE_THREADS) {
            const int row = idx >> 6, c4 = (idx & 63) * 4;
            const long long r = r0 + row;
            sr_f4 vi = {0.f, 0.f, 0.f, 0.f}, vh = vi;
            if (r < nrows) {
                const float *gp = gates + (size_t)r * (4 * SR_HID) + c4;
                vi = *reinterpret_cast<const sr_f4 *>(gp + gate * SR_HID);
                vh = gate == 2 ? *reinterpret_cast<const sr_f4 *>(gp + 3 * SR_HID) : vi;
            }
            *reinterpret_cast<sr_f4 *>(&fi[row * SB_LDF + c4]) = vi;
            if (SPLIT) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const __bf16 hi = (__bf16)vh[q];
                    xh[row * SR_LDH + c4 + q] = hi;
                    xl[row * SR_LDH + c4 + q] = (__bf16)(vh[q] - (float)hi);
                }
            } else {
                *reinterpret_cast<sr_f4 *>(&fh[row * SB_LDF + c4]) = vh;
            }
        }
        __syncthreads();
        // ---- carry += d_gh[:, gate] . W_hh[gate rows, :] ----
#pragma unroll
        for (int cbi = 0; cbi < 2; ++cbi) {
            const int col = (wave * 2 + cbi) * 16 + li;
            if (SPLIT) {
#pragma unroll 2
                for (int ks = 0; ks < SR_HID / 32; ++ks) {
                    const int k0 = ks * 32 + lk * 8;
                    const size_t ob = (size_t)col * 768 + gate * SR_HID + k0;
                    const bf16x8 bh = *reinterpret_cast<const bf16x8 *>(w.hht_hi + ob);
                    const bf16x8 bl = *reinterpret_cast<const bf16x8 *>(w.hht_lo + ob);
#pragma unroll
                    for (int rb = 0; rb < 4; ++rb) {
                        const int o = (rb * 16 + li) * SR_LDH + k0;
                        const bf16x8 a_hi = *reinterpret_cast<const bf16x8 *>(&xh[o]);
                        const bf16x8 a_lo = *reinterpret_cast<const bf16x8 *>(&xl[o]);
                        ac[cbi][rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo, bh, ac[cbi][rb], 0, 0, 0);
                        ac[cbi][rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, bl, ac[cbi][rb], 0, 0, 0);
                        ac[cbi][rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, bh, ac[cbi][rb], 0, 0, 0);
                    }
                }
            } else {
#pragma unroll 4
                for (int ks = 0; ks < SR_HID / 4; ++ks) {
                    const int k0 = ks * 4 + lk;
                    const float b = w.w_hh[(size_t)(gate * SR_HID + k0) * SR_HID + col];
#pragma unroll
                    for (int rb = 0; rb < 4; ++rb)
                        ac[cbi][rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(fh[(rb * 16 + li) * SB_LDF + k0], b, ac[cbi][rb], 0, 0, 0);
                }
            }
        }
        // ---- d_e += d_gi[:, gate] . W_ih[gate rows, :], exact fp32 ----
#pragma unroll 4
        for (int ks = 0; ks < SR_HID / 4; ++ks) {
            const int k0 = ks * 4 + lk;
            const float b = w.w_ih[(size_t)(gate * SR_HID + k0) * SR_EMB + ecol];
#pragma unroll
            for (int q = 0; q < 2; ++q) ae[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(fi[((erb + q) * 16 + li) * SB_LDF + k0], b, ae[q], 0, 0, 0);
        }
        __syncthreads();
    }
    // ---- epilogue; C/D layout: column = lane & 15, row = 4 * (lane >> 4) + i ----
#pragma unroll
    for (int cbi = 0; cbi < 2; ++cbi) {
        const int col = (wave * 2 + cbi) * 16 + li;
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long long r = r0 + rb * 16 + lk * 4 + i;
                if (r < nrows) {
                    const size_t o = (size_t)edge_row(r) * SR_HID + col;
                    s.carry_out[o] = s.masks[env_of(r)] * (s.carry[o] + ac[cbi][rb][i]);
                }
            }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long r = r0 + (erb + q) * 16 + lk * 4 + i;
            if (r < nrows) {
                const size_t o = (size_t)r * SR_EMB + ecol;
                de[o] = emb[o] > 0.0f ? ae[q][i] : 0.0f;
            }
        }
}

// ---- weight gradients ----
constexpr int SW_ROWS = 32;             // rows per staged tile
constexpr int SW_THREADS = 512;         // 8 wavefronts: 16 output rows (columns of D) each, all KB 16-wide blocks of A's columns

enum { SW_A_HP = 0, SW_A_PLAIN = 1 };

struct SrnnWgradArgs {
    const float *D;                     // [M, ldd]: the gradients of one weight set, rows in (t, row of the set) order
    int ldd, ncols;                     // ncols: output rows = slices of 128 columns of D; slice s starts at column s * 128 (+ skip when s >= 4)
    int skip;                           // dW_hh reads planes 0, 1, 3 of [dr, dz, dn, dn r]: skip = 256
    int M, rows_per_chunk;              // the range of chunk c is [c * rows_per_chunk, min(M, (c + 1) * rows_per_chunk))
    const float *A;                     // SW_A_PLAIN: [M, lda]; column ka of the operand is 1 (the bias gradient), columns above it 0
    int lda, ka;
    const float *h_all, *edge_h0, *masks;   // SW_A_HP: A = mask_t * h_{t-1}, gathered from h_all [T, N * (H+1), 256] (edge_h0 at t = 0)
    int N, H, is_t, rows_set;           // rows_set = N or N * H: row m is step m / rows_set, row m % rows_set of the set
    float *P;                           // partials [chunks, ncols, KB * 16]
};

// P[chunk][n][k] = sum over the chunk's rows m of D[m][col(n)] * A[m][k], rows in order, on v_mfma_f32_16x16x4_f32 (the four rows of a k-step
// are the MFMA's K).  The A tile is staged in LDS and shared by the eight wavefronts; D goes from global memory straight into A fragments.
template <int KB, int AMODE>
__global__ __launch_bounds__(SW_THREADS) void srnn_wgrad_kernel(SrnnWgradArgs a)
{
    constexpr int LDA = KB * 16 + 4;
    __shared__ __attribute__((aligned(16))) float As[SW_ROWS * LDA];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int slice = blockIdx.x, chunk = blockIdx.y;
    const int n0 = slice * 128 + wave * 16;                        // this wavefront's first output row
    const bool live = n0 < a.ncols;                                // ncols % 16 == 0
    const int dcol = n0 + (slice >= 4 ? a.skip : 0) + li;
    const int m_begin = chunk * a.rows_per_chunk;
    const int m_end = min(a.M, m_begin + a.rows_per_chunk);
    sr_f4 acc[KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) acc[kb] = sr_f4{0.f, 0.f, 0.f, 0.f};
    for (int m0 = m_begin; m0 < m_end; m0 += SW_ROWS) {
        float dv[SW_ROWS / 4];
#pragma unroll
        for (int q = 0; q < SW_ROWS / 4; ++q) {
            const int m = m0 + q * 4 + lk;
            dv[q] = (live && m < m_end) ? a.D[(size_t)m * a.ldd + dcol] : 0.0f;
        }
        if (AMODE == SW_A_HP) {
            for (int idx = tid; idx < SW_ROWS * (SR_HID / 4); idx += SW_THREADS) {
                const int row = idx >> 6, c4 = (idx & 63) * 4;
                const int m = m0 + row;
                sr_f4 v = {0.f, 0.f, 0.f, 0.f};
                if (m < m_end) {
                    const int t = m / a.rows_set, r = m % a.rows_set;
                    const int env = a.is_t ? r : r / a.H;
                    const size_t srow = a.is_t ? (size_t)r * (a.H + 1) : (size_t)env * (a.H + 1) + 1 + r % a.H;
                    const float *hp = t == 0 ? a.edge_h0 : a.h_all + (size_t)(t - 1) * a.N * (a.H + 1) * SR_HID;
                    v = *reinterpret_cast<const sr_f4 *>(hp + srow * SR_HID + c4) * a.masks[(size_t)t * a.N + env];
                }
                *reinterpret_cast<sr_f4 *>(&As[row * LDA + c4]) = v;
            }
        } else {
            for (int idx = tid; idx < SW_ROWS * KB * 16; idx += SW_THREADS) {
                const int row = idx / (KB * 16), k = idx % (KB * 16);
                const int m = m0 + row;
                float v = 0.0f;
                if (m < m_end) v = k < a.ka ? a.A[(size_t)m * a.lda + k] : (k == a.ka ? 1.0f : 0.0f);
                As[row * LDA + k] = v;
            }
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int q = 0; q < SW_ROWS / 4; ++q)
#pragma unroll
                for (int kb = 0; kb < KB; ++kb)
                    acc[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[q], As[(q * 4 + lk) * LDA + kb * 16 + li], acc[kb], 0, 0, 0);
        }
        __syncthreads();
    }
    if (live) {
        float *P = a.P + (size_t)chunk * a.ncols * (KB * 16);
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i) P[(size_t)(n0 + lk * 4 + i) * (KB * 16) + kb * 16 + li] = acc[kb][i];
    }
}

// dst[row][col] (row-major, `cols` wide, n elements) = sum over the chunks, in order, of P[chunk][row + (row >= row_split ? row_add : 0)][col_off + col]
__global__ void srnn_reduce_kernel(int n, int cols, float *__restrict__ dst, const float *__restrict__ P, int chunks, size_t chunk_stride, int ldp,
                                   int col_off, int row_split, int row_add)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int row = i / cols;
    const int col = i % cols;
    if (row >= row_split) row += row_add;
    const float *src = P + (size_t)row * ldp + col_off + col;
    float v = 0.0f;
    for (int c = 0; c < chunks; ++c) v += src[(size_t)c * chunk_stride];
    dst[i] = v;
}

} // namespace
