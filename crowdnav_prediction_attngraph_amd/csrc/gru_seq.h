// gru_seq.h -- the human-node GRU of the PPO update over a whole sequence: one launch forward, one backward (cn_gru_seq_fwd / _bwd and their
// _sized forms in linear.hip), for a hidden size R in {64, 128, 192, 256}.  torch.nn.GRU gate order r, z, n; rl/networks/srnn_model.py:35-105 runs
// the cell per time step with the hidden state multiplied by the done mask first: gi = x W_ih^T + b_ih (given), gh = hm W_hh^T + b_hh.
//
// The update runs the GRU over T = 30 steps with only N x R of state: as separate launches (a product and a pointwise kernel per step and
// direction) it is launch- and latency-bound.  Here a workgroup of four wavefronts owns GR = 16 rows (envs) for the whole sequence (2048 envs of a
// minibatch = 128 workgroups; with 32 rows it was 64 of 256 CUs) and wavefront w owns the hidden units (R/4) w .. (R/4) (w+1) - 1 as NA = R/64
// blocks of 16:
//   * forward: 3 NA column blocks (gate j, block a) per wavefront.  Per step the masked state hm (16 x R, LDS, double buffered as bf16 hi / lo
//     planes written by the lane that computed the value) is the A operand of the split-precision MFMAs (v_mfma_f32_16x16x32_bf16: lo*hi, hi*lo,
//     hi*hi per column block and k-step, term-major so that consecutive MFMAs write different accumulators); the accumulators of the r, z, n gates
//     of one (row, unit) sit in the same lane and register index, so the cell's pointwise part needs no exchange at all, and the previous state of
//     its z * h term stays in the lane that computed it; one barrier per step.  The forward keeps (r, z, n, gh_n) for the backward.
//   * backward (reverse time): the same wavefront computes d(gates) for its units from the saved (r, z, n, gh_n), publishes d(gh) [16 x 3R] as
//     hi / lo planes in LDS (written, read by everyone, overwritten: two barriers per step), and multiplies it with its 3R x R/4 slice of W_hh to
//     get d(hm) -- one accumulator per term and column block: the MFMAs of a step into NA accumulators would each wait for the one before; the
//     carried gradient stays in registers in the accumulator layout.  d(W_hh) is one product over all T*N rows afterwards.
// What depends on R is where W_hh lives.  A wavefront's slice as bf16 hi / lo MFMA fragments is 3 R^2 / 256 VGPRs per lane: 48 at R = 64, 192 at
// R = 128, 432 at R = 192, 768 at R = 256 -- against a 512-entry file that also holds the accumulators and the prefetched step inputs.  So:
//   * STREAM = false (R = 64, 128): the slice is read once from the fp32 W_hh, split in registers (split8) and stays there.  W = W_hh.
//   * STREAM = true (R = 192, 256): every step re-reads the slice from a PRE-SPLIT fragment image (gru_image_kernel; 12 R^2 bytes, L2 resident:
//     every workgroup of the launch reads the same image every step), one k-step's fragments per trip into the register set the previous k-step
//     has just released, so the loads of k-step kk+1 travel behind the MFMAs of k-step kk; the last k-step of a step already requests k-step 0
//     of the next one, which then crosses the cell's pointwise part and the barrier.  W = the image.
// The split is the same expression in both (split1), so operands, MFMA order and summation order are one code path for every R.
// Image layouts (elements of 8 bf16 = one lane's fragment; a wavefront's fragment is one contiguous 1 KB read):
//   forward : [wave][kk < R/32][gate j][block a][plane hi|lo][lane][8]   element = W_hh[j R + u][32 kk + 8 kg + e],  u = (R/4) wave + 16 a + l15
//   backward: [wave][kk < 3R/32][block a][plane hi|lo][lane][8]          element = W_hh[32 kk + 8 kg + e][u]
// Accumulator layout of the 16 x 16 MFMA: lane (l15 = lane & 15, kg = lane >> 4) holds rows 4 kg + r (r = 0..3) of column l15.
// Operand layout of v_mfma_f32_16x16x32_bf16: lane (l15, kg) supplies 8 consecutive k = 32 kk + 8 kg + e of row / column l15.
#pragma once
#include <hip/hip_runtime.h>
#include "split_bf16.h"

namespace {

constexpr int GR = 16; // rows per workgroup.  The LDS planes' row strides are R + 8 / 3R + 8 bf16: 16 bytes past a multiple of 128, so the 16-byte
                       // fragment reads of 16 rows tile all banks
typedef float f32x4g __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ void split1(float x, __bf16 &hi, __bf16 &lo) { const __bf16 h = (__bf16)x; hi = h; lo = (__bf16)(x - (float)h); }
__device__ __forceinline__ void split8(const float (&x)[8], bf16x8 &hi, bf16x8 &lo)
{
#pragma unroll
    for (int e = 0; e < 8; ++e) { __bf16 h, l; split1(x[e], h, l); hi[e] = h; lo[e] = l; }
}

__global__ __launch_bounds__(256) void gru_image_kernel(int R, int backward, const float *__restrict__ Whh, __bf16 *__restrict__ img)
{
    const int NA = R / 64, KK = backward ? 3 * R / 32 : R / 32, G = backward ? 1 : 3;
    const int frags = 4 * KK * G * NA; // (wave, kk, j, a)
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= frags * 64 * 8) return;
    const int e = idx & 7, lane = (idx >> 3) & 63, f = idx >> 9;
    const int a = f % NA, j = (f / NA) % G, kk = (f / (NA * G)) % KK, wave = f / (NA * G * KK);
    const int kg = lane >> 4, l15 = lane & 15, u = (R / 4) * wave + 16 * a + l15, k = 32 * kk + 8 * kg + e;
    const size_t o = ((size_t)(2 * f) * 64 + lane) * 8 + e;
    split1(backward ? Whh[(size_t)k * R + u] : Whh[(size_t)(j * R + u) * R + k], img[o], img[o + 512]);
}

// W: the fp32 W_hh [3R, R] (STREAM = false) or its forward fragment image (STREAM = true)
template <int R, bool STREAM>
__global__ __launch_bounds__(256) void gru_seq_fwd_kernel(int T, int N, const float *__restrict__ gi, const float *__restrict__ h0,
                                                          const float *__restrict__ m, const void *__restrict__ W, const float *__restrict__ bhh,
                                                          float *__restrict__ hs, float *__restrict__ hms, float *__restrict__ gates)
{
    constexpr int NA = R / 64, KK = R / 32, UW = R / 4, PS = R + 8; // blocks per wavefront, k-steps, units per wavefront, plane row stride (bf16)
    constexpr int NSET = STREAM ? 2 : KK;
    __shared__ __attribute__((aligned(16))) __bf16 hmh[2][GR * PS], hml[2][GR * PS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kg = lane >> 4, l15 = lane & 15;
    const int row0 = blockIdx.x * GR;
    // B fragments: column = unit u(a) = UW wave + 16 a + l15 of gate j, k = 32 kk + 8 kg + e
    bf16x8 wf[NSET][3][NA][2];
    int opaque = 0; // keeps the (step-invariant) image loads of the streamed form inside the time loop
    auto load_w = [&](int set, int kk) {
        const __bf16 *p = static_cast<const __bf16 *>(W) + ((size_t)((wave * KK + kk) * 3 * NA * 2) * 64 + lane) * 8 + opaque; // streamed: this k-step's fragments
        const float *wr = static_cast<const float *>(W) + (size_t)(UW * wave + l15) * R + 32 * kk + 8 * kg;                   // resident: this lane's k of unit u(0)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                if (STREAM) {
                    wf[set][j][a][0] = *reinterpret_cast<const bf16x8 *>(p + (size_t)((j * NA + a) * 2) * 512);
                    wf[set][j][a][1] = *reinterpret_cast<const bf16x8 *>(p + (size_t)((j * NA + a) * 2 + 1) * 512);
                } else {
                    float x[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) x[e] = wr[(size_t)(j * R + 16 * a) * R + e];
                    split8(x, wf[set][j][a][0], wf[set][j][a][1]);
                }
            }
    };
    if (STREAM) load_w(0, 0);
    else {
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) load_w(kk, kk);
    }
    float bias[3][NA];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int a = 0; a < NA; ++a) bias[j][a] = bhh[j * R + UW * wave + 16 * a + l15];
    for (int i = tid; i < GR * R; i += 256) {
        const int r = i / R, c = i % R, row = row0 + r;
        const float v = row < N ? h0[(size_t)row * R + c] * m[row] : 0.0f;
        split1(v, hmh[0][r * PS + c], hml[0][r * PS + c]);
        if (row < N) hms[(size_t)row * R + c] = v;
    }
    float hprev[NA][4]; // the masked previous state of this lane's cells (what the LDS planes hold, unsplit)
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 4 * kg + r, rowc = min(row, N - 1);
            const float v = h0[(size_t)rowc * R + UW * wave + 16 * a + l15] * m[rowc];
            hprev[a][r] = row < N ? v : 0.0f;
        }
    __syncthreads();
    // A step's inputs (gi of the step, the mask of the next) do not depend on the state: they are requested one step ahead, right after the
    // cells have used the current ones, unpredicated (surplus rows of the last workgroup read row N-1) -- a whole step hides the round trip.
    // Loaded inside the per-row `if (row < N)` blocks below, every row paid its own memory round trip.
    float gir[NA][4], giz[NA][4], gin[NA][4], mk[4];
    auto request = [&](int a, int r, int t) {
        const int rowc = min(row0 + 4 * kg + r, N - 1);
        const float *gip = gi + ((size_t)min(t, T - 1) * N + rowc) * (3 * R) + UW * wave + 16 * a + l15;
        gir[a][r] = gip[0]; giz[a][r] = gip[R]; gin[a][r] = gip[2 * R];
        if (a == 0) mk[r] = m[(size_t)min(t + 1, T - 1) * N + rowc];
    };
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) request(a, r, 0);
    for (int t = 0; t < T; ++t) {
        const int cur = t & 1;
        if (STREAM) asm volatile("" : "+s"(opaque));
        f32x4g acc[3][NA];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int a = 0; a < NA; ++a) acc[j][a] = f32x4g{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            const int set = STREAM ? (kk & 1) : kk;
            if (STREAM) load_w((kk + 1) & 1, (kk + 1) % KK); // the other set is free since the previous k-step (KK is even)
            const bf16x8 ah = *reinterpret_cast<const bf16x8 *>(&hmh[cur][l15 * PS + 32 * kk + 8 * kg]);
            const bf16x8 al = *reinterpret_cast<const bf16x8 *>(&hml[cur][l15 * PS + 32 * kk + 8 * kg]);
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int a = 0; a < NA; ++a) acc[j][a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, wf[set][j][a][0], acc[j][a], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int a = 0; a < NA; ++a) acc[j][a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wf[set][j][a][1], acc[j][a], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int a = 0; a < NA; ++a) acc[j][a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wf[set][j][a][0], acc[j][a], 0, 0, 0);
        }
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rl = 4 * kg + r, row = row0 + rl, u = UW * wave + 16 * a + l15;
                const float hn = acc[2][a][r] + bias[2][a];
                const float rg = sigmoidf_(gir[a][r] + acc[0][a][r] + bias[0][a]);
                const float zg = sigmoidf_(giz[a][r] + acc[1][a][r] + bias[1][a]);
                const float ng = tanhf(gin[a][r] + rg * hn);
                const float hnew = (1.0f - zg) * ng + zg * hprev[a][r];
                const float next = row < N ? hnew * mk[r] : 0.0f;
                if (row < N) { // stores only: nothing in here waits for memory
                    const size_t tr = (size_t)t * N + row;
                    hs[tr * R + u] = hnew;
                    float *gp = gates + tr * (4 * R);
                    gp[u] = rg; gp[R + u] = zg; gp[2 * R + u] = ng; gp[3 * R + u] = hn;
                    if (t + 1 < T) hms[(tr + N) * R + u] = next;
                }
                hprev[a][r] = next;
                if (t + 1 < T) split1(next, hmh[cur ^ 1][rl * PS + u], hml[cur ^ 1][rl * PS + u]);
            }
        // (mk[r] is shared by the blocks of a row: the reloads go behind the last block's use)
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) request(a, r, t + 1);
        __syncthreads();
    }
}

// W: the fp32 W_hh [3R, R] (STREAM = false) or its backward fragment image (STREAM = true)
template <int R, bool STREAM>
__global__ __launch_bounds__(256) void gru_seq_bwd_kernel(int T, int N, const float *__restrict__ gates, const float *__restrict__ hms,
                                                          const float *__restrict__ m, const void *__restrict__ W, const float *__restrict__ d_hs,
                                                          float *__restrict__ dgi, float *__restrict__ dgh, float *__restrict__ dh0)
{
    constexpr int NA = R / 64, KK = 3 * R / 32, UW = R / 4, QS = 3 * R + 8; // k-steps over the 3R gate columns; row stride (bf16) of the d(gh) planes
    constexpr int NSET = STREAM ? 2 : KK;
    __shared__ __attribute__((aligned(16))) __bf16 dgp_h[GR * QS], dgp_l[GR * QS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kg = lane >> 4, l15 = lane & 15;
    const int row0 = blockIdx.x * GR;
    // d(hm)[row][n] = sum_c d(gh)[row][c] * W_hh[c][n]: this lane's columns n = u(a), k = c = 32 kk + 8 kg + e
    bf16x8 wf[NSET][NA][2];
    int opaque = 0;
    auto load_w = [&](int set, int kk) {
        const __bf16 *p = static_cast<const __bf16 *>(W) + ((size_t)((wave * KK + kk) * NA * 2) * 64 + lane) * 8 + opaque;
        const float *wc = static_cast<const float *>(W) + (size_t)(32 * kk + 8 * kg) * R + UW * wave + l15;
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            if (STREAM) {
                wf[set][a][0] = *reinterpret_cast<const bf16x8 *>(p + (size_t)(a * 2) * 512);
                wf[set][a][1] = *reinterpret_cast<const bf16x8 *>(p + (size_t)(a * 2 + 1) * 512);
            } else {
                float x[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = wc[(size_t)e * R + 16 * a];
                split8(x, wf[set][a][0], wf[set][a][1]);
            }
        }
    };
    if (!STREAM) {
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) load_w(kk, kk);
    }
    float carry[NA][4];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) carry[a][r] = 0.0f;
    // The saved gates / states / incoming gradients of a step do not depend on the carried gradient: they are requested one step ahead,
    // unpredicated (surplus rows read row N-1), right behind the barrier that ends their last use -- the MFMAs of the current step hide the
    // round trip.
    float s_rg[NA][4], s_zg[NA][4], s_ng[NA][4], s_hn[NA][4], s_h[NA][4], s_d[NA][4], s_m[4];
    auto preload = [&](int t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rowc = min(row0 + 4 * kg + r, N - 1);
            const size_t tr = (size_t)t * N + rowc;
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                const int u = UW * wave + 16 * a + l15;
                const float *gp = gates + tr * (4 * R) + u;
                s_rg[a][r] = gp[0]; s_zg[a][r] = gp[R]; s_ng[a][r] = gp[2 * R]; s_hn[a][r] = gp[3 * R];
                s_h[a][r] = hms[tr * R + u];
                s_d[a][r] = d_hs[tr * R + u];
            }
            s_m[r] = m[tr];
        }
    };
    auto put = [&](int off, float v) { split1(v, dgp_h[off], dgp_l[off]); };
    preload(T - 1);
    for (int t = T - 1; t >= 0; --t) {
        if (STREAM) { asm volatile("" : "+s"(opaque)); load_w(0, 0); }
        float direct[NA][4], mt[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rl = 4 * kg + r, row = row0 + rl;
            const bool ok = row < N;
            mt[r] = s_m[r];
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                const int u = UW * wave + 16 * a + l15;
                const float rg = s_rg[a][r], zg = s_zg[a][r], ng = s_ng[a][r], hn = s_hn[a][r], h = s_h[a][r];
                const float d = s_d[a][r] + carry[a][r];
                const float din = d * (1.0f - zg) * (1.0f - ng * ng); // d(i_n)
                const float dr = ok ? din * hn * rg * (1.0f - rg) : 0.0f; // d(i_r) = d(h_r)
                const float dz = ok ? d * (h - ng) * zg * (1.0f - zg) : 0.0f; // d(i_z) = d(h_z)
                const float dn = ok ? din * rg : 0.0f;
                direct[a][r] = ok ? d * zg : 0.0f; // the direct path d(hm) = dh' * z
                if (ok) { // stores only
                    const size_t tr = (size_t)t * N + row;
                    float *p1 = dgi + tr * (3 * R), *p2 = dgh + tr * (3 * R);
                    p1[u] = dr; p1[R + u] = dz; p1[2 * R + u] = din;
                    p2[u] = dr; p2[R + u] = dz; p2[2 * R + u] = dn;
                }
                put(rl * QS + u, dr); put(rl * QS + R + u, dz); put(rl * QS + 2 * R + u, dn);
            }
        }
        __syncthreads();
        preload(t > 0 ? t - 1 : 0);
        f32x4g acc[3][NA];
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int a = 0; a < NA; ++a) acc[q][a] = f32x4g{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            const int set = STREAM ? (kk & 1) : kk;
            if (STREAM && kk + 1 < KK) load_w((kk + 1) & 1, kk + 1);
            const bf16x8 ah = *reinterpret_cast<const bf16x8 *>(&dgp_h[l15 * QS + 32 * kk + 8 * kg]);
            const bf16x8 al = *reinterpret_cast<const bf16x8 *>(&dgp_l[l15 * QS + 32 * kk + 8 * kg]);
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                acc[0][a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, wf[set][a][0], acc[0][a], 0, 0, 0);
                acc[1][a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wf[set][a][1], acc[1][a], 0, 0, 0);
                acc[2][a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wf[set][a][0], acc[2][a], 0, 0, 0);
            }
        }
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + 4 * kg + r;
                carry[a][r] = row < N ? (direct[a][r] + ((acc[0][a][r] + acc[1][a][r]) + acc[2][a][r])) * mt[r] : 0.0f;
            }
        __syncthreads(); // the next (earlier) step overwrites the planes
    }
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 4 * kg + r;
            if (row < N) dh0[(size_t)row * R + UW * wave + 16 * a + l15] = carry[a][r];
        }
}

} // namespace
