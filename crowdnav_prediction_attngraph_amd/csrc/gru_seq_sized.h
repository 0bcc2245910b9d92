// gru_seq_sized.h -- the GRU sequence of the PPO update at a hidden size R other than 128 (cn_gru_seq_fwd_sized / cn_gru_seq_bwd_sized; R = 128
// keeps gru_seq_fwd_kernel / gru_seq_bwd_kernel of linear.hip, bit for bit).  Part of linear.hip's translation unit (split8, sigmoidf_, f32x4g).
//
// Same division of labour as the R = 128 kernels: a workgroup of four wavefronts owns GR = 16 rows (envs) for the whole sequence, wavefront w
// owns the hidden units (R/4) w .. (R/4) (w+1) - 1 as NA = R/64 blocks of 16, the r, z, n accumulators of one (row, unit) sit in the same lane
// and register index, one barrier per step forward (two backward, as at R = 128: the d(gh) planes are written, read by everyone, overwritten).
// What differs is where W_hh lives.  A wavefront's slice as bf16 hi / lo MFMA fragments is 3 R^2 / 256 VGPRs per lane: 48 at R = 64, 432 at
// R = 192, 768 at R = 256 -- against a 512-entry file that also holds the accumulators and the prefetched step inputs.  So:
//   * STREAM = false (R = 64): the slice is loaded once and stays in registers.
//   * STREAM = true (R = 192, 256): every step re-reads the slice from a PRE-SPLIT fragment image (gru_image_kernel below; 12 R^2 bytes, L2
//     resident: every workgroup of the launch reads the same image every step), one k-step's fragments per trip into the register set the
//     previous k-step has just released, so the loads of k-step kk+1 travel behind the MFMAs of k-step kk; the last k-step of a step already
//     requests k-step 0 of the next one, which then crosses the cell's pointwise part and the barrier.
// Both forms read the image, so the arithmetic (operands, MFMA order, summation order) is one code path.  The previous state of the cell's
// z * h term stays in the lane that computed it (registers), so the only LDS is the two bf16 planes of the A operand.
// Image layouts (elements of 8 bf16 = one lane's fragment; a wavefront's fragment is one contiguous 1 KB read):
//   forward : [wave][kk < R/32][gate j][block a][plane hi|lo][lane][8]   element = W_hh[j R + u][32 kk + 8 kg + e],  u = (R/4) wave + 16 a + l15
//   backward: [wave][kk < 3R/32][block a][plane hi|lo][lane][8]          element = W_hh[32 kk + 8 kg + e][u]
#pragma once

namespace {

__global__ __launch_bounds__(256) void gru_image_kernel(int R, int backward, const float *__restrict__ Whh, __bf16 *__restrict__ img)
{
    const int NA = R / 64, KK = backward ? 3 * R / 32 : R / 32, G = backward ? 1 : 3;
    const int frags = 4 * KK * G * NA; // (wave, kk, j, a)
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= frags * 64 * 8) return;
    const int e = idx & 7, lane = (idx >> 3) & 63, f = idx >> 9;
    const int a = f % NA, j = (f / NA) % G, kk = (f / (NA * G)) % KK, wave = f / (NA * G * KK);
    const int kg = lane >> 4, l15 = lane & 15, u = (R / 4) * wave + 16 * a + l15, k = 32 * kk + 8 * kg + e;
    const float x = backward ? Whh[(size_t)k * R + u] : Whh[(size_t)(j * R + u) * R + k];
    const __bf16 h = (__bf16)x;
    const size_t o = ((size_t)(2 * f) * 64 + lane) * 8 + e;
    img[o] = h;
    img[o + 512] = (__bf16)(x - (float)h);
}

template <int R, bool STREAM>
__global__ __launch_bounds__(256) void gru_seq_fwd_sized_kernel(int T, int N, const float *__restrict__ gi, const float *__restrict__ h0,
                                                                const float *__restrict__ m, const __bf16 *__restrict__ img, const float *__restrict__ bhh,
                                                                float *__restrict__ hs, float *__restrict__ hms, float *__restrict__ gates)
{
    constexpr int NA = R / 64, KK = R / 32, UW = R / 4, PS = R + 8; // blocks per wavefront, k-steps, units per wavefront, plane row stride (bf16)
    constexpr int NSET = STREAM ? 2 : KK;
    __shared__ __attribute__((aligned(16))) __bf16 hmh[2][GR * PS], hml[2][GR * PS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kg = lane >> 4, l15 = lane & 15;
    const int row0 = blockIdx.x * GR;
    bf16x8 wf[NSET][3][NA][2];
    int opaque = 0; // keeps the (step-invariant) image loads of the streamed form inside the time loop
    auto load_w = [&](int set, int kk) {
        const __bf16 *p = img + ((size_t)((wave * KK + kk) * 3 * NA * 2) * 64 + lane) * 8 + opaque;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                wf[set][j][a][0] = *reinterpret_cast<const bf16x8 *>(p + (size_t)((j * NA + a) * 2) * 512);
                wf[set][j][a][1] = *reinterpret_cast<const bf16x8 *>(p + (size_t)((j * NA + a) * 2 + 1) * 512);
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
        const __bf16 h = (__bf16)v;
        hmh[0][r * PS + c] = h; hml[0][r * PS + c] = (__bf16)(v - (float)h);
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
    // a step's inputs are requested one step ahead, unpredicated (surplus rows of the last workgroup read row N-1), as at R = 128
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
            // term-major inside a k-step: consecutive MFMAs write different accumulators
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
                if (t + 1 < T) {
                    const __bf16 h = (__bf16)next;
                    hmh[cur ^ 1][rl * PS + u] = h; hml[cur ^ 1][rl * PS + u] = (__bf16)(next - (float)h);
                }
            }
        // (mk[r] is shared by the blocks of a row: the reloads go behind the last block's use)
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) request(a, r, t + 1);
        __syncthreads();
    }
}

template <int R, bool STREAM>
__global__ __launch_bounds__(256) void gru_seq_bwd_sized_kernel(int T, int N, const float *__restrict__ gates, const float *__restrict__ hms,
                                                                const float *__restrict__ m, const __bf16 *__restrict__ img, const float *__restrict__ d_hs,
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
        const __bf16 *p = img + ((size_t)((wave * KK + kk) * NA * 2) * 64 + lane) * 8 + opaque;
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            wf[set][a][0] = *reinterpret_cast<const bf16x8 *>(p + (size_t)(a * 2) * 512);
            wf[set][a][1] = *reinterpret_cast<const bf16x8 *>(p + (size_t)(a * 2 + 1) * 512);
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
    // the saved gates / states / incoming gradients of a step are requested one step ahead, unpredicated (surplus rows read row N-1)
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
    auto put = [&](int off, float v) { const __bf16 h = (__bf16)v; dgp_h[off] = h; dgp_l[off] = (__bf16)(v - (float)h); };
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
                const float din = d * (1.0f - zg) * (1.0f - ng * ng);
                const float dr = ok ? din * hn * rg * (1.0f - rg) : 0.0f;
                const float dz = ok ? d * (h - ng) * zg * (1.0f - zg) : 0.0f;
                const float dn = ok ? din * rg : 0.0f;
                direct[a][r] = ok ? d * zg : 0.0f;
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
        // one accumulator per term and column block
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
