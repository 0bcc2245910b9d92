// gemm3_tn.h -- the PPO update's weight gradients in the split-precision ("bf16x3", split_bf16.h) arithmetic: the TN products
// P[s][n][k] = sum_{m in split s} dY[m][n] X[m][k] over row splits -- gemm3_tn_kernel (two barriers per K tile: small products and
// row tails) and gemm3p_tn_kernel (pipelined: whole 128-column tiles over >= 32768 rows) -- and the fixed-order reduction of their
// partials.  Only linear.hip includes it (cn_linear_wgrad).
#pragma once
#include "common.h"
#include "gemm.h"
#include "split_bf16.h"

namespace {

// K tile of gemm3_tn_kernel (large stand-alone products, where occupancy beats tile depth -- see the measurements in gemm3.h): 16 = ONE
// MFMA k-step, 24.6 KB of LDS and <= 128 VGPRs -> four workgroups per CU (three with the ReLU gate).  LDS rows are the K tile + 8 bf16 of pad.
constexpr int TN_BK = 16;
constexpr int TN_STRIDE = TN_BK + 8;

// Weight-gradient GEMM (TN): P[s][n][k] = sum_{m in split s} dY[m][n] * X[m][k], both operands fp32 activations with the
// reduction index m as the SLOW axis in memory.  The MFMA wants 8 consecutive reduction elements per lane, so the tiles
// are transposed on their way into LDS: thread (column c, group g) loads 8 rows m of its column with 8 coalesced dword
// loads (64 lanes = 256 contiguous bytes each), splits them into bf16 hi/lo and writes ONE 16-byte LDS word per plane
// at [c][8g .. 8g+7].  Consecutive lanes hit rows 144 B apart -> conflict-free ds_write_b128, and the LDS image is
// exactly that of gemm3_nt_kernel (gemm3.h), so the MFMA section reads the same.  The m range is cut into `gridDim.z` splits (partials summed
// by reduce_partials_kernel in a fixed order: deterministic).  Blocks of k tile 0 also produce the column sums of dY
// (the bias gradient) from the registers they stage anyway.
template <bool GATE>
__global__ __launch_bounds__(256, GATE ? 3 : 4) void gemm3_tn_kernel(int M, int N, int K, const float *__restrict__ dY, int ldy, const float *__restrict__ Ygate,
                                                       const float *__restrict__ X, int ldx, int rows_per_split, float *__restrict__ partials,
                                                       float *__restrict__ db_part)
{
    constexpr int BN = 128;
    constexpr int NB = BN / 64;
    extern __shared__ __attribute__((aligned(16))) char smem3[];
    __bf16 *Ah = reinterpret_cast<__bf16 *>(smem3);
    __bf16 *Al = Ah + BM * TN_STRIDE;
    __bf16 *Wh = Al + BM * TN_STRIDE;
    __bf16 *Wl = Wh + BN * TN_STRIDE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int n_blk = blockIdx.x * BM, k_blk = blockIdx.y * BN, split = blockIdx.z;
    const int m_begin = split * rows_per_split;
    const int m_end = min(M, m_begin + rows_per_split);
    const int c = tid & 127, g0 = tid >> 7;
    const bool n_ok = n_blk + c < N; // N may end inside the tile (64-wide layers): the surplus columns stay zero
    const bool k_ok = k_blk + c < K; // and so may K (a multiple of 64): the surplus X columns are zero and their products are not stored
    const bool want_db = db_part != nullptr && blockIdx.y == 0;

    f32x16 acc[2][NB];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    constexpr int TG = TN_BK / 16; // 8-row groups per thread per chunk (2 thread halves x TG groups x 8 rows = TN_BK rows)
    float pa[TG][8], pb[TG][8], pg[GATE ? TG : 1][8];
    const float *a_col = dY + n_blk + c, *b_col = X + k_blk + c;
    const float *g_col = GATE ? Ygate + n_blk + c : nullptr; // backward through a ReLU: dY gated by the forward output
    auto load_chunk = [&](int m0) {
#pragma unroll
        for (int p = 0; p < TG; ++p)
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int m = m0 + (g0 + 2 * p) * 8 + u;
                const bool ok = m < m_end;
                pa[p][u] = ok && n_ok ? a_col[(size_t)m * ldy] : 0.0f;
                if (GATE) pg[p][u] = ok && n_ok ? g_col[(size_t)m * ldy] : 0.0f; // raw load; the select happens in store_chunk
                pb[p][u] = ok && k_ok ? b_col[(size_t)m * ldx] : 0.0f;
            }
    };
    float colsum = 0.0f;
    auto store_chunk = [&]() {
#pragma unroll
        for (int p = 0; p < TG; ++p) {
            bf16x8 ahi, alo, bhi, blo;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (GATE) pa[p][u] = pg[GATE ? p : 0][u] > 0.0f ? pa[p][u] : 0.0f;
                ahi[u] = (__bf16)pa[p][u];
                alo[u] = (__bf16)(pa[p][u] - (float)ahi[u]);
                bhi[u] = (__bf16)pb[p][u];
                blo[u] = (__bf16)(pb[p][u] - (float)bhi[u]);
                colsum += pa[p][u];
            }
            const int o = c * TN_STRIDE + (g0 + 2 * p) * 8;
            *reinterpret_cast<bf16x8 *>(&Ah[o]) = ahi;
            *reinterpret_cast<bf16x8 *>(&Al[o]) = alo;
            *reinterpret_cast<bf16x8 *>(&Wh[o]) = bhi;
            *reinterpret_cast<bf16x8 *>(&Wl[o]) = blo;
        }
    };

    load_chunk(m_begin);
    const int half = lane >> 5, l31 = lane & 31;
    for (int m0 = m_begin; m0 < m_end; m0 += TN_BK) {
        __syncthreads();
        store_chunk();
        __syncthreads();
        if (m0 + TN_BK < m_end) load_chunk(m0 + TN_BK);
#pragma unroll
        for (int ks = 0; ks < TN_BK / 16; ++ks) {
            bf16x8 ah[2], al[2], bh[NB], bl[NB];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int o = (wm * 64 + i * 32 + l31) * TN_STRIDE + ks * 16 + half * 8;
                ah[i] = *reinterpret_cast<const bf16x8 *>(&Ah[o]);
                al[i] = *reinterpret_cast<const bf16x8 *>(&Al[o]);
            }
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int o = (wn * (BN / 2) + j * 32 + l31) * TN_STRIDE + ks * 16 + half * 8;
                bh[j] = *reinterpret_cast<const bf16x8 *>(&Wh[o]);
                bl[j] = *reinterpret_cast<const bf16x8 *>(&Wl[o]);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
    }
    float *P = partials + (size_t)split * N * K;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int col = k_blk + wn * (BN / 2) + j * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = n_blk + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (row < N && col < K) P[(size_t)row * K + col] = acc[i][j][r];
            }
        }
    if (want_db) { // uniform per block
        __syncthreads();
        float *red = reinterpret_cast<float *>(smem3);
        red[tid] = colsum;
        __syncthreads();
        if (tid < 128 && n_blk + tid < N) db_part[(size_t)split * N + n_blk + tid] = red[tid] + red[tid + 128];
    }
}

// ---- the pipelined form of the same product (see gemm3_tn_kernel above for the contract) ----
// Same division of labour as gemm3p_nt_kernel (gemm3p.h): the 128 dY columns of the tile are shared by the four wavefronts and go through
// the LDS (transposed on the way in: a thread loads 8 consecutive m of ONE column with 8 coalesced dword loads and stores them as
// one 16-byte fragment word per plane), the X columns belong to exactly one wavefront each (32 NB of them) and go straight from
// global memory into fragment registers: lane (l31, half) of block j loads X[m0 + 8 half + e][k0 + 32 j + l31], e = 0..7 -- eight
// dword loads of two full 128-byte lines each.  One barrier per 32 rows of m; no LDS traffic for X at all.  NB = 1, 2 or 4 (a wavefront
// then owns 32 / 64 / 128 X columns and 64 / 128 / 256 accumulator registers).
template <int NB, bool GATE>
__global__ __launch_bounds__(256, 1) void gemm3p_tn_kernel(int M, int N, int K, const float *__restrict__ dY, int ldy, const float *__restrict__ Ygate,
                                                           const float *__restrict__ X, int ldx, int rows_per_split, int nsplit,
                                                           float *__restrict__ partials, float *__restrict__ db_part)
{
    constexpr int MI = 4, PS = 40, BUF = 2 * 128 * PS;
    extern __shared__ __attribute__((aligned(16))) char smem3p[];
    __bf16 *lds = reinterpret_cast<__bf16 *>(smem3p);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6); // (uniform: the buffer resources below live in SGPRs)
    const int half = lane >> 5, l31 = lane & 31;
    // XCD-aware 1-D grid: workgroup L runs on XCD L % 8 (round-robin dispatch); all tiles of one split go to ONE XCD, so the rows
    // of dY and X that the split owns stream through one L2 once (the tiles advance over m together) instead of through up to 8 of
    // them (with x-fastest 3-D indexing every tile of a split sat on a different XCD: 14.7 GB of L2 misses for 3.3 GB of operands)
    const int L = blockIdx.x, NX = N / 128, tiles = NX * (K / (128 * NB));
    const int split = (L & 7) + 8 * ((L >> 3) / tiles), tile = (L >> 3) % tiles;
    if (split >= nsplit) return;
    const int n_blk = (tile % NX) * 128, k_blk = (tile / NX) * (128 * NB) + wave * 32 * NB;
    // M and rows_per_split are multiples of 32 here (the launcher hands the last M % 32 rows to gemm3_tn_kernel): no row predicates,
    // and every row offset below is wave-uniform, i.e. scalar address arithmetic (one SALU add per load instead of a 64-bit VALU chain)
    const int m_begin = split * rows_per_split;
    const int m_end = min(M, m_begin + rows_per_split);
    const int T = (m_end - m_begin) / 32;
    const bool want_db = db_part != nullptr && tile / NX == 0;

    f32x16 acc[MI][NB];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // dY staging: thread (column c, half-tile g0) owns m groups g0 and g0 + 2 (8 rows each) of the 32-row tile
    const int c = tid & 127, g0 = __builtin_amdgcn_readfirstlane(tid >> 7);
    // Buffer addressing relative to the split's first row: a load is ONE instruction (per-lane byte offset register + wave-uniform
    // scalar offset + immediate).  With flat 64-bit addresses every one of the 48 loads of a 32-row tile carried a 64-bit VALU add
    // and three scalar multiplies / adds -- 130 of the loop's 460 instructions, on a wavefront that is alone on its SIMD.
    // (a split spans < 2^31 bytes of either operand: rows_per_split * ld * 4)
    const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc((void *)(dY + (size_t)m_begin * ldy + n_blk), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc((void *)((GATE ? Ygate : dY) + (size_t)m_begin * ldy + n_blk), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void *)(X + (size_t)m_begin * ldx + k_blk), 0, 0x7fffffff, 0x00020000);
    unsigned yv[8], xv[8]; // per-lane byte offsets of row e of a group: column c of dY; the lane's X column, its 8 rows start 8 * half below the k-step's first row
#pragma unroll
    for (int e = 0; e < 8; ++e) { yv[e] = (unsigned)(e * ldy + c) * 4u; xv[e] = (unsigned)((half * 8 + e) * ldx + l31) * 4u; }
    float sy[2][8], sg[GATE ? 2 : 1][8];
    // X: raw rows of this lane's fragments, [k-step][block][e]
    float rx[2][NB][8];
    bf16x8 fah[2][MI], fal[2][MI], fwh[2][NB], fwl[2][NB];
    float colsum = 0.0f;
    // tiles past the end of the split (the pipeline runs two ahead) read its last tile again; what they stage is never multiplied
    auto load_y = [&](int q, int tile) {
        const unsigned so = (unsigned)((min(tile, T - 1) * 32 + (g0 + 2 * q) * 8) * ldy) * 4u; // wave-uniform
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sy[q][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(yrs, yv[e], so, 0));
            if (GATE) sg[GATE ? q : 0][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(grs, yv[e], so, 0));
        }
    };
    auto stage_y = [&](int q, int tile, int b) {
        const float cm = tile < T ? 1.0f : 0.0f; // the column sums count every row once
        __bf16 *Ah = lds + b * BUF, *Al = Ah + 128 * PS;
        bf16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float a = sy[q][e];
            if (GATE) a = sg[GATE ? q : 0][e] > 0.0f ? a : 0.0f;
            colsum = fmaf(cm, a, colsum);
            const __bf16 h = (__bf16)a;
            hi[e] = h;
            lo[e] = (__bf16)(a - (float)h);
        }
        *reinterpret_cast<bf16x8 *>(&Ah[c * PS + (g0 + 2 * q) * 8]) = hi;
        *reinterpret_cast<bf16x8 *>(&Al[c * PS + (g0 + 2 * q) * 8]) = lo;
    };
    auto load_x = [&](int ks, int j, int tile) {
        const unsigned so = (unsigned)((min(tile, T - 1) * 32 + ks * 16) * ldx) * 4u; // wave-uniform
#pragma unroll
        for (int e = 0; e < 8; ++e) rx[ks][j][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, xv[e] + 128u * j, so, 0));
    };
    auto convert_x = [&](int ks, int j) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float a = rx[ks][j][e];
            const __bf16 h = (__bf16)a;
            fwh[ks][j][e] = h;
            fwl[ks][j][e] = (__bf16)(a - (float)h);
        }
    };
    const int a_off = l31 * PS + half * 8;
    auto read_a = [&](int ks, int s, int b) {
        const __bf16 *Ah = lds + b * BUF + ks * 16 + a_off, *Al = Ah + 128 * PS;
        if (s < 4) fah[ks][s] = *reinterpret_cast<const bf16x8 *>(&Ah[s * 32 * PS]);
        else fal[ks][s - 4] = *reinterpret_cast<const bf16x8 *>(&Al[(s - 4) * 32 * PS]);
    };
    auto mfma_one = [&](int ks, int s) {
        const int t = s / (MI * NB), i = (s % (MI * NB)) / NB, j = s % NB;
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(t == 0 ? fal[ks][i] : fah[ks][i], t == 1 ? fwl[ks][j] : fwh[ks][j], acc[i][j], 0, 0, 0);
    };
    constexpr int G = MI * NB, RPG = 8 / G; // groups of three MFMAs per k-step; dY fragment reads per group

    // prologue: dY tile 0 in LDS buffer 0, tile 1 staged; X tile 0 converted (k-step 0) / raw (k-step 1), tile 1 k-step 0 requested
    load_y(0, 0); load_y(1, 0);
#pragma unroll
    for (int j = 0; j < NB; ++j) { load_x(0, j, 0); load_x(1, j, 0); }
    stage_y(0, 0, 0); stage_y(1, 0, 0);
    load_y(0, 1); load_y(1, 1);
#pragma unroll
    for (int j = 0; j < NB; ++j) { convert_x(0, j); load_x(0, j, 1); }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 8; ++s) read_a(0, s, 0);
    int cur = 0;
    for (int t = 0; t < T; ++t) {
        // Branch-free body.
        // ---- phase A: k-step 0 | dY fragments of k-step 1; dY tile t+1 into the other buffer, tile t+2 requested; X k-step 1 of
        //      tile t converted, of tile t+1 requested ----
#pragma unroll
        for (int g = 0; g < G; ++g) {
            mfma_one(0, 3 * g);
#pragma unroll
            for (int r = 0; r < RPG; ++r) read_a(1, g * RPG + r, cur);
            if (RPG == 0 && g % (G / 8) == 0) read_a(1, g / (G / 8), cur);
            mfma_one(0, 3 * g + 1);
            if (g == 0 || g == G / 2) { const int q = g ? 1 : 0; stage_y(q, t + 1, cur ^ 1); load_y(q, t + 2); }
            if (g % (G / NB) == G / NB - 1) { const int j = g / (G / NB); convert_x(1, j); load_x(1, j, t + 1); }
            mfma_one(0, 3 * g + 2);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads(); // dY tile t+1 is complete, the buffer of tile t is free
        // ---- phase B: k-step 1 | dY fragments (k-step 0) of tile t+1; X k-step 0 of tile t+1 converted, of tile t+2 requested ----
#pragma unroll
        for (int g = 0; g < G; ++g) {
            mfma_one(1, 3 * g);
#pragma unroll
            for (int r = 0; r < RPG; ++r) read_a(0, g * RPG + r, cur ^ 1);
            if (RPG == 0 && g % (G / 8) == 0) read_a(0, g / (G / 8), cur ^ 1);
            mfma_one(1, 3 * g + 1);
            if (g % (G / NB) == G / NB - 1) { const int j = g / (G / NB); convert_x(0, j); load_x(0, j, t + 2); }
            mfma_one(1, 3 * g + 2);
            __builtin_amdgcn_sched_barrier(0);
        }
        cur ^= 1;
    }
    float *P = partials + (size_t)split * N * K;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            float *pp = P + (size_t)(n_blk + i * 32 + 4 * half) * K + k_blk + j * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) pp[(size_t)((r & 3) + 8 * (r >> 2)) * K] = acc[i][j][r];
        }
    if (want_db) { // uniform per block
        __syncthreads();
        float *red = reinterpret_cast<float *>(smem3p);
        red[tid] = colsum;
        __syncthreads();
        if (tid < 128) db_part[(size_t)split * N + n_blk + tid] = red[tid] + red[tid + 128];
    }
}

// out[i] = sum_s part[s][i] in split order (deterministic)
__global__ void reduce_partials_kernel(size_t n, int splits, const float *__restrict__ part, float *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        float acc = 0.0f;
        for (int s = 0; s < splits; ++s) acc += part[(size_t)s * n + i];
        out[i] = acc;
    }
}

// The same sum for MANY partials of a SMALL output (embed0's 128 x (D + 1) gradient from thousands of blocks, a bias gradient from
// 64 splits): one output per wavefront instead of per thread -- lane l adds partials l, l + 64, ... (ascending), then the 64 lane
// sums are combined in a fixed butterfly order: deterministic, and the serial chain is splits / 64 long instead of splits.
__global__ __launch_bounds__(256) void reduce_partials_wide_kernel(size_t n, int splits, const float *__restrict__ part, float *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    float acc = 0.0f;
    for (int s = lane; s < splits; s += 64) acc += part[(size_t)s * n + i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) out[i] = acc;
}

// dW and db of one weight gradient in ONE launch: blocks 0 .. nb1-1 reduce (n1, part1 -> out1), the rest (n2, part2 -> out2), each with the
// per-output summation order of the kernel above that launch_reduce_partials would have picked for it (results are bit-identical)
__global__ __launch_bounds__(256) void reduce_partials_pair_kernel(size_t n1, size_t n2, int splits, const float *__restrict__ part1, float *__restrict__ out1,
                                                                   const float *__restrict__ part2, float *__restrict__ out2, int nb1, int wide1, int wide2)
{
    const bool second = (int)blockIdx.x >= nb1;
    const size_t n = second ? n2 : n1;
    const float *part = second ? part2 : part1;
    float *out = second ? out2 : out1;
    const unsigned b = second ? blockIdx.x - nb1 : blockIdx.x;
    if (second ? wide2 : wide1) {
        const size_t i = (size_t)b * 4 + (threadIdx.x >> 6);
        const int lane = threadIdx.x & 63;
        if (i >= n) return;
        float acc = 0.0f;
        for (int s = lane; s < splits; s += 64) acc += part[(size_t)s * n + i];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) out[i] = acc;
    } else {
        const size_t i = (size_t)b * 256 + threadIdx.x;
        if (i < n) {
            float acc = 0.0f;
            for (int s = 0; s < splits; ++s) acc += part[(size_t)s * n + i];
            out[i] = acc;
        }
    }
}
static void launch_reduce_partials_pair(size_t n1, size_t n2, int splits, const float *part1, float *out1, const float *part2, float *out2, hipStream_t st)
{
    const int w1 = splits >= 48 && n1 <= 16384, w2 = splits >= 48 && n2 <= 16384;
    const int nb1 = (int)(w1 ? (n1 + 3) / 4 : (n1 + 255) / 256), nb2 = (int)(w2 ? (n2 + 3) / 4 : (n2 + 255) / 256);
    hipLaunchKernelGGL(reduce_partials_pair_kernel, dim3(nb1 + nb2), dim3(256), 0, st, n1, n2, splits, part1, out1, part2, out2, nb1, w1, w2);
}

static void launch_reduce_partials(size_t n, int splits, const float *part, float *out, hipStream_t st)
{
    if (splits >= 48 && n <= 16384) hipLaunchKernelGGL(reduce_partials_wide_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, n, splits, part, out);
    else hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, splits, part, out);
}

} // namespace
