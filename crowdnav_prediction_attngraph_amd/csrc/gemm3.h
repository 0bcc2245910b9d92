// gemm3.h -- the split-precision ("bf16x3", split_bf16.h) NT GEMM of the rollout forward's separate-launch mode and the plain hi / lo
// split of its weights.  Only policy.hip includes it; the PPO update has its own kernels (gemm3p.h, gemm3_tn.h).
#pragma once
#include "common.h"
#include "gemm.h"
#include "split_bf16.h"

namespace {

// The kernel is a plain two-barrier loop whose phases (global loads in flight, convert + LDS stores, MFMA, C stores) do not
// overlap inside one workgroup; what hides them is other workgroups in other phases.  Stand-alone, occupancy beats tile depth --
// measured on the q|k|v shapes (random operands)  BK 64 / 2 per CU: 180 us | 2348 us (M = 24.5 k | 368 k),
// BK 32 / 3 per CU: 168 | 2025,  BK 16 / 4 per CU: 161 | 1888 (307 TFLOP/s algorithmic = 920 executed) -- but the rollout forward
// shares the chip with the ORCA side stream and does best with deep tiles (the update's two-barrier TN kernel, gemm3_tn.h, takes the
// shallow end: TN_BK = 16).
// LDS rows are the K tile + 8 bf16 of pad: 16 consecutive rows' 16-byte fragment reads then tile all 64 banks.

// K tile of gemm3_nt_kernel (the rollout forward's separate-launch mode): 64, two workgroups per CU
constexpr int NT_BK = 64;
constexpr int NT_STRIDE = NT_BK + 8;

template <int TBM, int BN, int ACT>
__global__ __launch_bounds__(256, 2) void gemm3_nt_kernel(int M, int N, int K, const float *__restrict__ A, int lda,
                                                       const __bf16 *__restrict__ Whi, const __bf16 *__restrict__ Wlo,
                                                       const float *__restrict__ bias, float *__restrict__ C, int ldc,
                                                       const int *__restrict__ m_dev)
{
    if (m_dev) { const int md = *m_dev; M = md < M ? md : M; }
    int row_tile, col_tile;
    if ((size_t)N * K > (size_t)512 * 1024 && !(gridDim.x & 1)) xcd_tile_split(row_tile, col_tile); // W planes > 2 MB: halve the per-L2 W set
    else xcd_tile(row_tile, col_tile);
    if (row_tile * TBM >= M) return;
    constexpr int MI = TBM / 64;             // 32-row MFMA blocks per wavefront (2 x 2 wavefronts: TBM/2 rows each)
    constexpr int NB = BN / 64;
    constexpr int AQ = NT_BK / 4, ARP = 256 / AQ; // float4 per A row of the K tile, rows staged per pass
    constexpr int ALD = TBM / ARP;                // float4 loads of A per thread per K tile
    constexpr int WQ = NT_BK / 8;                 // 16-byte chunks per W row of the K tile
    constexpr int WCH = BN * WQ / 256;            // chunks of each W plane per thread per K tile
    static_assert(WCH >= 1 && ALD >= 1, "tile too small for 256 staging threads");
    extern __shared__ __attribute__((aligned(16))) char smem3[];
    __bf16 *Ah = reinterpret_cast<__bf16 *>(smem3);
    __bf16 *Al = Ah + TBM * NT_STRIDE;
    __bf16 *Wh = Al + TBM * NT_STRIDE;
    __bf16 *Wl = Wh + BN * NT_STRIDE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m_blk = row_tile * TBM, n_blk = col_tile * BN;
    const int lrow = tid / AQ, lcol = (tid % AQ) * 4; // A staging: AQ lanes cover one row segment of the K tile

    f32x16 acc[MI][NB];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    f32x4 pa[ALD];
    bf16x8 pwh[WCH], pwl[WCH];
    auto load_tiles = [&](int k0) {
#pragma unroll
        for (int p = 0; p < ALD; ++p) {
            const int r = m_blk + lrow + ARP * p;
            if (r < M) pa[p] = *reinterpret_cast<const f32x4 *>(A + (size_t)r * lda + k0 + lcol);
            else pa[p] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int p = 0; p < WCH; ++p) {
            const int c = tid + 256 * p, r = n_blk + c / WQ, col = (c % WQ) * 8;
            pwh[p] = *reinterpret_cast<const bf16x8 *>(Whi + (size_t)r * K + k0 + col);
            pwl[p] = *reinterpret_cast<const bf16x8 *>(Wlo + (size_t)r * K + k0 + col);
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int p = 0; p < ALD; ++p) {
            bf16x4 hi, lo;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float a = pa[p][q];
                hi[q] = (__bf16)a;
                lo[q] = (__bf16)(a - (float)hi[q]);
            }
            *reinterpret_cast<bf16x4 *>(&Ah[(lrow + ARP * p) * NT_STRIDE + lcol]) = hi;
            *reinterpret_cast<bf16x4 *>(&Al[(lrow + ARP * p) * NT_STRIDE + lcol]) = lo;
        }
#pragma unroll
        for (int p = 0; p < WCH; ++p) {
            const int c = tid + 256 * p, r = c / WQ, col = (c % WQ) * 8;
            *reinterpret_cast<bf16x8 *>(&Wh[r * NT_STRIDE + col]) = pwh[p];
            *reinterpret_cast<bf16x8 *>(&Wl[r * NT_STRIDE + col]) = pwl[p];
        }
    };

    load_tiles(0);
    const int half = lane >> 5, l31 = lane & 31;
    for (int k0 = 0; k0 < K; k0 += NT_BK) {
        __syncthreads();
        store_tiles();
        __syncthreads();
        if (k0 + NT_BK < K) load_tiles(k0 + NT_BK);
#pragma unroll
        for (int ks = 0; ks < NT_BK / 16; ++ks) {
            bf16x8 ah[MI], al[MI], bh[NB], bl[NB];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int o = (wm * (TBM / 2) + i * 32 + l31) * NT_STRIDE + ks * 16 + half * 8;
                ah[i] = *reinterpret_cast<const bf16x8 *>(&Ah[o]);
                al[i] = *reinterpret_cast<const bf16x8 *>(&Al[o]);
            }
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int o = (wn * (BN / 2) + j * 32 + l31) * NT_STRIDE + ks * 16 + half * 8;
                bh[j] = *reinterpret_cast<const bf16x8 *>(&Wh[o]);
                bl[j] = *reinterpret_cast<const bf16x8 *>(&Wl[o]);
            }
            // term-major issue order: consecutive MFMAs hit different accumulators (no back-to-back dependent chain)
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
    }
    // Epilogue.  The bias is fetched and waited for once, and a tile that lies inside M stores without per-row predicates: with
    // the predicate every store sits in its own basic block behind an s_waitcnt vmcnt(0) (the compiler cannot tell there that
    // the bias load has landed), i.e. every store waits for the previous one to complete (see gemm3p.h).
    float bv[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) bv[j] = bias ? bias[n_blk + wn * (BN / 2) + j * 32 + l31] : 0.0f;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    auto store_all = [&](auto guard) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int col = n_blk + wn * (BN / 2) + j * 32 + l31;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m_blk + wm * (TBM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    float v = acc[i][j][r] + bv[j];
                    if (ACT == ACT_RELU) v = fmaxf(v, 0.0f);
                    if (ACT == ACT_TANH) v = tanhf(v);
                    // streaming result (150 MB for q|k|v, far beyond any L2): non-temporal stores keep A / W resident in the L2
                    if (guard(row)) __builtin_nontemporal_store(v, &C[(size_t)row * ldc + col]);
                }
            }
    };
    if (m_blk + TBM <= M) store_all([](int) { return true; });
    else store_all([&](int row) { return row < M; });
}

// split a fp32 weight matrix into bf16 hi / lo parts
__global__ void split_bf16_kernel(size_t n, const float *__restrict__ w, __bf16 *__restrict__ hi, __bf16 *__restrict__ lo)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const __bf16 h = (__bf16)w[i];
        hi[i] = h;
        lo[i] = (__bf16)(w[i] - (float)h);
    }
}

// rows = live humans: BM-row tiles, like the exact-fp32 launch_gemm of policy.hip
template <int BN, int ACT>
static int launch_gemm3(int M, int N, int K, const float *A, int lda, const __bf16 *Whi, const __bf16 *Wlo, const float *bias, float *C, int ldc,
                        hipStream_t st, const int *m_dev)
{
    CN_REQUIRE(N % BN == 0 && K % NT_BK == 0 && lda % 4 == 0, "gemm3: unsupported shape M=%d N=%d K=%d lda=%d", M, N, K, lda);
    if (M == 0) return CN_OK;
    dim3 grid(N / BN, (((M + BM - 1) / BM) + 7) & ~7);
    constexpr size_t lds = (size_t)(2 * BM + 2 * BN) * NT_STRIDE * sizeof(__bf16); // 73.7 KB at 128 x 128: needs the opt-in above 64 KB
    if (int rc = cn_lds_opt_in<&gemm3_nt_kernel<BM, BN, ACT>>((int)lds)) return rc;
    hipLaunchKernelGGL((gemm3_nt_kernel<BM, BN, ACT>), grid, dim3(256), lds, st, M, N, K, A, lda, Whi, Wlo, bias, C, ldc, m_dev);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

} // namespace
