// attention.h -- the two attention cores of the policy outside the fused kernels, forward and backward: the human-human multi-head
// attention on the compacted rows (hh_attention_kernel per size class, hh_classify_kernel, the VALU and MFMA backward kernels and
// their launchers) and the robot-human attention (hr_attention_kernel, hr_attention_bwd_kernel).  The rollout's separate-launch
// modes and the training entry points both launch them; part of policy.hip's translation unit.
#pragma once
#include "common.h"

namespace {

// Human-human multi-head attention core (torch.nn.MultiheadAttention with key_padding_mask, 8 heads x 64) on the
// compacted rows: one wavefront per (env, head).
//   load    : lane d reads element d of every live row: Q, K rows go to LDS (row stride 68 floats = 16-byte aligned and
//             conflict-free for ds_read_b128), V stays in registers (lane d only ever needs column d of V)
//   scores  : lanes enumerate (query i, key j) pairs, 64 pairs per pass; each dot product is 16 x (2 b128 reads + 4 FMA)
//   softmax : lane i owns row i of S (LDS, row stride CAP, zero padded so P*V can read float4s)
//   P*V     : lane d: o[i][d] = sum_j S[i][j] * v[j]
// Masked keys are simply absent (softmax over the nd live keys == softmax with -inf on the padded ones).
// CAP in {8,16,32,64} are size classes sharing one launch grid: class (cap_lo, CAP] handles the units with that many
// detected humans (the common case of ~6 uses 4.6 KB of LDS per wavefront -> high occupancy); other units exit at once.
template <int CAP>
__global__ __launch_bounds__(256) void hh_attention_kernel(int E, int cap_lo, const float *__restrict__ qkv, const int *__restrict__ row_off,
                                                           const int *__restrict__ cls_cnt, const int *__restrict__ cls_list,
                                                           float *__restrict__ out, float scale)
{
    constexpr int RS = 68;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    // wavefronts walk (env, head) units.  Without a class list every unit is inspected in env order and filtered by nd
    // (grid = one unit per wavefront); with one (the rare big classes, whose 39-65 KB blocks would otherwise queue up
    // just to exit) a resident-sized grid walks only that class's envs.
    const int n_units = (cls_list ? *cls_cnt : E) * 8;
    for (int unit = blockIdx.x * wpb + wave; unit < n_units; unit += gridDim.x * wpb) {
    const int e = cls_list ? cls_list[unit >> 3] : unit >> 3, head = unit & 7;
    const int r0 = row_off[e], nd = row_off[e + 1] - r0;
    if (nd <= cap_lo || nd > CAP) continue; // another size class handles this unit
    float *Ks = smem + (size_t)wave * (2 * CAP * RS + CAP * CAP);
    float *Qs = Ks + CAP * RS;
    float *S = Qs + CAP * RS;
    const float *base = qkv + (size_t)r0 * 1536 + head * 64 + lane;
    float v[CAP];
#pragma unroll
    for (int j0 = 0; j0 < CAP; j0 += 8) {
        if (j0 < nd) { // wave-uniform
            float q[8], k[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float *row = base + (size_t)(j0 + u < nd ? j0 + u : 0) * 1536;
                q[u] = row[0]; k[u] = row[512]; v[j0 + u] = row[1024];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (j0 + u < nd) { Qs[(j0 + u) * RS + lane] = q[u]; Ks[(j0 + u) * RS + lane] = k[u]; }
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) v[j0 + u] = 0.0f;
        }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f); // lgkmcnt(0): LDS writes of this wavefront visible to its own reads
    const int npairs = nd * nd;
    for (int q = lane; q < npairs; q += 64) {
        const int qi = q / nd, qj = q - qi * nd;
        const f32x4 *qp = reinterpret_cast<const f32x4 *>(Qs + qi * RS);
        const f32x4 *kp = reinterpret_cast<const f32x4 *>(Ks + qj * RS);
        float s = 0.0f;
#pragma unroll
        for (int d = 0; d < 16; ++d) {
            const f32x4 a = qp[d], b = kp[d];
            s += a[0] * b[0]; s += a[1] * b[1]; s += a[2] * b[2]; s += a[3] * b[3];
        }
        S[qi * CAP + qj] = s * scale;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);
    if (lane < nd) {
        // whole row in registers (16-byte reads, all issued before the first use): as loops over the run-time nd, every LDS read
        // waited for the one before it.  Entries past nd hold stale scores of earlier units: masked here, stored as zeros.
        float *row = S + lane * CAP;
        float p[CAP];
#pragma unroll
        for (int j4 = 0; j4 < CAP / 4; ++j4) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(row + 4 * j4);
#pragma unroll
            for (int u = 0; u < 4; ++u) p[4 * j4 + u] = a[u];
        }
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < CAP; ++j) mx = j < nd ? fmaxf(mx, p[j]) : mx;
        float sum = 0.0f;
#pragma unroll
        for (int j = 0; j < CAP; ++j) { p[j] = j < nd ? expf(p[j] - mx) : 0.0f; sum += p[j]; }
        const float inv = 1.0f / sum;
#pragma unroll
        for (int j4 = 0; j4 < CAP / 4; ++j4)
            *reinterpret_cast<f32x4 *>(row + 4 * j4) = f32x4{p[4 * j4] * inv, p[4 * j4 + 1] * inv, p[4 * j4 + 2] * inv, p[4 * j4 + 3] * inv};
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);
    for (int i = 0; i < nd; ++i) {
        const f32x4 *prow = reinterpret_cast<const f32x4 *>(S + i * CAP);
        float o = 0.0f;
#pragma unroll
        for (int j4 = 0; j4 < CAP / 4; ++j4) {
            const f32x4 p = prow[j4];
            o += p[0] * v[4 * j4]; o += p[1] * v[4 * j4 + 1]; o += p[2] * v[4 * j4 + 2]; o += p[3] * v[4 * j4 + 3];
        }
        out[(size_t)(r0 + i) * 512 + head * 64 + lane] = o;
    }
    __builtin_amdgcn_wave_barrier(); // the next unit reuses this wavefront's LDS slices
    }
}

template <int CAP>
static int launch_hh_attention(int E, int cap_lo, const float *qkv, const int *row_off, float *out, hipStream_t st, float scale = 1.0f,
                               const int *cls_cnt = nullptr, const int *cls_list = nullptr)
{
    const size_t per_wave = (size_t)(2 * CAP * 68 + CAP * CAP) * sizeof(float);
    int wpb = (int)(65536 / per_wave); wpb = wpb < 1 ? 1 : (wpb > 4 ? 4 : wpb);
    int per_cu = (int)((160 * 1024) / (per_wave * wpb)); per_cu = per_cu > 8 ? 8 : per_cu; // resident blocks per CU (LDS / 32-wave cap)
    int blocks = (E * 8 + wpb - 1) / wpb;
    if (cls_list && blocks > 256 * per_cu) blocks = 256 * per_cu; // (a new cap: move tests/test_gpu_strided_grids.py, which runs past twice this one)
    hipLaunchKernelGGL(hh_attention_kernel<CAP>, dim3(blocks), dim3(64 * wpb), per_wave * wpb, st, E, cap_lo, qkv, row_off, cls_cnt, cls_list, out, scale);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

// Size classes of the (sample, head) units for the training kernels: class c holds the samples with cap_lo(c) < nd <= cap(c),
// caps 8 / 16 / 32 / 64.  cls = [4] counts followed by [4][B] sample lists (order inside a list is arbitrary -- a unit writes
// only its own rows).  One launch per class then walks exactly its own units with an LDS footprint sized for that class.
__global__ __launch_bounds__(256) void hh_classify_kernel(int B, const int *__restrict__ row_off, int *__restrict__ cls)
{
    __shared__ int cnt[4], base[4];
    const int t = threadIdx.x;
    if (t < 4) cnt[t] = 0;
    __syncthreads();
    const int b = blockIdx.x * blockDim.x + t;
    int c = -1, slot = 0;
    if (b < B) {
        const int nd = row_off[b + 1] - row_off[b];
        c = nd <= 8 ? 0 : (nd <= 16 ? 1 : (nd <= 32 ? 2 : 3));
        slot = atomicAdd(&cnt[c], 1);
    }
    __syncthreads();
    if (t < 4) base[t] = cnt[t] ? atomicAdd(&cls[t], cnt[t]) : 0;
    __syncthreads();
    if (c >= 0) cls[4 + (size_t)c * B + base[c] + slot] = b;
}

// Backward of the attention core for training (PPO update): per (sample, head) on the compacted rows.
//   S = scale * Q K^T, P = softmax(S), O = P V ;   given dO:
//   dV = P^T dO ; dP = dO V^T ; dS = scale * P .* (dP - rowsum(dP .* P)) ; dQ = dS K ; dK = dS^T Q
// One wavefront per unit; Q, K, V, dO rows in LDS (stride 68), P and dS as nd x nd matrices (stride CAP) in LDS.  CAP is the size
// class (see hh_classify_kernel): the common class of <= 8 detected humans needs 9 KB per wavefront instead of the 25 KB of H = 20,
// so 16 wavefronts are resident per CU instead of 6.
template <int CAP>
__global__ __launch_bounds__(256) void hh_attention_bwd_kernel(int B, const float *__restrict__ qkv, const int *__restrict__ row_off,
                                                               const int *__restrict__ cls_cnt, const int *__restrict__ cls_list,
                                                               const float *__restrict__ d_out, float *__restrict__ d_qkv, float scale)
{
    constexpr int RS = 68;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int n_units = (cls_list ? *cls_cnt : B) * 8;
    constexpr bool REG = CAP <= 32; // softmax rows and the K / Q / dO columns in registers, see below
    float *Qs = smem + (size_t)wave * (4 * CAP * RS + (REG ? 4 : 2) * CAP * CAP);
    float *Ks = Qs + CAP * RS, *Vs = Ks + CAP * RS, *Gs = Vs + CAP * RS; // Gs = dO rows
    float *P = Gs + CAP * RS, *dS = P + CAP * CAP;
    float *PT = dS + CAP * CAP, *dST = PT + CAP * CAP; // (REG only) transposed copies: dK and dV walk columns of dS and P
    if (REG) { // rows at or past nd are read (with zero weights) by the unrolled loops below: they must hold finite numbers
        for (int x = lane; x < 4 * CAP * RS; x += 64) Qs[x] = 0.0f;
    }
    // A wavefront walks ~240 units, and a unit starts with three DEPENDENT memory round trips (class list -> row offsets -> rows)
    // before any arithmetic.  For the small classes (4 CAP registers) the walk is a three-stage pipeline instead: while unit u is
    // computed, the rows of unit u+1, the row offsets of unit u+2 and the sample id of unit u+3 are in flight.
    constexpr bool PIPE = CAP <= 16;
    float pq[PIPE ? CAP : 1], pk[PIPE ? CAP : 1], pv[PIPE ? CAP : 1], pg[PIPE ? CAP : 1];
    const int stride = gridDim.x * wpb;
    int unit = blockIdx.x * wpb + wave;
    auto sample_of = [&](int u) { return u < n_units ? (cls_list ? cls_list[u >> 3] : u >> 3) : 0; };
    auto request_rows = [&](int r0n, int ndn, int head) {
        const float *base = qkv + (size_t)r0n * 1536 + head * 64 + lane;
        const float *gbase = d_out + (size_t)r0n * 512 + head * 64 + lane;
#pragma unroll
        for (int j = 0; j < (PIPE ? CAP : 0); ++j)
            if (j < ndn) { // wave-uniform
                pq[j] = base[(size_t)j * 1536]; pk[j] = base[(size_t)j * 1536 + 512]; pv[j] = base[(size_t)j * 1536 + 1024];
                pg[j] = gbase[(size_t)j * 512];
            }
    };
    int c_r0 = 0, c_nd = 0, n_lo = 0, n_hi = 0, b2 = 0; // rows in flight belong to (c_r0, c_nd); raw offsets of the unit after it; sample after that
    if (PIPE && unit < n_units) {
        const int b0 = sample_of(unit), b1 = sample_of(unit + stride);
        b2 = sample_of(unit + 2 * stride);
        c_r0 = row_off[b0]; c_nd = row_off[b0 + 1] - c_r0;
        n_lo = row_off[b1]; n_hi = row_off[b1 + 1];
        request_rows(c_r0, c_nd, unit & 7);
    }
    for (; unit < n_units; unit += stride) {
        const int head = unit & 7;
        int r0, nd;
        if (PIPE) {
            r0 = c_r0; nd = c_nd;
#pragma unroll
            for (int j = 0; j < (PIPE ? CAP : 0); ++j)
                if (j < nd && nd <= CAP) { Qs[j * RS + lane] = pq[j]; Ks[j * RS + lane] = pk[j]; Vs[j * RS + lane] = pv[j]; Gs[j * RS + lane] = pg[j]; }
            c_r0 = n_lo; c_nd = n_hi - n_lo;
            request_rows(c_r0, c_nd, (unit + stride) & 7);        // (past the end: sample 0 again, never used)
            n_lo = row_off[b2]; n_hi = row_off[b2 + 1];
            b2 = sample_of(unit + 3 * stride);
            if (nd > CAP) continue; // (only without a class list: another launch handles it)
        } else {
            const int b = cls_list ? cls_list[unit >> 3] : unit >> 3;
            r0 = row_off[b]; nd = row_off[b + 1] - r0;
            if (nd > CAP) continue; // (only without a class list: another launch handles it)
            const float *base = qkv + (size_t)r0 * 1536 + head * 64 + lane;
            const float *gbase = d_out + (size_t)r0 * 512 + head * 64 + lane;
#pragma unroll 4
            for (int j = 0; j < nd; ++j) {
                const float q = base[(size_t)j * 1536], k = base[(size_t)j * 1536 + 512], v = base[(size_t)j * 1536 + 1024], g = gbase[(size_t)j * 512];
                Qs[j * RS + lane] = q; Ks[j * RS + lane] = k; Vs[j * RS + lane] = v; Gs[j * RS + lane] = g;
            }
        }
        if (REG) { // entries outside nd x nd stay zero for this unit
#pragma unroll
            for (int x = 0; x < 4 * CAP * CAP; x += 64) P[x + lane] = 0.0f;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);
        const int npairs = nd * nd;
        for (int q = lane; q < npairs; q += 64) {
            const int qi = q / nd, qj = q - qi * nd;
            const f32x4 *qp = reinterpret_cast<const f32x4 *>(Qs + qi * RS), *kp = reinterpret_cast<const f32x4 *>(Ks + qj * RS);
            const f32x4 *gp = reinterpret_cast<const f32x4 *>(Gs + qi * RS), *vp = reinterpret_cast<const f32x4 *>(Vs + qj * RS);
            float s = 0.0f, dp = 0.0f;
#pragma unroll
            for (int d = 0; d < 16; ++d) {
                const f32x4 a = qp[d], bb = kp[d], g = gp[d], v = vp[d];
                s += a[0] * bb[0]; s += a[1] * bb[1]; s += a[2] * bb[2]; s += a[3] * bb[3];
                dp += g[0] * v[0]; dp += g[1] * v[1]; dp += g[2] * v[2]; dp += g[3] * v[3];
            }
            P[qi * CAP + qj] = s * scale;
            dS[qi * CAP + qj] = dp;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);
        float *ob = d_qkv + (size_t)r0 * 1536 + head * 64 + lane;
        if (REG) {
            // The loops over nd below have run-time bounds: left as loops, every LDS read waits for the one before it (a (sample,
            // head) unit cost ~nd^2 serial LDS round trips).  Here they run to the compile-time CAP on whole rows in registers
            // (16-byte reads, all issued before the first use); entries past nd are zeros, so they add nothing.
            if (lane < nd) {
                float p[CAP], d[CAP];
#pragma unroll
                for (int j4 = 0; j4 < CAP / 4; ++j4) {
                    const f32x4 a = *reinterpret_cast<const f32x4 *>(P + lane * CAP + 4 * j4), b = *reinterpret_cast<const f32x4 *>(dS + lane * CAP + 4 * j4);
#pragma unroll
                    for (int u = 0; u < 4; ++u) { p[4 * j4 + u] = a[u]; d[4 * j4 + u] = b[u]; }
                }
                float mx = -INFINITY;
#pragma unroll
                for (int j = 0; j < CAP; ++j) mx = j < nd ? fmaxf(mx, p[j]) : mx;
                float sum = 0.0f;
#pragma unroll
                for (int j = 0; j < CAP; ++j) { p[j] = j < nd ? expf(p[j] - mx) : 0.0f; sum += p[j]; }
                const float inv = 1.0f / sum;
                float rd = 0.0f;
#pragma unroll
                for (int j = 0; j < CAP; ++j) { p[j] *= inv; rd += d[j] * p[j]; }
#pragma unroll
                for (int j = 0; j < CAP; ++j) d[j] = scale * p[j] * (d[j] - rd);
#pragma unroll
                for (int j4 = 0; j4 < CAP / 4; ++j4)
                    *reinterpret_cast<f32x4 *>(dS + lane * CAP + 4 * j4) = f32x4{d[4 * j4], d[4 * j4 + 1], d[4 * j4 + 2], d[4 * j4 + 3]};
#pragma unroll
                for (int j = 0; j < CAP; ++j) { PT[j * CAP + lane] = p[j]; dST[j * CAP + lane] = d[j]; }
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_waitcnt(0xc07f);
            float kr[CAP], qr[CAP], gr[CAP]; // column `lane` of K, Q, dO
#pragma unroll
            for (int i = 0; i < CAP; ++i) { kr[i] = Ks[i * RS + lane]; qr[i] = Qs[i * RS + lane]; gr[i] = Gs[i * RS + lane]; }
            for (int j = 0; j < nd; ++j) {
                float dq = 0.0f, dk = 0.0f, dv = 0.0f; // row j of dQ, dK, dV, column `lane`
#pragma unroll
                for (int i4 = 0; i4 < CAP / 4; ++i4) {
                    const f32x4 a = *reinterpret_cast<const f32x4 *>(dS + j * CAP + 4 * i4), b = *reinterpret_cast<const f32x4 *>(dST + j * CAP + 4 * i4);
                    const f32x4 c = *reinterpret_cast<const f32x4 *>(PT + j * CAP + 4 * i4);
#pragma unroll
                    for (int u = 0; u < 4; ++u) { dq += a[u] * kr[4 * i4 + u]; dk += b[u] * qr[4 * i4 + u]; dv += c[u] * gr[4 * i4 + u]; }
                }
                ob[(size_t)j * 1536] = dq; ob[(size_t)j * 1536 + 512] = dk; ob[(size_t)j * 1536 + 1024] = dv;
            }
        } else {
        if (lane < nd) {
            float *prow = P + lane * CAP, *drow = dS + lane * CAP;
            float mx = -INFINITY;
            for (int j = 0; j < nd; ++j) mx = fmaxf(mx, prow[j]);
            float sum = 0.0f;
            for (int j = 0; j < nd; ++j) { const float e = expf(prow[j] - mx); prow[j] = e; sum += e; }
            const float inv = 1.0f / sum;
            float rd = 0.0f;
            for (int j = 0; j < nd; ++j) { prow[j] *= inv; rd += drow[j] * prow[j]; }
            for (int j = 0; j < nd; ++j) drow[j] = scale * prow[j] * (drow[j] - rd);
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);
        for (int j = 0; j < nd; ++j) {
            float dq = 0.0f, dk = 0.0f, dv = 0.0f; // row j of dQ, dK, dV, column `lane`
            for (int i = 0; i < nd; ++i) {
                dq += dS[j * CAP + i] * Ks[i * RS + lane];
                dk += dS[i * CAP + j] * Qs[i * RS + lane];
                dv += P[i * CAP + j] * Gs[i * RS + lane];
            }
            ob[(size_t)j * 1536] = dq; ob[(size_t)j * 1536 + 512] = dk; ob[(size_t)j * 1536 + 1024] = dv;
        }
        }
        __builtin_amdgcn_wave_barrier(); // the next unit reuses this wavefront's LDS slices
    }
}

// The classes of 9 .. 16 and 17 .. 32 detected humans on the matrix pipe (exact fp32: v_mfma_f32_16x16x4_f32).  One wavefront per (sample, head) unit as
// above, the unit's five small products as 16 x 16 MFMA tiles instead of ~nd^2 dependent LDS reads and FMAs per lane:
//   S = Q K^T, dP = dO V^T            A / B = 16 consecutive features of row (lane & 15), feature block lane >> 4: four 16-byte LDS reads each
//   softmax / dS                      in the accumulator layout (lane holds rows 4 (lane >> 4) + r of column lane & 15): row sums by DPP rotations
//   dV = P^T dO, dK = dS^T Q          A = the accumulator registers themselves (P[4 kb + s][lane & 15] IS register s of this lane)
//   dQ = dS K                         A = dS read back transposed from a 16 x 17 LDS tile
// With the k index of a product taken as (lane >> 4, step) -> 4 (lane >> 4) + step (same permutation for A and B, so the sums are unchanged).
// Rows at or past nd hold stale finite data of earlier units: P is masked to zero there, which zeroes every term they appear in.
typedef float f32x4m __attribute__((ext_vector_type(4)));
template <int CTRL>
__device__ __forceinline__ float row_rot(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false)); }
__device__ __forceinline__ float row16_sum(float v) { v += row_rot<0x128>(v); v += row_rot<0x124>(v); v += row_rot<0x122>(v); v += row_rot<0x121>(v); return v; }
__device__ __forceinline__ float row16_max(float v)
{
    v = fmaxf(v, row_rot<0x128>(v)); v = fmaxf(v, row_rot<0x124>(v)); v = fmaxf(v, row_rot<0x122>(v)); v = fmaxf(v, row_rot<0x121>(v));
    return v;
}
template <int NT> // NT x NT tiles of 16 x 16: classes of <= 16 (NT = 1) and <= 32 (NT = 2) detected humans
__global__ __launch_bounds__(256) void hh_attention_bwd_mfma_kernel(int B, const float *__restrict__ qkv, const int *__restrict__ row_off,
                                                                    const int *__restrict__ cls_cnt, const int *__restrict__ cls_list,
                                                                    const float *__restrict__ d_out, float *__restrict__ d_qkv, float scale)
{
    constexpr int CAP = 16 * NT, RS = 68, TS = CAP + 1;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int n_units = (cls_list ? *cls_cnt : B) * 8;
    float *Qs = smem + (size_t)wave * (4 * CAP * RS + CAP * TS);
    float *Ks = Qs + CAP * RS, *Vs = Ks + CAP * RS, *Gs = Vs + CAP * RS; // Gs = dO rows
    float *dSt = Gs + CAP * RS;                                           // dS, CAP x (CAP + 1)
    for (int x = lane; x < 4 * CAP * RS; x += 64) Qs[x] = 0.0f;
    const int l15 = lane & 15, kb = lane >> 4;
    float pq[CAP], pk[CAP], pv[CAP], pg[CAP];
    const int stride = gridDim.x * wpb;
    int unit = blockIdx.x * wpb + wave;
    auto sample_of = [&](int u) { return u < n_units ? (cls_list ? cls_list[u >> 3] : u >> 3) : 0; };
    auto request_rows = [&](int r0n, int ndn, int head) {
        const float *base = qkv + (size_t)r0n * 1536 + head * 64 + lane;
        const float *gbase = d_out + (size_t)r0n * 512 + head * 64 + lane;
#pragma unroll
        for (int j = 0; j < CAP; ++j)
            if (j < ndn) { // wave-uniform
                pq[j] = base[(size_t)j * 1536]; pk[j] = base[(size_t)j * 1536 + 512]; pv[j] = base[(size_t)j * 1536 + 1024];
                pg[j] = gbase[(size_t)j * 512];
            }
    };
    int c_r0 = 0, c_nd = 0, n_lo = 0, n_hi = 0, b2 = 0;
    if (unit < n_units) {
        const int b0 = sample_of(unit), b1 = sample_of(unit + stride);
        b2 = sample_of(unit + 2 * stride);
        c_r0 = row_off[b0]; c_nd = row_off[b0 + 1] - c_r0;
        n_lo = row_off[b1]; n_hi = row_off[b1 + 1];
        request_rows(c_r0, c_nd, unit & 7);
    }
    for (; unit < n_units; unit += stride) {
        const int head = unit & 7;
        const int r0 = c_r0, nd = c_nd;
#pragma unroll
        for (int j = 0; j < CAP; ++j)
            if (j < nd && nd <= CAP) { Qs[j * RS + lane] = pq[j]; Ks[j * RS + lane] = pk[j]; Vs[j * RS + lane] = pv[j]; Gs[j * RS + lane] = pg[j]; }
        c_r0 = n_lo; c_nd = n_hi - n_lo;
        request_rows(c_r0, c_nd, (unit + stride) & 7);        // (past the end: sample 0 again, never used)
        n_lo = row_off[b2]; n_hi = row_off[b2 + 1];
        b2 = sample_of(unit + 3 * stride);
        if (nd > CAP) continue; // (only without a class list: another launch handles it)
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);
        // ---- S = Q K^T and dP = dO V^T: tile (ti, tj) = rows 16 ti .., columns 16 tj .. ----
        f32x4m S[NT][NT], dP[NT][NT];
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int tj = 0; tj < NT; ++tj) { S[ti][tj] = f32x4m{0.f, 0.f, 0.f, 0.f}; dP[ti][tj] = f32x4m{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4m q4[NT], k4[NT], g4[NT], v4[NT];
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) {
                const int o = (16 * tt + l15) * RS + 16 * kb + 4 * t;
                q4[tt] = *reinterpret_cast<const f32x4m *>(Qs + o); k4[tt] = *reinterpret_cast<const f32x4m *>(Ks + o);
                g4[tt] = *reinterpret_cast<const f32x4m *>(Gs + o); v4[tt] = *reinterpret_cast<const f32x4m *>(Vs + o);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int tj = 0; tj < NT; ++tj) {
                        S[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(q4[ti][u], k4[tj][u], S[ti][tj], 0, 0, 0);
                        dP[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(g4[ti][u], v4[tj][u], dP[ti][tj], 0, 0, 0);
                    }
        }
        // ---- softmax over the keys (column 16 tj + lane & 15) of every query row 16 ti + 4 kb + r; dS = scale * P * (dP - sum_j dP P) ----
        f32x4m P[NT][NT], dS[NT][NT];
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool rowv = 16 * ti + 4 * kb + r < nd;
                float sv[NT], mx = -INFINITY;
#pragma unroll
                for (int tj = 0; tj < NT; ++tj) { sv[tj] = (rowv && 16 * tj + l15 < nd) ? S[ti][tj][r] * scale : -INFINITY; mx = fmaxf(mx, sv[tj]); }
                mx = row16_max(mx);
                float e[NT], sum = 0.0f;
#pragma unroll
                for (int tj = 0; tj < NT; ++tj) { e[tj] = (rowv && 16 * tj + l15 < nd) ? expf(sv[tj] - mx) : 0.0f; sum += e[tj]; }
                sum = row16_sum(sum);
                const float inv = sum > 0.0f ? 1.0f / sum : 0.0f;
                float rd = 0.0f;
#pragma unroll
                for (int tj = 0; tj < NT; ++tj) { e[tj] *= inv; rd += dP[ti][tj][r] * e[tj]; } // (e = 0 where masked)
                rd = row16_sum(rd);
#pragma unroll
                for (int tj = 0; tj < NT; ++tj) {
                    const float d = scale * e[tj] * (dP[ti][tj][r] - rd);
                    P[ti][tj][r] = e[tj];
                    dS[ti][tj][r] = d;
                    dSt[(16 * ti + 4 * kb + r) * TS + 16 * tj + l15] = d;
                }
            }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);
        // ---- dV = P^T dO, dK = dS^T Q (rows = keys 16 tj ..), dQ = dS K (rows = queries 16 ti ..): four 16-feature column blocks each ----
        float *ob = d_qkv + (size_t)r0 * 1536 + head * 64 + l15;
#pragma unroll
        for (int to = 0; to < NT; ++to) {   // output row tile
            float dsT[NT][4];               // dS[16 to + lane & 15][16 tj + 4 kb + s]
#pragma unroll
            for (int tj = 0; tj < NT; ++tj)
#pragma unroll
                for (int sI = 0; sI < 4; ++sI) dsT[tj][sI] = dSt[(16 * to + l15) * TS + 16 * tj + 4 * kb + sI];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                f32x4m aq = {0.f, 0.f, 0.f, 0.f}, ak = {0.f, 0.f, 0.f, 0.f}, av = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int tc = 0; tc < NT; ++tc)  // contraction tile
#pragma unroll
                    for (int sI = 0; sI < 4; ++sI) {
                        const int ro = (16 * tc + 4 * kb + sI) * RS + 16 * cb + l15;
                        av = __builtin_amdgcn_mfma_f32_16x16x4f32(P[tc][to][sI], Gs[ro], av, 0, 0, 0);
                        ak = __builtin_amdgcn_mfma_f32_16x16x4f32(dS[tc][to][sI], Qs[ro], ak, 0, 0, 0);
                        aq = __builtin_amdgcn_mfma_f32_16x16x4f32(dsT[tc][sI], Ks[ro], aq, 0, 0, 0);
                    }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * to + 4 * kb + r;
                    if (row < nd) {
                        float *o = ob + (size_t)row * 1536 + 16 * cb;
                        o[0] = aq[r]; o[512] = ak[r]; o[1024] = av[r];
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier(); // the next unit reuses this wavefront's LDS slices
    }
}

template <int CAP>
static int launch_hh_attention_bwd(int B, const float *qkv, const int *row_off, const int *cls, int c, const float *d_out, float *d_qkv, float scale,
                                   hipStream_t st)
{
    if (CAP == 16 || CAP == 32) {
        constexpr int NT = CAP == 32 ? 2 : 1;
        const size_t per_wave = (size_t)(4 * CAP * 68 + CAP * (CAP + 1)) * sizeof(float); // 18.5 KB / 39 KB
        const int wpb = CAP == 16 ? 4 : 2, per_cu = 2;                                    // 8 / 4 wavefronts per CU
        int blocks = (B * 8 + wpb - 1) / wpb;
        if (blocks > 256 * per_cu) blocks = 256 * per_cu; // (a new cap: move tests/test_gpu_strided_grids.py, which runs past twice this one)
        if (int rc = cn_lds_opt_in<&hh_attention_bwd_mfma_kernel<NT>>(160 * 1024)) return rc;
        hipLaunchKernelGGL(hh_attention_bwd_mfma_kernel<NT>, dim3(blocks), dim3(64 * wpb), per_wave * wpb, st, B, qkv, row_off, cls + c, cls + 4 + (size_t)c * B,
                           d_out, d_qkv, scale);
        CN_CHECK_LAUNCH();
        return CN_OK;
    }
    const size_t per_wave = (size_t)(4 * CAP * 68 + (CAP <= 32 ? 4 : 2) * CAP * CAP) * sizeof(float);
    int wpb = (int)(65536 / per_wave); wpb = wpb < 1 ? 1 : (wpb > 4 ? 4 : wpb);
    int per_cu = (int)((160 * 1024) / (per_wave * wpb)); per_cu = per_cu > 8 ? 8 : (per_cu < 1 ? 1 : per_cu);
    int blocks = (B * 8 + wpb - 1) / wpb;
    if (blocks > 256 * per_cu) blocks = 256 * per_cu; // resident-sized grid walking the class list (a new cap: move tests/test_gpu_strided_grids.py)
    if (per_wave * wpb > 65536)
        if (int rc = cn_lds_opt_in<&hh_attention_bwd_kernel<CAP>>(160 * 1024)) return rc;
    hipLaunchKernelGGL(hh_attention_bwd_kernel<CAP>, dim3(blocks), dim3(64 * wpb), per_wave * wpb, st, B, qkv, row_off, cls + c, cls + 4 + (size_t)c * B,
                       d_out, d_qkv, scale);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

// Robot-human attention (EdgeAttention_M.att_func, selfAttn_srnn_temp_node.py:145-177) on the compacted rows: one
// wavefront per env.  The reference scores are t . s_j with t = temporal_edge_layer(robot) [64] and s_j =
// spatial_edge_layer(o_j) = Ws o_j + bs [64].  Since t . (Ws o_j + bs) = (Ws^T t) . o_j + t . bs and the softmax is
// invariant to the per-env constant t . bs, the kernel takes u = Ws^T t [256] and scores u . o_j directly: the
// [rows,256]x[256,64] projection of every human row (and its two backward products) is replaced by a [E,64]x[64,256]
// product per env.  masked_fill(-1e9) + softmax gives padded humans exactly zero weight (exp underflows to 0), so the
// softmax and the weighted sum run over the nd live rows only.
// (both kernels: the rows of a sample are requested eight at a time ahead of the wave-wide reductions that consume them -- as a loop of
// "load row j, reduce" every row paid its own memory round trip -- and the first eight stay in registers for the second pass: most samples
// have no more.  Same operations in the same order as the plain loops: bit-identical results.)
struct HrRows { float v[8][4]; };
__device__ __forceinline__ void hr_load8(HrRows &r, const float *__restrict__ out_sp, int r0, int j0, int nd, int lane)
{
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float *row = out_sp + (size_t)(r0 + max(min(j0 + q, nd - 1), 0)) * 256 + lane; // (rows past nd repeat the last one: loaded, never used)
#pragma unroll
        for (int c = 0; c < 4; ++c) r.v[q][c] = row[64 * c];
    }
}
__global__ __launch_bounds__(256) void hr_attention_kernel(int E, int H, float temp, const float *__restrict__ u, int u_ld, const float *__restrict__ out_sp,
                                                           const int *__restrict__ row_off, float *__restrict__ hr_out, float *__restrict__ hr_attn)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.x * 4 + wave;
    if (e >= E) return;
    const int r0 = row_off[e], nd = row_off[e + 1] - r0;
    const float *ue = u + (size_t)e * u_ld;
    const float u0 = ue[lane], u1 = ue[64 + lane], u2 = ue[128 + lane], u3 = ue[192 + lane];
    // temp: the temperature num_edges / sqrt(attention_size), formed by the host (H / 8 at the reference's attention_size = 64)
    float s = -INFINITY; // lane j holds the score of human j
    HrRows k0;
    hr_load8(k0, out_sp, r0, 0, nd, lane);
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if (q < nd) {
            const float tot = wv_sum(u0 * k0.v[q][0] + u1 * k0.v[q][1] + u2 * k0.v[q][2] + u3 * k0.v[q][3]);
            if (lane == q) s = tot * temp;
        }
    for (int j0 = 8; j0 < nd; j0 += 8) {
        HrRows r;
        hr_load8(r, out_sp, r0, j0, nd, lane);
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (j0 + q < nd) {
                const float tot = wv_sum(u0 * r.v[q][0] + u1 * r.v[q][1] + u2 * r.v[q][2] + u3 * r.v[q][3]);
                if (lane == j0 + q) s = tot * temp;
            }
    }
    const float mx = wv_max(s);
    const float p = lane < nd ? expf(s - mx) : 0.0f;
    const float denom = wv_sum(p);
    const float a = p / denom;
    if (hr_attn && lane < H) hr_attn[(size_t)e * H + lane] = a;
    float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if (q < nd) {
            const float aj = wv_readlane(a, q);
            o0 += aj * k0.v[q][0]; o1 += aj * k0.v[q][1]; o2 += aj * k0.v[q][2]; o3 += aj * k0.v[q][3];
        }
    for (int j0 = 8; j0 < nd; j0 += 8) {
        HrRows r;
        hr_load8(r, out_sp, r0, j0, nd, lane);
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (j0 + q < nd) {
                const float aj = wv_readlane(a, j0 + q);
                o0 += aj * r.v[q][0]; o1 += aj * r.v[q][1]; o2 += aj * r.v[q][2]; o3 += aj * r.v[q][3];
            }
    }
    float *o = hr_out + (size_t)e * 256;
    o[lane] = o0; o[64 + lane] = o1; o[128 + lane] = o2; o[192 + lane] = o3;
}

// Backward of hr_attention_kernel for the PPO update: one wavefront per sample on the compacted rows.
//   a_j = T (u . o_j), p = softmax(a), hr = sum_j p_j o_j         (T = temp, the forward's temperature: H / 8 at attention_size = 64)
//   dp_j = d_hr . o_j ; g_j = T p_j (dp_j - sum_k p_k dp_k) ; d_u = sum_j g_j o_j ; d_o_j = p_j d_hr + g_j u
__global__ __launch_bounds__(256) void hr_attention_bwd_kernel(int B, int H, const float *__restrict__ u, const float *__restrict__ out_sp,
                                                               const int *__restrict__ row_off, const float *__restrict__ attn,
                                                               const float *__restrict__ d_hr, float *__restrict__ d_u, float *__restrict__ d_o, int u_ld, int du_ld,
                                                               float temp)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.x * 4 + wave;
    if (e >= B) return;
    const int r0 = row_off[e], nd = row_off[e + 1] - r0;
    const float a = lane < nd ? attn[(size_t)e * H + lane] : 0.0f; // lanes = humans
    const float *g = d_hr + (size_t)e * 256, *ue = u + (size_t)e * u_ld;
    const float g0 = g[lane], g1 = g[64 + lane], g2 = g[128 + lane], g3 = g[192 + lane];
    const float u0 = ue[lane], u1 = ue[64 + lane], u2 = ue[128 + lane], u3 = ue[192 + lane];
    float dp = 0.0f;
    HrRows k0;
    hr_load8(k0, out_sp, r0, 0, nd, lane);
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if (q < nd) {
            const float tot = wv_sum(g0 * k0.v[q][0] + g1 * k0.v[q][1] + g2 * k0.v[q][2] + g3 * k0.v[q][3]);
            if (lane == q) dp = tot;
        }
    for (int j0 = 8; j0 < nd; j0 += 8) {
        HrRows r;
        hr_load8(r, out_sp, r0, j0, nd, lane);
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (j0 + q < nd) {
                const float tot = wv_sum(g0 * r.v[q][0] + g1 * r.v[q][1] + g2 * r.v[q][2] + g3 * r.v[q][3]);
                if (lane == j0 + q) dp = tot;
            }
    }
    const float dot = wv_sum(a * dp);
    const float gg = a * (dp - dot) * temp;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
    auto second = [&](const HrRows &r, int j0) {
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (j0 + q < nd) {
                const float aj = wv_readlane(a, j0 + q), gj = wv_readlane(gg, j0 + q);
                float *dor = d_o + (size_t)(r0 + j0 + q) * 256;
                d0 += gj * r.v[q][0]; d1 += gj * r.v[q][1]; d2 += gj * r.v[q][2]; d3 += gj * r.v[q][3];
                dor[lane] = aj * g0 + gj * u0; dor[64 + lane] = aj * g1 + gj * u1; dor[128 + lane] = aj * g2 + gj * u2; dor[192 + lane] = aj * g3 + gj * u3;
            }
    };
    second(k0, 0);
    for (int j0 = 8; j0 < nd; j0 += 8) {
        HrRows r;
        hr_load8(r, out_sp, r0, j0, nd, lane);
        second(r, j0);
    }
    float *du = d_u + (size_t)e * du_ld;
    du[lane] = d0; du[64 + lane] = d1; du[128 + lane] = d2; du[192 + lane] = d3;
}

} // namespace
