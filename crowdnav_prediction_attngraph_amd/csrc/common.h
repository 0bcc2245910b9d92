// Shared host/device helpers for libcrowdnav_hip.so (gfx950 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "crowdnav_hip.h"

void cn_set_error(const char *fmt, ...);

#define CN_HIP(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t cn_e_ = (expr);                                                                           \
        if (cn_e_ != hipSuccess) {                                                                           \
            cn_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(cn_e_), __FILE__, __LINE__);      \
            return CN_ERR_HIP;                                                                               \
        }                                                                                                    \
    } while (0)

#define CN_CHECK_LAUNCH() CN_HIP(hipGetLastError())

#define CN_REQUIRE(cond, ...)               \
    do {                                    \
        if (!(cond)) {                      \
            cn_set_error(__VA_ARGS__);      \
            return CN_ERR_INVALID;          \
        }                                   \
    } while (0)

// The opt-in above 64 KB of dynamic LDS (hipFuncSetAttribute) is per DEVICE: a launch site calls cn_lds_opt_in<&kernel>(bytes) in front of the
// launch, and the opt-in is repeated whenever the calling thread's current device is one that kernel has not been served on yet (a process-wide
// "done" flag left every device but the first without the attribute: the launch then fails there).  Races between threads only repeat an
// idempotent call.
template <auto Kernel> int cn_lds_opt_in(int bytes)
{
    static unsigned long long served = 0; // bit d: done on device d
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (served & (1ull << (dev & 63))) return CN_OK;
    CN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    served |= 1ull << (dev & 63);
    return CN_OK;
}

int cn_require_device();

// ---- device-side launch stamps (measurement aid: cn_prof_set_stamps / cn_prof_next_step, include/crowdnav_hip.h) ----
// One slot of CN_PROF_SLOT_WORDS uint64 per (step, kernel) = 2 x 64 sub-slots of 16 words (128 bytes: a cache line of their own each).
// Sub-slot b of the first half receives atomicMin of the 100 MHz wall clock (s_memrealtime) when workgroup b < 64 starts, sub-slot
// (workgroup & 63) of the second half atomicMax when a wavefront ends; word 1 of the slot is free for a kernel-specific count (the
// human-human kernel: live rows).  Same-address atomics serialise in the L2 at ~6 ns each -- 20 000 wavefronts stamping ONE word
// stretched a 47 us kernel to 135 us -- hence one line per sub-slot.  A kernel's duration on the device = max(ends) - min(starts) in
// 10 ns ticks, and since the clock is global the slots of a step also give its timeline (gaps, overlaps).  NULL = no stamping.
enum { CN_K_ENV_STEP = 0, CN_K_ORCA_LANE = 1, CN_K_HH_FUSED = 2, CN_K_RN_FUSED = 3, CN_K_ORCA_LP3 = 4, CN_K_PREGEN = 5, CN_K_ROW_PLAN = 6, CN_K_OTHER = 7 };
unsigned long long *cn_stamp_slot(int kernel_id); // host: the current step's slot of `kernel_id`, or NULL (off, masked out, ring exhausted)

#ifdef __HIPCC__
struct CnStampScope {
    unsigned long long *s;
    unsigned blk;   // the block's index within ITS part of the launch (a launch that hosts two kernels' work stamps each part from 0)
    __device__ __forceinline__ explicit CnStampScope(unsigned long long *slot, int block = -1) : s(slot), blk(block < 0 ? blockIdx.x : (unsigned)block)
    {
        if (s && threadIdx.x == 0) {
            const unsigned long long now = (unsigned long long)wall_clock64();
            if (blk < 64) atomicMin(s + blk * 16, now);
            atomicMax(s + (blk & 63) * 16 + 8, now);   // latest first instruction among the workgroups b with b & 63 == slot
        }
    }
    __device__ __forceinline__ ~CnStampScope()
    {
        if (s && (threadIdx.x & 63) == 0) atomicMax(s + (64 + (blk & 63)) * 16, (unsigned long long)wall_clock64());
    }
};
#endif

#define CN_WAVE 64

// ---- wave-level primitives (64 lanes) ----
// A value that was loaded ahead of its use: what is computed from it stays below this point (the compiler otherwise hoists the first
// operation on it -- a conversion, a readfirstlane -- up to the load and waits for the load there).
template <class T> __device__ __forceinline__ T held(T v) { asm volatile("" : "+v"(v)); return v; }
// ... of a wave-uniform value: from here on it lives in scalar registers
template <class T> __device__ __forceinline__ T held_uniform(T v)
{
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "held_uniform: one or two words");
    v = held(v);
    int w[sizeof(T) / 4];
    __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) / 4); ++k) w[k] = __builtin_amdgcn_readfirstlane(w[k]);
    __builtin_memcpy(&v, w, sizeof(T));
    return v;
}

// tanh(x) = 1 - 2 / (1 + e^{2x}) and the sigmoid on v_exp_f32: absolute error < 3e-7 (e^{2x} overflows to inf -> 1, underflows to 0 -> -1)
__device__ __forceinline__ float fast_tanh(float x)
{
    const float e = __builtin_amdgcn_exp2f(x * 2.88539008177792681472f); // 2 * log2(e)
    return 1.0f - 2.0f / (1.0f + e);
}
__device__ __forceinline__ float fast_sigmoid(float x) { return 1.0f / (1.0f + __builtin_amdgcn_exp2f(x * -1.44269504088896340736f)); }

__device__ __forceinline__ float wv_readlane(float x, int lane_uniform)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane_uniform));
}
// DPP reductions (gfx9 family): row_shr 1/2/4/8 leave each 16-lane row's result in its last lane, row_bcast:15 and
// row_bcast:31 fold the rows, lane 63 holds the wave result, one v_readlane broadcasts it.  7 VALU ops instead of six
// ds_bpermute round trips.  Lanes without a DPP source keep `identity` (bound_ctrl = 0 -> `old` operand).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float wv_dpp(float v, float identity)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(identity), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wv_min(float v)
{
    const float I = __builtin_inff();
    v = fminf(v, wv_dpp<0x111, 0xf>(v, I));
    v = fminf(v, wv_dpp<0x112, 0xf>(v, I));
    v = fminf(v, wv_dpp<0x114, 0xf>(v, I));
    v = fminf(v, wv_dpp<0x118, 0xf>(v, I));
    v = fminf(v, wv_dpp<0x142, 0xa>(v, I));
    v = fminf(v, wv_dpp<0x143, 0xc>(v, I));
    return wv_readlane(v, 63);
}
__device__ __forceinline__ float wv_max(float v)
{
    const float I = -__builtin_inff();
    v = fmaxf(v, wv_dpp<0x111, 0xf>(v, I));
    v = fmaxf(v, wv_dpp<0x112, 0xf>(v, I));
    v = fmaxf(v, wv_dpp<0x114, 0xf>(v, I));
    v = fmaxf(v, wv_dpp<0x118, 0xf>(v, I));
    v = fmaxf(v, wv_dpp<0x142, 0xa>(v, I));
    v = fmaxf(v, wv_dpp<0x143, 0xc>(v, I));
    return wv_readlane(v, 63);
}
__device__ __forceinline__ float wv_sum(float v)
{
    // Hillis-Steele inside each 16-lane row (row_shr 1,2,4,8), then fold the rows; total lands in lane 63
    v += wv_dpp<0x111, 0xf>(v, 0.0f);
    v += wv_dpp<0x112, 0xf>(v, 0.0f);
    v += wv_dpp<0x114, 0xf>(v, 0.0f);
    v += wv_dpp<0x118, 0xf>(v, 0.0f);
    v += wv_dpp<0x142, 0xa>(v, 0.0f);
    v += wv_dpp<0x143, 0xc>(v, 0.0f);
    return wv_readlane(v, 63);
}
__device__ __forceinline__ double wv_readlane_d(double v, int lane_uniform)
{
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b & 0xffffffffll), lane_uniform);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)b >> 32), lane_uniform);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// the same DPP steps on the two halves of a double (both halves move with one control word, so a lane always sees a whole operand)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double wv_dpp(double v, double identity)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v), id = (unsigned long long)__double_as_longlong(identity);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)id, (int)(unsigned)b, CTRL, ROW_MASK, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)(id >> 32), (int)(unsigned)(b >> 32), CTRL, ROW_MASK, 0xf, false);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// min is order-independent (no NaN operands here), so the fp64 minimum may take the DPP tree of the fp32 one: 12 DPP moves, 6 v_min_f64
// and two v_readlane instead of 12 ds_bpermute round trips.  Every lane of the wavefront must be active.  The result is wave-uniform.
// (Sums keep the xor butterfly below: their association is part of the bits.)
__device__ __forceinline__ double wv_min_dpp(double v)
{
    const double I = __builtin_inf();
    v = fmin(v, wv_dpp<0x111, 0xf>(v, I));
    v = fmin(v, wv_dpp<0x112, 0xf>(v, I));
    v = fmin(v, wv_dpp<0x114, 0xf>(v, I));
    v = fmin(v, wv_dpp<0x118, 0xf>(v, I));
    v = fmin(v, wv_dpp<0x142, 0xa>(v, I));
    v = fmin(v, wv_dpp<0x143, 0xc>(v, I));
    return wv_readlane_d(v, 63);
}
__device__ __forceinline__ double wv_min(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wv_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
