// mt19937.h -- numpy's legacy RandomState (MT19937) for the simulator: the per-env stream staged in LDS, its wave-uniform draws
// (uniform, normal, randint) and the tempering that the placement loops apply to raw stream words.  Part of env_sim.hip's
// translation unit.
#pragma once
#include "env_dev.h"
#include "det_math.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// MT19937 (numpy legacy RandomState) staged in LDS, wave-uniform draws.  The state belongs to ONE wavefront (R.mt: the block's array in the
// one-wavefront kernels, a per-wavefront slice in the ORCA tail kernel that also hosts the episode generator), so everything that orders its
// LDS traffic is wave-level: LDS operations of a wavefront are executed in issue order, the fence only keeps the compiler from moving them.
// ------------------------------------------------------------------------------------------------------------------
__shared__ uint32_t g_mt_lds[MT_N]; // the staged MT19937 state of a one-wavefront block
struct Rng {
    int pos;
    bool loaded;
    uint32_t *mt = g_mt_lds;
    bool pre_ok = false; // rng_prefetch: the state is on its way into mt, its position into pre_pos
    int pre_pos = 0;
};
__device__ __forceinline__ void rng_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// The 624 words of one stream, global -> LDS without passing through registers (global_load_lds_dword: lane l of chunk t lands at
// dst[64 t + l], the stream's own order).  Nothing waits here: the copy runs beside whatever follows until mt_dma_wait().
__device__ __forceinline__ void mt_dma(uint32_t *dst, const uint32_t *src, int lane)
{
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    typedef __attribute__((address_space(1))) const uint32_t glb_u32;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the wavefront's earlier LDS traffic on dst has landed
#pragma unroll
    for (int t = 0; t < (MT_N + 63) / 64; ++t)
        if (lane + 64 * t < MT_N) __builtin_amdgcn_global_load_lds((glb_u32 *)(src + lane + 64 * t), (lds_u32 *)(dst + 64 * t), 4, 0, 0);
}
__device__ __forceinline__ void mt_dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// a wavefront that knows it will draw fetches its stream early; the rng_load at the first draw then only waits for it
template <class S>
__device__ __forceinline__ void rng_prefetch(Rng &R, const S &s, int e, int lane)
{
    if (R.loaded || R.pre_ok) return;
    mt_dma(R.mt, s.mt + (size_t)e * MT_N, lane);
    R.pre_pos = s.mt_pos[e];
    R.pre_ok = true;
}
template <class S>
__device__ __forceinline__ void rng_load(Rng &R, const S &s, int e, int lane)
{
    if (R.loaded) return;
    if (R.pre_ok) {
        mt_dma_wait();
        R.pos = held(R.pre_pos);
    } else {
        for (int k = lane; k < MT_N; k += 64) R.mt[k] = s.mt[(size_t)e * MT_N + k];
        R.pos = s.mt_pos[e];
    }
    R.loaded = true;
    rng_sync();
}
template <class S>
__device__ __forceinline__ void rng_store(Rng &R, const S &s, int e, int lane)
{
    if (!R.loaded) return;
    rng_sync();
    for (int k = lane; k < MT_N; k += 64) s.mt[(size_t)e * MT_N + k] = R.mt[k];
    if (lane == 0) s.mt_pos[e] = R.pos;
}
// np.random.seed(int) == init_genrand: serial recurrence, computed redundantly by all lanes (wave-uniform)
__device__ __forceinline__ void rng_seed(Rng &R, uint32_t seed, int lane)
{
    rng_sync();
    // (the seed comes out of vector loads: without this the 624-step chain runs on the vector ALU -- shift, xor, a quarter-rate 32-bit
    // multiply and an add per step, ~13 us -- instead of four scalar instructions)
    uint32_t sd = (uint32_t)__builtin_amdgcn_readfirstlane((int)seed);
    for (int base = 0; base < MT_N; base += 64) {
        uint32_t mine = 0;
        for (int t = 0; t < 64; ++t) {
            const int pos = base + t;
            if (pos < MT_N) {
                if (t == lane) mine = sd;
                sd = 1812433253u * (sd ^ (sd >> 30)) + (uint32_t)pos + 1u;
            }
        }
        if (base + lane < MT_N) R.mt[base + lane] = mine;
    }
    R.pos = MT_N;
    R.loaded = true;
    rng_sync();
}
__device__ __forceinline__ uint32_t mt_mix(uint32_t a, uint32_t b, uint32_t c)
{
    const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
    return c ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}
// lane-parallel regeneration of the 624-word block; dependencies are at distance 227 (>= 64), so 64-wide chunks
// processed in order reproduce the sequential recurrence exactly.
__device__ __forceinline__ void mt_twist_buf(uint32_t *k, int lane)
{
    rng_sync();
    for (int base = 0; base < 227; base += 64) {
        const int i = base + lane;
        const bool act = i < 227;
        uint32_t a = 0, b = 0, c = 0;
        if (act) { a = k[i]; b = k[i + 1]; c = k[i + 397]; }
        rng_sync();
        if (act) k[i] = mt_mix(a, b, c);
        rng_sync();
    }
    for (int base = 227; base < 623; base += 64) {
        const int i = base + lane;
        const bool act = i < 623;
        uint32_t a = 0, b = 0, c = 0;
        if (act) { a = k[i]; b = k[i + 1]; c = k[i - 227]; }
        rng_sync();
        if (act) k[i] = mt_mix(a, b, c);
        rng_sync();
    }
    if (lane == 0) k[623] = mt_mix(k[623], k[0], k[396]);
    rng_sync();
}
__device__ __forceinline__ void rng_twist(Rng &R, int lane)
{
    mt_twist_buf(R.mt, lane);
    R.pos = 0;
}
__device__ __forceinline__ uint32_t rng_u32(Rng &R, int lane)
{
    if (R.pos == MT_N) rng_twist(R, lane);
    uint32_t y = R.mt[R.pos++];
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
}
// random_sample(): 53-bit double from two words
__device__ __forceinline__ double rng_double(Rng &R, int lane)
{
    const uint32_t a = rng_u32(R, lane) >> 5, b = rng_u32(R, lane) >> 6;
    return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
}
__device__ __forceinline__ double rng_uniform(Rng &R, int lane, double lo, double hi) { return lo + (hi - lo) * rng_double(R, lane); }
// np.random.normal(loc, scale) of the legacy RandomState: loc + scale * legacy_gauss (polar Box-Muller, the second deviate of a pair is
// cached for the next call).  gauss / has_gauss are the caller's copies of the cache (wave-uniform).
__device__ __forceinline__ double rng_normal(Rng &R, int lane, double loc, double scale, double &gauss, bool &has_gauss)
{
    double g;
    if (has_gauss) { g = gauss; has_gauss = false; gauss = 0.0; }
    else {
        double x1, x2, r2;
        do {
            x1 = 2.0 * rng_double(R, lane) - 1.0;
            x2 = 2.0 * rng_double(R, lane) - 1.0;
            r2 = x1 * x1 + x2 * x2;
        } while (r2 >= 1.0 || r2 == 0.0);
        const double f = sqrt(-2.0 * det_log(r2) / r2);
        gauss = f * x1; has_gauss = true;
        g = f * x2;
    }
    return loc + scale * g;
}
// legacy RandomState.randint(low, high), default int64 dtype (numpy/random/_bounded_integers: _rand_int64 -> masked rejection on 32-bit
// words): no draw when the range is a single value
__device__ __forceinline__ int rng_randint(Rng &R, int lane, int low, int high)
{
    const uint32_t rng = (uint32_t)(high - 1 - low);
    if (rng == 0) return low;
    uint32_t mask = rng;
    mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
    uint32_t v;
    do { v = rng_u32(R, lane) & mask; } while (v > rng);
    return low + (int)v;
}

__device__ __forceinline__ uint32_t mt_temper(uint32_t y)
{
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
}

} // namespace
