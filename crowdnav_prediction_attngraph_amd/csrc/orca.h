// orca.h -- ORCA for the simulator's humans: RVO2's linear programs in two wave-cooperative forms (lp*_wave: one program per
// wavefront, lp*_pair: two), the step's solve kernels (orca_lane_kernel + orca_lp3_kernel, orca_kernel), the 'truth' roll-outs
// (orca_truth_kernel, sf_truth_kernel) and the stand-alone orca_solve_kernel.  Part of env_sim.hip's translation unit.
#pragma once
#include "env_dev.h"
#include "det_math.h"
#include <type_traits>

namespace {

// ------------------------------------------------------------------------------------------------------------------
// Wave-cooperative RVO2 linear programs.  Lane k holds line k = (point, direction); `valid` marks live lines
// (bit k).  All scalars (result, t bounds, ...) are wave-uniform: every lane computes them identically.
// RVO2 v2.0.2 Agent.cpp linearProgram1/2/3; call site crowd_nav/policy/orca.py:113 (doStep).
// ------------------------------------------------------------------------------------------------------------------
struct LpLine { float px, py, dx, dy; };

__device__ __forceinline__ bool wv_any(bool p) { return __ballot(p) != 0ull; }

// Optimise along line i subject to the disc and to every earlier valid line (lane-parallel clip).  Returns success.
__device__ __forceinline__ bool lp1_wave(const LpLine &L, uint64_t valid, int i, float ipx, float ipy, float idx, float idy,
                                         float radius, float optx, float opty, bool dirOpt, int lane, float &rx, float &ry)
{
    const float dotProduct = ipx * idx + ipy * idy;
    const float discriminant = dotProduct * dotProduct + radius * radius - (ipx * ipx + ipy * ipy);
    if (discriminant < 0.0f) return false;
    const float sq = sqrtf(discriminant);
    float tLeft = -dotProduct - sq;
    float tRight = -dotProduct + sq;
    const bool mine = lane < i && ((valid >> lane) & 1ull);
    const float denominator = idx * L.dy - idy * L.dx;
    const float numerator = L.dx * (ipy - L.py) - L.dy * (ipx - L.px);
    const bool parallel = fabsf(denominator) <= RVO_EPS;
    const bool pfail = mine && parallel && numerator < 0.0f;
    const float t = numerator / denominator;
    const float candR = (mine && !parallel && denominator >= 0.0f) ? t : INFINITY;
    const float candL = (mine && !parallel && denominator < 0.0f) ? t : -INFINITY;
    tRight = fminf(tRight, wv_min(candR));
    tLeft = fmaxf(tLeft, wv_max(candL));
    // sequential RVO2 fails at the first prefix with tLeft > tRight or a parallel infeasible line; bounds are monotone,
    // so "any prefix fails" == "final bounds cross or any parallel line fails".
    if (wv_any(pfail) || tLeft > tRight) return false;
    float t_opt;
    if (dirOpt) {
        t_opt = (optx * idx + opty * idy > 0.0f) ? tRight : tLeft;
    } else {
        const float tt = idx * (optx - ipx) + idy * (opty - ipy);
        t_opt = tt < tLeft ? tLeft : (tt > tRight ? tRight : tt);
    }
    rx = ipx + t_opt * idx;
    ry = ipy + t_opt * idy;
    return true;
}

// Returns n on success, else the index of the line that failed.  RVO2 walks the lines in order and re-optimises at every
// line the current result violates; lines it does not violate are no-ops, so the walk jumps from violated line to
// violated line: every lane tests its own line against the current result, a ballot + ffs finds the next one.
__device__ __forceinline__ int lp2_wave(const LpLine &L, uint64_t valid, int n, float radius, float optx, float opty,
                                        bool dirOpt, int lane, float &rx, float &ry)
{
    if (dirOpt) {
        rx = radius * optx; ry = radius * opty;
    } else if (optx * optx + opty * opty > radius * radius) {
        const float inv = 1.0f / sqrtf(optx * optx + opty * opty);
        rx = radius * (optx * inv); ry = radius * (opty * inv);
    } else {
        rx = optx; ry = opty;
    }
    uint64_t todo = valid & (n >= 64 ? ~0ull : ((1ull << n) - 1ull));
    for (;;) {
        const uint64_t vm = __ballot(L.dx * (L.py - ry) - L.dy * (L.px - rx) > 0.0f) & todo;
        if (!vm) return n;
        const int i = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)vm) - 1);
        todo &= ~((2ull << i) - 1ull); // lines 0..i are behind us
        const float ipx = wv_readlane(L.px, i), ipy = wv_readlane(L.py, i);
        const float idx = wv_readlane(L.dx, i), idy = wv_readlane(L.dy, i);
        const float tx = rx, ty = ry;
        if (!lp1_wave(L, valid, i, ipx, ipy, idx, idy, radius, optx, opty, dirOpt, lane, rx, ry)) {
            rx = tx; ry = ty;
            return i;
        }
    }
}

__device__ __forceinline__ void lp3_wave(const LpLine &L, int n, int beginLine, float radius, int lane, float &rx, float &ry)
{
    float distance = 0.0f;
    uint64_t todo = (n >= 64 ? ~0ull : ((1ull << n) - 1ull)) & ~((1ull << beginLine) - 1ull);
    for (;;) {
        const uint64_t vm = __ballot(L.dx * (L.py - ry) - L.dy * (L.px - rx) > distance) & todo;
        if (!vm) return;
        const int i = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)vm) - 1);
        todo &= ~((2ull << i) - 1ull);
        const float ipx = wv_readlane(L.px, i), ipy = wv_readlane(L.py, i);
        const float idx = wv_readlane(L.dx, i), idy = wv_readlane(L.dy, i);
        // every lane j < i projects its line onto line i (RVO2 builds projLines sequentially; same set, same order)
        LpLine Pj;
        const float determinant = idx * L.dy - idy * L.dx;
        const bool par = fabsf(determinant) <= RVO_EPS;
        const bool skip = par && (idx * L.dx + idy * L.dy > 0.0f);
        if (par) {
            Pj.px = 0.5f * (ipx + L.px); Pj.py = 0.5f * (ipy + L.py);
        } else {
            const float s = (L.dx * (ipy - L.py) - L.dy * (ipx - L.px)) / determinant;
            Pj.px = ipx + s * idx; Pj.py = ipy + s * idy;
        }
        const float ddx = L.dx - idx, ddy = L.dy - idy;
        const float inv = 1.0f / sqrtf(ddx * ddx + ddy * ddy);
        Pj.dx = ddx * inv; Pj.dy = ddy * inv;
        const uint64_t pvalid = __ballot(lane < i && !skip);
        const float tx = rx, ty = ry;
        if (lp2_wave(Pj, pvalid, i, radius, -idy, idx, true, lane, rx, ry) < i) { rx = tx; ry = ty; }
        distance = idx * (ipy - ry) - idy * (ipx - rx);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// linearProgram3 for TWO programs per wavefront: lanes 0..31 hold the lines of one, lanes 32..63 those of another (at most 32 lines
// each: the lane kernel's limit).  Per program the arithmetic is lp3_wave's; what is wave-uniform there (the result, the bounds, the
// index of the line being processed) is uniform per HALF here and lives in vector registers, each half's walk is predicated on its
// own state, and a loop ends when both halves are through.  hl = lane & 31.
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t hw_ballot(bool p, int lane)
{
    const uint64_t b = __ballot(p);
    return (lane & 32) ? (uint32_t)(b >> 32) : (uint32_t)b;
}
__device__ __forceinline__ float hw_read(float v, int lane, int i) // v of lane i of this lane's half (i uniform per half)
{
    return __int_as_float(__builtin_amdgcn_ds_bpermute(((lane & 32) + i) << 2, __float_as_int(v)));
}
__device__ __forceinline__ float hw_last(float v, int lane) // lanes 31 / 63 -> every lane of their half
{
    const float a = wv_readlane(v, 31), b = wv_readlane(v, 63);
    return (lane & 32) ? b : a;
}
// Minimum / maximum over a half.  The tree runs on order-preserving integer keys (key(a) < key(b) <=> a < b, -0 below +0 as v_min_f32 has
// it; no NaN operands here): an unsigned minimum takes its DPP operand itself, one instruction per step, where a float step is four
// (identity, DPP move, canonicalise, minimum).  Minimum and maximum do not depend on the order of their operands: hw_unkey of the result has
// the bits of the fminf / fmaxf tree.
__device__ __forceinline__ uint32_t hw_key(float f)
{
    const uint32_t u = __float_as_uint(f);
    return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}
__device__ __forceinline__ float hw_unkey(uint32_t k) { return __uint_as_float(k ^ ((uint32_t)((int32_t)~k >> 31) | 0x80000000u)); }
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t hw_dpp(uint32_t v, uint32_t identity)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ uint32_t hw_min(uint32_t v, int lane) // keys in, key out
{
    v = min(v, hw_dpp<0x111, 0xf>(v, ~0u));
    v = min(v, hw_dpp<0x112, 0xf>(v, ~0u));
    v = min(v, hw_dpp<0x114, 0xf>(v, ~0u));
    v = min(v, hw_dpp<0x118, 0xf>(v, ~0u));
    v = min(v, hw_dpp<0x142, 0xa>(v, ~0u)); // row_bcast:15 into rows 1 and 3: lane 31 = lanes 0..31, lane 63 = lanes 32..63
    return __float_as_uint(hw_last(__uint_as_float(v), lane));
}
__device__ __forceinline__ uint32_t hw_max(uint32_t v, int lane)
{
    v = max(v, hw_dpp<0x111, 0xf>(v, 0u));
    v = max(v, hw_dpp<0x112, 0xf>(v, 0u));
    v = max(v, hw_dpp<0x114, 0xf>(v, 0u));
    v = max(v, hw_dpp<0x118, 0xf>(v, 0u));
    v = max(v, hw_dpp<0x142, 0xa>(v, 0u));
    return __float_as_uint(hw_last(__uint_as_float(v), lane));
}

// What linearProgram1 on line i computes from line i alone: its chord of the disc (the bounds before any clip, whether there is one) and
// which end the direction of optimisation picks.  Every lane works this out for ITS line once, when the lines are set up; a clip on line
// i fetches lane i's.  The same operations on the same operands as in lp1_wave, done once per line instead of once per clip by 32 lanes.
struct LpChord { uint32_t kLeft, kRight, inDisc, pickRight; }; // the bounds as keys (hw_key); masks: bit k = line k, uniform per half

__device__ __forceinline__ LpChord lp_chords(const LpLine &L, float radius, float optx, float opty, int lane)
{
    LpChord c;
    const float dotProduct = L.px * L.dx + L.py * L.dy;
    const float discriminant = dotProduct * dotProduct + radius * radius - (L.px * L.px + L.py * L.py);
    const float sq = sqrtf(discriminant);
    c.kLeft = hw_key(-dotProduct - sq);
    c.kRight = hw_key(-dotProduct + sq);
    c.inDisc = hw_ballot(!(discriminant < 0.0f), lane);
    c.pickRight = hw_ballot(optx * L.dx + opty * L.dy > 0.0f, lane);
    return c;
}

// lp1_wave with dirOpt = true for both halves at once; commits the new result only where `act` and the program is feasible
__device__ __forceinline__ bool lp1_pair(const LpLine &L, const LpChord &C, uint32_t valid, int i, float ipx, float ipy, float idx, float idy,
                                         bool act, int lane, float &rx, float &ry)
{
    const int hl = lane & 31;
    bool ok = (C.inDisc >> i) & 1u;
    const uint32_t kLeft = __float_as_uint(hw_read(__uint_as_float(C.kLeft), lane, i));
    const uint32_t kRight = __float_as_uint(hw_read(__uint_as_float(C.kRight), lane, i));
    const bool mine = hl < i && ((valid >> hl) & 1u);
    const float denominator = idx * L.dy - idy * L.dx;
    const float numerator = L.dx * (ipy - L.py) - L.dy * (ipx - L.px);
    const bool parallel = fabsf(denominator) <= RVO_EPS;
    const bool pfail = mine && parallel && numerator < 0.0f;
    const float t = numerator / denominator;
    const uint32_t kt = hw_key(t);
    const uint32_t candR = (mine && !parallel && denominator >= 0.0f) ? kt : 0xff800000u; // key(+inf)
    const uint32_t candL = (mine && !parallel && denominator < 0.0f) ? kt : 0x007fffffu;  // key(-inf)
    const float tRight = hw_unkey(min(kRight, hw_min(candR, lane)));
    const float tLeft = hw_unkey(max(kLeft, hw_max(candL, lane)));
    const uint32_t pf = hw_ballot(pfail, lane); // (every cross-lane operation of these routines sits outside their predicated parts)
    ok = ok & (pf == 0u) & !(tLeft > tRight);
    const float t_opt = ((C.pickRight >> i) & 1u) ? tRight : tLeft;
    if (act && ok) {
        rx = ipx + t_opt * idx;
        ry = ipy + t_opt * idy;
    }
    return ok;
}

// lp2_wave with dirOpt = true over the lines 0 .. n-1 of each half (n, radius, opt uniform per half).  Returns n or the failing line.
__device__ __forceinline__ int lp2_pair(const LpLine &L, uint32_t valid, int n, float radius, float optx, float opty, bool act, int lane,
                                        float &rx, float &ry)
{
    if (act) { rx = radius * optx; ry = radius * opty; }
    const LpChord C = lp_chords(L, radius, optx, opty, lane);
    uint32_t todo = valid & ((1u << n) - 1u); // n <= 31: line n itself is the one being projected on
    int res = n;
    bool running = act;
    for (;;) {
        const uint32_t vm = hw_ballot(L.dx * (L.py - ry) - L.dy * (L.px - rx) > 0.0f, lane) & todo;
        const bool go = running && vm != 0u;
        if (__ballot(go) == 0ull) return res;
        running = go; // a half without a violated line left is through
        const int i = go ? __ffs((int)vm) - 1 : 0;
        if (go) todo &= ~((2u << i) - 1u);
        const float ipx = hw_read(L.px, lane, i), ipy = hw_read(L.py, lane, i);
        const float idx = hw_read(L.dx, lane, i), idy = hw_read(L.dy, lane, i);
        const bool ok = lp1_pair(L, C, valid, i, ipx, ipy, idx, idy, go, lane, rx, ry);
        if (go && !ok) { res = i; running = false; } // (lp1_pair left the result alone)
    }
}

__device__ __forceinline__ void lp3_pair(const LpLine &L, int n, int beginLine, float radius, bool act, int lane, float &rx, float &ry)
{
    const int hl = lane & 31;
    float distance = 0.0f;
    uint32_t todo = (n >= 32 ? ~0u : ((1u << n) - 1u)) & ~((1u << beginLine) - 1u);
    bool running = act;
    for (;;) {
        const uint32_t vm = hw_ballot(L.dx * (L.py - ry) - L.dy * (L.px - rx) > distance, lane) & todo;
        const bool go = running && vm != 0u;
        if (__ballot(go) == 0ull) return;
        running = go;
        const int i = go ? __ffs((int)vm) - 1 : 0;
        if (go) todo &= ~((2u << i) - 1u);
        const float ipx = hw_read(L.px, lane, i), ipy = hw_read(L.py, lane, i);
        const float idx = hw_read(L.dx, lane, i), idy = hw_read(L.dy, lane, i);
        LpLine Pj;
        const float determinant = idx * L.dy - idy * L.dx;
        const bool par = fabsf(determinant) <= RVO_EPS;
        const bool skip = par && (idx * L.dx + idy * L.dy > 0.0f);
        if (par) {
            Pj.px = 0.5f * (ipx + L.px); Pj.py = 0.5f * (ipy + L.py);
        } else {
            const float s = (L.dx * (ipy - L.py) - L.dy * (ipx - L.px)) / determinant;
            Pj.px = ipx + s * idx; Pj.py = ipy + s * idy;
        }
        const float ddx = L.dx - idx, ddy = L.dy - idy;
        const float inv = 1.0f / sqrtf(ddx * ddx + ddy * ddy);
        Pj.dx = ddx * inv; Pj.dy = ddy * inv;
        const uint32_t pvalid = hw_ballot(hl < i && !skip, lane);
        const float tx = rx, ty = ry;
        const int f = lp2_pair(Pj, pvalid, i, radius, -idy, idx, go, lane, rx, ry);
        if (go && f < i) { rx = tx; ry = ty; }
        if (go) distance = idx * (ipy - ry) - idy * (ipx - rx);
    }
}

// the agents orca_lane_kernel could not finish (infeasible program -> linearProgram3): two per wavefront, lane k of a half = line k
__global__ __launch_bounds__(256) void orca_lp3_kernel(EnvDev s)
{
    const CnStampScope stamp_scope(s.stamp);
    const int lane = threadIdx.x & 63, hl = lane & 31, half = lane >> 5;
    const int total = *s.lp3_cnt;
    const int pairs = (total + 1) >> 1;
    const int H = s.H;
    for (int p = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); p < pairs; p += gridDim.x * 4) {
        const bool act = 2 * p + half < total;
        const int k = act ? 2 * p + half : 2 * p; // (an odd list: the upper half of the last wavefront idles on a copy of the lower one's data)
        // (header and line in one round trip: all 32 line slots of a listed agent are allocated, the ones past nn hold stale lines)
        const Lp3Hdr hd = s.lp3_hdr[k];
        float4 raw = s.lp3_lines[(size_t)k * 32 + hl];
        raw.x = held(raw.x); raw.y = held(raw.y); raw.z = held(raw.z); raw.w = held(raw.w); // (or the load sinks behind the test of nn again)
        const float4 ln = hl < hd.nn ? raw : make_float4(0.0f, 0.0f, 1.0f, 0.0f);
        LpLine L;
        L.px = ln.x; L.py = ln.y; L.dx = ln.z; L.dy = ln.w;
        float rx = hd.rx, ry = hd.ry;
        lp3_pair(L, hd.nn, hd.line_fail, hd.radius, act, lane, rx, ry);
        if (act && hl == 0) {
            const int e = hd.agent / H, i = hd.agent - e * H;
            s.hact[(size_t)e * 2 * H + i] = rx;
            s.hact[(size_t)e * 2 * H + H + i] = ry;
        }
    }
}

// One agent's new velocity.  Lane j < nl holds candidate neighbour j (cand == true) in index order.
// RVO2 Agent::computeNeighbors (range filter, ascending distSq, at most maxNeighbors) + computeNewVelocity.
__device__ __forceinline__ void orca_wave(int lane, int nl, bool cand, float opx, float opy, float ovx, float ovy, float orad,
                                          float spx, float spy, float svx, float svy, float srad, float maxspeed, float prefx,
                                          float prefy, float nd, int max_nb, float th, float dt, float &outx, float &outy)
{
    // neighbour selection: key = distSq if within range else +inf; rank by (key, index) -> stable ascending order
    const float ddx0 = spx - opx, ddy0 = spy - opy;
    const float dq = ddx0 * ddx0 + ddy0 * ddy0;
    const bool inrange = cand && dq < nd * nd;
    const float key = inrange ? dq : INFINITY;
    int rank = 0;
    for (int m = 0; m < nl; ++m) {
        const float km = wv_readlane(key, m);
        rank += (km < key || (km == key && m < lane)) ? 1 : 0;
    }
    if (lane >= nl) rank = lane;
    int nn = __popcll(__ballot(inrange));
    if (nn > max_nb) nn = max_nb;
    // ORCA half-plane of this lane's neighbour
    const float rpx = opx - spx, rpy = opy - spy;   // relativePosition
    const float rvx = svx - ovx, rvy = svy - ovy;   // relativeVelocity
    const float distSq = rpx * rpx + rpy * rpy;
    const float cr = srad + orad;
    const float crSq = cr * cr;
    float ldx, ldy, ux, uy;
    if (distSq > crSq) {
        const float invTH = 1.0f / th;
        const float wx = rvx - invTH * rpx, wy = rvy - invTH * rpy;
        const float wLenSq = wx * wx + wy * wy;
        const float dot1 = wx * rpx + wy * rpy;
        if (dot1 < 0.0f && dot1 * dot1 > crSq * wLenSq) {
            const float wLen = sqrtf(wLenSq);
            const float inv = 1.0f / wLen;
            const float uwx = wx * inv, uwy = wy * inv;
            ldx = uwy; ldy = -uwx;
            const float s = cr * invTH - wLen;
            ux = s * uwx; uy = s * uwy;
        } else {
            const float leg = sqrtf(distSq - crSq);
            const float invD = 1.0f / distSq;
            if (rpx * wy - rpy * wx > 0.0f) {
                ldx = (rpx * leg - rpy * cr) * invD;
                ldy = (rpx * cr + rpy * leg) * invD;
            } else {
                ldx = -((rpx * leg + rpy * cr) * invD);
                ldy = -((-rpx * cr + rpy * leg) * invD);
            }
            const float dot2 = rvx * ldx + rvy * ldy;
            ux = dot2 * ldx - rvx; uy = dot2 * ldy - rvy;
        }
    } else {
        const float invDT = 1.0f / dt;
        const float wx = rvx - invDT * rpx, wy = rvy - invDT * rpy;
        const float wLen = sqrtf(wx * wx + wy * wy);
        const float inv = 1.0f / wLen;
        const float uwx = wx * inv, uwy = wy * inv;
        ldx = uwy; ldy = -uwx;
        const float s = cr * invDT - wLen;
        ux = s * uwx; uy = s * uwy;
    }
    const float lpx = svx + 0.5f * ux, lpy = svy + 0.5f * uy;
    // scatter lines into sorted order: lane `rank` receives this lane's line
    LpLine L;
    L.px = __int_as_float(__builtin_amdgcn_ds_permute(rank << 2, __float_as_int(lpx)));
    L.py = __int_as_float(__builtin_amdgcn_ds_permute(rank << 2, __float_as_int(lpy)));
    L.dx = __int_as_float(__builtin_amdgcn_ds_permute(rank << 2, __float_as_int(ldx)));
    L.dy = __int_as_float(__builtin_amdgcn_ds_permute(rank << 2, __float_as_int(ldy)));
    const uint64_t valid = nn >= 64 ? ~0ull : ((1ull << nn) - 1ull);
    float rx, ry;
    const int lineFail = lp2_wave(L, valid, nn, maxspeed, prefx, prefy, false, lane, rx, ry);
    if (lineFail < nn) lp3_wave(L, nn, lineFail, maxspeed, lane, rx, ry);
    outx = rx; outy = ry;
}

// ------------------------------------------------------------------------------------------------------------------
// ORCA for every human of every env.  crowd_sim.py:680-703 get_human_actions + crowd_nav/policy/orca.py:64-117.
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void orca_agent(const EnvDev &s, int agent, int lane)
{
    const int H = s.H;
    const int e = agent / H, i = agent - e * H;
    const int n = crowd_size(s, e); // humans present (== H unless sim.human_num_range > 0)
    if (i >= n) return;
    const double *hum = s.hum + (size_t)e * 8 * H;
    const bool isH = lane < n;
    const int lj = isH ? lane : 0;
    const double px = hum[F_PX * H + lj], py = hum[F_PY * H + lj], vx = hum[F_VX * H + lj], vy = hum[F_VY * H + lj];
    const double rad = hum[F_RAD * H + lj];
    // self (lane i) values, wave-uniform
    const double spx = __shfl(px, i, 64), spy = __shfl(py, i, 64), svx = __shfl(vx, i, 64), svy = __shfl(vy, i, 64);
    const double sgx = hum[F_GX * H + i], sgy = hum[F_GY * H + i], srad = hum[F_RAD * H + i], svpref = hum[F_VPREF * H + i];
    const double safety = s.cfg.orca_safety_space;
    // lazily (re)build human i's private simulator: orca.py:83-89
    const size_t ei = (size_t)e * H + i;
    float nd, self_r, self_ms, seen_r;
    const bool rv = s.cfg.robot_visible != 0;
    const int n_agents = n + (rv ? 1 : 0);
    // other humans as seen by i (human FOV = 2*pi: always the true state unless coincident, otherwise the ones inside i's cone; the rest
    // are the dummy (7,7,0,0)); with robot.visible the robot is appended as the last neighbour on lane n (crowd_sim.py:695-699), same
    // visibility rule
    const bool isR = rv && lane == n;
    const double *rob = s.rob + (size_t)e * 8;
    const double qx = isR ? rob[R_PX] : px, qy = isR ? rob[R_PY] : py, qvx = isR ? rob[R_VX] : vx, qvy = isR ? rob[R_VY] : vy;
    const bool coincident = s.cfg.human_fov < 2.0 ? !in_fov(s.cfg, s.cfg.human_fov, spx, spy, svx, svy, 0.0, qx, qy) : (qx == spx) && (qy == spy);
    if (!s.sim_valid[ei] || (s.sim_n && s.sim_n[ei] != n_agents)) {
        nd = (float)s.shared_nd[e];
        self_r = (float)(srad + 0.01 + safety);
        self_ms = (float)svpref;
        // addAgent takes the radius of the state it is handed: a human outside i's field of view right now is the dummy human with the
        // config radius, and keeps that size in this simulator
        seen_r = (float)((coincident ? s.cfg.human_radius : rad) + 0.01 + safety);
        if (s.sim_seen && isH) s.sim_seen[ei * H + lane] = seen_r;
        if (lane == 0) {
            s.sim_nd[ei] = nd; s.sim_self_radius[ei] = self_r; s.sim_self_maxspeed[ei] = self_ms; s.sim_valid[ei] = 1;
            if (s.sim_n) s.sim_n[ei] = (uint8_t)n_agents;
        }
    } else {
        nd = s.sim_nd[ei]; self_r = s.sim_self_radius[ei]; self_ms = s.sim_self_maxspeed[ei];
        seen_r = s.sim_seen ? s.sim_seen[ei * H + lj] : (float)(rad + 0.01 + safety);
    }
    if (isR) seen_r = (float)(s.cfg.robot_radius + 0.01 + safety); // fixed for the whole run
    const bool cand = (isH && lane != i) || isR;
    const float opx = coincident ? 7.0f : (float)qx, opy = coincident ? 7.0f : (float)qy;
    const float ovx = coincident ? 0.0f : (float)qvx, ovy = coincident ? 0.0f : (float)qvy;
    // preferred velocity: orca.py:97-100
    double gvx = sgx - spx, gvy = sgy - spy;
    const double speed = sqrt(gvx * gvx + gvy * gvy);
    if (speed > 1.0) { gvx = gvx / speed; gvy = gvy / speed; }
    float ox, oy;
    orca_wave(lane, n_agents, cand, opx, opy, ovx, ovy, seen_r, (float)spx, (float)spy, (float)svx, (float)svy, self_r, self_ms,
              (float)gvx, (float)gvy, nd, n_agents - 1, (float)s.cfg.orca_time_horizon, (float)s.cfg.time_step, ox, oy);
    if (lane == 0) {
        s.hact[(size_t)e * 2 * H + i] = ox;
        s.hact[(size_t)e * 2 * H + H + i] = oy;
    }
}

// The grid is capped (prefetch_orca): this kernel shares the chip with the policy forward on the caller's stream, and a resident-sized
// grid of wavefronts that walk the agents keeps its share of the issue slots bounded instead of flooding every SIMD.
__global__ __launch_bounds__(256) void orca_kernel(EnvDev s)
{
    const CnStampScope stamp_scope(s.stamp);
    const int lane = threadIdx.x & 63;
    const int total = s.E * s.H;
    for (int agent = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); agent < total; agent += gridDim.x * 4)
        orca_agent(s, agent, lane);
}

// ------------------------------------------------------------------------------------------------------------------
// One LANE per agent (the common case of <= 32 agents in a crowd): the scalar RVO2 algorithm exactly as a CPU would run it,
// 64 agents per wavefront.  The kernel runs BEFORE the policy forward of the same step (prefetch_orca puts it on the caller's
// stream): next to the human-human kernel both slow down several-fold (that kernel saturates the L2 -> CU path this one's
// dependent loads queue behind), alone it takes ~1/10 of the step.
// Everything a lane indexes at run time lives in global memory (the env's agent records, L1-resident); everything it keeps in
// registers is indexed statically: the neighbour keys are ordered by a sorting network, the ORCA lines are built in that order,
// and the linear programs are fully unrolled over (line i, earlier line j).  linearProgram3 (the infeasible case, a few agents
// per thousand) would unroll to O(NB^3) code: those agents are put on a list and redone by the wave-cooperative routine above.
// Same arithmetic, same operation order as orca_wave / the oracle: results are bit-identical.
//
// The launch is a chain of VALU / SALU instructions per wavefront, and a quarter of the SIMDs carry two agent wavefronts (1280 of them on
// 1024 SIMDs at 4096 x 20): what the agent path does not issue comes off the launch twice.  profiles/HISTORY.md section 23 took out of it
// what the result does not need, with every operation that defines the result left where it was:
//   - the staging block converts each record ONCE: (float) px, py, vx, vy as one float4 and the radius (float)(rad + 0.01 + safety); only
//     the positions stay as doubles as well.  Pass 1 and pass 2 read floats (one ds_read per neighbour) instead of converting 5 doubles
//     and adding 2 in every turn;
//   - the exact coincidence test (double positions equal -> the dummy human at (7, 7)) sits behind a float filter, see pass 1;
//   - pass 1 is unrolled (static slot offsets, static key registers), in scheduling groups of four;
//   - the neighbour order compares (key bits, slot) as one 64-bit integer: 6 instructions per compare-exchange, none of them control flow
//     (the short-circuit comparator was 14 with an s_and_saveexec);
//   - 1 / time horizon and 1 / time step are pinned in registers (the select between them was compiled as a select of the doubles, a
//     conversion and a full division per neighbour), the selects of pass 2 are bitwise;
//   - the divisor of the pair walk comes from a lane-computed table, the loop bound from a DPP reduction.
// Measured (4096 x 20, stamped step, two runs): orca_lane 41.1-41.8 -> 35.1-36.6 us; the launch still ends with the row-plan builders.  Resources of <20,32>: 168 VGPRs, no scratch, 61
// spilled scalars (parent 69), 25 408 B static LDS (parent 25 920; six workgroups per CU need <= 27 306).
// ------------------------------------------------------------------------------------------------------------------
#include "orca_sortnet.inc"
#include "row_plan.h"

template <int W> struct LaneVec;
template <> struct LaneVec<8> { typedef float f __attribute__((ext_vector_type(8))); };
template <> struct LaneVec<32> { typedef float f __attribute__((ext_vector_type(32))); };

// NB = slots the sorting network orders (>= candidate neighbours incl. self), VW = width of the register vectors that hold the
// per-lane arrays.  The loops over the sorted neighbours / the lines (pass 2, the linear program) are ROLLED with wave-uniform counters: a
// vector element is then selected by a uniform register index (s_set_gpr_idx), not by 20-32 unrolled copies -- fully unrolled the kernel
// was 85 KB of straight-line code that every wavefront fetched exactly once (instruction-fetch bound, slower than the cooperative kernel).
// Pass 1 (a dozen instructions per slot) is unrolled.
template <int NB, int VW>
__global__ __launch_bounds__(64) void orca_lane_kernel(EnvDev s, const float *plan_det, int32_t *plan, int plan_groups, unsigned long long *plan_stamp)
{
    const CnStampScope stamp_scope((plan && (int)blockIdx.x < plan_groups) ? plan_stamp : s.stamp); // the plan builders' wavefronts have their own slot
    // the first workgroups (one wavefront each, rp_groups(E) of them) build the row plan of the policy's human-human kernel for the observation
    // that was just written (row_plan.h): they only need the detected-human counts, and this kernel is on the step's critical path anyway
    // (a builder's tables and the agents' line table below share one buffer: a workgroup is one or the other)
    constexpr int RAW = (int)sizeof(rowplan::Lds) > NB * 64 * 16 ? (int)sizeof(rowplan::Lds) : NB * 64 * 16;
    __shared__ __attribute__((aligned(16))) char s_raw[RAW];
    // (dispatched first; a builder is the longest chain of the launch, so it also takes the issue priority)
    if (plan && (int)blockIdx.x < plan_groups) {
        __builtin_amdgcn_s_setprio(3);
        rowplan::build((int)blockIdx.x, plan_groups, s.E, s.H, rp_workgroups(s.E, s.H), plan_det, plan, *reinterpret_cast<rowplan::Lds *>(s_raw), nullptr, s.plan_arrive);
        return;
    }
    const int blk = (int)blockIdx.x - (plan ? plan_groups : 0);
    typedef typename LaneVec<VW>::f vec;
    const int agent = blk * 64 + threadIdx.x;
    const int H = s.H;
    const bool live_lane = agent < s.E * H;
    const int e = live_lane ? agent / H : (blk * 64) / H, i = live_lane ? agent - e * H : 0;
    const int n = crowd_size(s, e);
    const bool active = live_lane && i < n; // (inactive lanes run along with nn = 0: the loop counters below must stay wave-uniform)
    const cn_env_config &c = s.cfg;
    // the agent records of the 1 + 63/H (+1) envs this wavefront's lanes belong to, staged once: every later access -- uniform in
    // pass 1, a per-lane gather in pass 2 -- is an LDS read instead of an L2 round trip (the kernel is a chain of dependent loads)
    // (the kernel for NB slots serves crowds of more than NB' agents, NB' the next smaller network: at most 63 / (NB' - 1) + 2 envs per wavefront)
    constexpr int NENV = NB == 8 ? 65 : (NB == 20 ? 10 : 5);
    // Per agent: the position as doubles (the own goal vector and the exact coincidence test need them) and, converted ONCE by the lane that
    // stages the row, what the loops below work on: (float) px, py, vx, vy and the radius as a neighbour's simulator holds it,
    // (float)(rad + 0.01 + safety).  The robots' words likewise.  (Kept as doubles and converted in every turn of pass 1 and pass 2, a
    // neighbour cost 5 ds_read_b64, 5 conversions and two double additions per half-plane.)
    __shared__ double s_px[128], s_py[128], s_rob[NENV][2];
    __shared__ float4 s_f4[128], s_frob[NENV];
    __shared__ float s_fr[128];
    // this lane's own words go out in the same batch as the staging loads, not behind the barrier and behind each other: its goal and
    // preferred speed, and its private simulator -- read whether it is still valid or not (a rebuild below overwrites what was read)
    const double *hum = s.hum + (size_t)e * 8 * H;
    const size_t ei = (size_t)e * H + i;
    const double safety = c.orca_safety_space;
    double sgx, sgy, svpref, shared_nd_in;
    int sim_valid_in, sim_n_in = 0;
    float sim_nd_in, sim_r_in, sim_ms_in;
    {
        const int a0 = blk * 64;
        const int e0 = a0 / H, e1 = (min(a0 + 63, s.E * H - 1)) / H;
        const int nrows = (e1 - e0 + 1) * H; // <= 63 + 2 H <= 127 (H <= 32): two rows per lane at most
        double st[2][5];
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int r = threadIdx.x + 64 * it;
            if (r < nrows) {
                const int ee = e0 + r / H, j = r - (r / H) * H;
                const double *hm = s.hum + (size_t)ee * 8 * H;
                st[it][0] = hm[F_PX * H + j]; st[it][1] = hm[F_PY * H + j]; st[it][2] = hm[F_VX * H + j]; st[it][3] = hm[F_VY * H + j];
                st[it][4] = hm[F_RAD * H + j];
            }
        }
        sgx = hum[F_GX * H + i]; sgy = hum[F_GY * H + i]; svpref = hum[F_VPREF * H + i];
        sim_valid_in = s.sim_valid[ei];
        if (s.sim_n) sim_n_in = s.sim_n[ei];
        sim_nd_in = s.sim_nd[ei]; sim_r_in = s.sim_self_radius[ei]; sim_ms_in = s.sim_self_maxspeed[ei];
        shared_nd_in = s.shared_nd[e];
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int r = threadIdx.x + 64 * it;
            if (r < nrows) {
                s_px[r] = st[it][0]; s_py[r] = st[it][1];
                s_f4[r] = make_float4((float)st[it][0], (float)st[it][1], (float)st[it][2], (float)st[it][3]);
                s_fr[r] = (float)(st[it][4] + 0.01 + safety);
            }
        }
        if (c.robot_visible)
            for (int q = threadIdx.x; q <= e1 - e0; q += 64) {
                const double *rb = s.rob + (size_t)(e0 + q) * 8;
                const double rx0 = rb[R_PX], ry0 = rb[R_PY], rvx0 = rb[R_VX], rvy0 = rb[R_VY];
                s_rob[q][0] = rx0; s_rob[q][1] = ry0;
                s_frob[q] = make_float4((float)rx0, (float)ry0, (float)rvx0, (float)rvy0);
            }
        __syncthreads();
    }
    const int eq = e - (blk * 64) / H, eb = eq * H; // this lane's env inside the staged block
    const double spx = s_px[eb + i], spy = s_py[eb + i];
    const float4 self4 = s_f4[eb + i];
    const bool rv = c.robot_visible != 0;
    const int n_agents = n + (rv ? 1 : 0);
    // lazily (re)build human i's private simulator: orca.py:80-89
    float nd = 0.0f, self_r = 0.0f, self_ms = 0.0f;
    if (active) {
        const bool rebuild = !sim_valid_in || (s.sim_n && sim_n_in != n_agents);
        if (rebuild) {
            nd = (float)shared_nd_in;
            self_r = s_fr[eb + i];
            self_ms = (float)svpref;
            if (s.sim_seen)
                for (int j = 0; j < n; ++j) s.sim_seen[ei * H + j] = s_fr[eb + j];
            s.sim_nd[ei] = nd; s.sim_self_radius[ei] = self_r; s.sim_self_maxspeed[ei] = self_ms; s.sim_valid[ei] = 1;
            if (s.sim_n) s.sim_n[ei] = (uint8_t)n_agents;
        } else {
            nd = sim_nd_in; self_r = sim_r_in; self_ms = sim_ms_in;
        }
    }
    const float fpx = self4.x, fpy = self4.y, fvx = self4.z, fvy = self4.w;
    float4 rob4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (rv) rob4 = s_frob[eq];
    const float rob_r = (float)(c.robot_radius + 0.01 + safety); // fixed for the whole run
    // pass 1: distance keys of the candidates in index order (slot j = agent j; self and empty slots get +inf).  Fully unrolled: slot j of this
    // lane's env sits at a fixed offset from the lane's base, the reads go out together and key[j] is a register of its own.
    // The reference substitutes (7, 7, 0, 0) for a neighbour whose DOUBLE position equals the agent's.  (float) is a function: positions that
    // differ as floats differ as doubles, so the loop compares the staged floats, and only a wavefront in which some candidate's floats are
    // equal to its agent's goes through the exact form (the rolled loop behind it, which reads the doubles) -- almost never.
    vec key, idx; // idx holds the slot numbers' bits
    int nn = 0;
    unsigned coin = 0u; // bit j: slot j is coincident with this agent (the dummy human)
    {
        const float ndSq = nd * nd;
        bool feq = false;
        auto pass1 = [&](auto with_robot) {
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                // (slots j >= n read the rows behind the env's, inside the arrays for every crowd size the kernel serves: not candidates)
                float qx = s_f4[eb + j].x, qy = s_f4[eb + j].y;
                bool cand = active && j < n && j != i;
                if constexpr (decltype(with_robot)::value) {
                    const bool isR = j == n;
                    qx = isR ? rob4.x : qx; qy = isR ? rob4.y : qy;
                    cand = cand || (active && isR);
                }
                feq |= cand & (qx == fpx) & (qy == fpy); // (bitwise: `||` / `&&` became control flow around each compare)
                const float ddx0 = fpx - qx, ddy0 = fpy - qy;
                const float dq = ddx0 * ddx0 + ddy0 * ddy0;
                const bool inrange = cand && dq < ndSq;
                key[j] = inrange ? dq : INFINITY;
                nn += inrange ? 1 : 0;
                // (groups of four: scheduled as one block, the 20-32 candidate masks are all alive at once and spill scalar registers)
                if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        };
        if (rv) pass1(std::true_type{}); else pass1(std::false_type{});
        if (__ballot(feq) != 0ull) {
            nn = 0;
#pragma unroll 1
            for (int j = 0; j < NB; ++j) {
                const bool isR = rv && j == n;
                const bool cand = active && ((j < n && j != i) || isR);
                const int lj = j < n ? j : 0;
                const double qxd = isR ? s_rob[eq][0] : s_px[eb + lj], qyd = isR ? s_rob[eq][1] : s_py[eb + lj];
                const float qx = isR ? rob4.x : s_f4[eb + lj].x, qy = isR ? rob4.y : s_f4[eb + lj].y;
                const bool coincident = (qxd == spx) && (qyd == spy);
                if (cand && coincident) coin |= 1u << j;
                const float opx = coincident ? 7.0f : qx, opy = coincident ? 7.0f : qy;
                const float ddx0 = fpx - opx, ddy0 = fpy - opy;
                const float dq = ddx0 * ddx0 + ddy0 * ddy0;
                const bool inrange = cand && dq < ndSq;
                key[j] = inrange ? dq : INFINITY;
                nn += inrange ? 1 : 0;
            }
        }
    }
    const bool any_coin = __ballot(coin != 0u) != 0ull;
    // ascending (distSq, index): RVO2's insertion order; the +inf slots end up behind the nn real neighbours.  A key is a sum of squares or
    // +inf: not negative, no NaN, so its bit pattern orders like the float, and (key bits, slot) as ONE 64-bit integer orders like the pair:
    // a compare-exchange is one comparison and four selects, without control flow.  Only the slots are used below.
    {
        unsigned long long kv[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) kv[j] = ((unsigned long long)__float_as_uint(key[j]) << 32) | (unsigned)j;
#define ORCA_CE(a, b)                                                  \
    {                                                                  \
        const unsigned long long ka0 = kv[a], kb0 = kv[b];             \
        const bool sw = kb0 < ka0;                                     \
        kv[a] = sw ? kb0 : ka0; kv[b] = sw ? ka0 : kb0;                \
    }
        if constexpr (NB == 8) { ORCA_SORTNET_8(ORCA_CE) }
        else if constexpr (NB == 20) { ORCA_SORTNET_20(ORCA_CE) }
        else { static_assert(NB == 32, "sorting networks exist for 8, 20 and 32 slots"); ORCA_SORTNET_32(ORCA_CE) }
#undef ORCA_CE
#pragma unroll
        for (int j = 0; j < NB; ++j) idx[j] = __uint_as_float(held((unsigned)kv[j])); // (pinned: or pass 2 indexes kv[] itself, in scratch)
    }
    const int nmax = rowplan::wave_max(nn); // wave-uniform loop bound (a DPP reduction: six ds_bpermute round trips as shuffles)
    // pass 2: the ORCA half-plane of the k-th nearest neighbour (Agent::computeNewVelocity), kept in LDS as s_line[k][lane]: the
    // linear program below reads lines of OTHER lanes' agents at per-lane line numbers, which registers cannot do.
    // The three cases of RVO2 (cut-off circle, legs, collision) go through ONE sqrtf and ONE division whose operands are selected per
    // case -- the same operations on the same operands as the branchy form (no contraction in this file), so the same bits, but no
    // divergence: with 64 agents in a wavefront every branch was taken by somebody.
    // (1 / time horizon and 1 / time step are pinned: left to the compiler, `collide ? invDT : invTH` became a select of the two DOUBLES, a
    // conversion and a third full division in every turn)
    const float invTH = held(1.0f / (float)c.orca_time_horizon), invDT = held(1.0f / (float)c.time_step);
    float4 *const s_line = reinterpret_cast<float4 *>(s_raw);
    const int tid = threadIdx.x;
#pragma unroll 1
    for (int k = 0; k < nmax; ++k) {
        float o_px = 0.0f, o_py = 0.0f, o_dx = 1.0f, o_dy = 0.0f;
        const int j = (int)__float_as_uint(idx[k]);
        if (k < nn) {
            const bool isR = j == n; // only reachable when rv
            const int lj = isR ? 0 : j;
            float4 q = s_f4[eb + lj];
            float orad;
            if (s.sim_seen) orad = s.sim_seen[ei * H + lj];
            else orad = held(s_fr[eb + lj]); // (pinned: or the two become one flat load through a selected pointer)
            if (rv) { q.x = isR ? rob4.x : q.x; q.y = isR ? rob4.y : q.y; q.z = isR ? rob4.z : q.z; q.w = isR ? rob4.w : q.w; orad = isR ? rob_r : orad; }
            if (any_coin) { // (wave-uniform)
                const bool coincident = (coin >> j) & 1u;
                q.x = coincident ? 7.0f : q.x; q.y = coincident ? 7.0f : q.y; q.z = coincident ? 0.0f : q.z; q.w = coincident ? 0.0f : q.w;
            }
            const float opx = q.x, opy = q.y, ovx = q.z, ovy = q.w;
            const float rpx = opx - fpx, rpy = opy - fpy;   // relativePosition
            const float rvx = fvx - ovx, rvy = fvy - ovy;   // relativeVelocity
            const float distSq = rpx * rpx + rpy * rpy;
            const float cr = self_r + orad;
            const float crSq = cr * cr;
            const bool collide = !(distSq > crSq);
            const float invT = collide ? invDT : invTH;
            const float wx = rvx - invT * rpx, wy = rvy - invT * rpy;
            const float wLenSq = wx * wx + wy * wy;
            const float dot1 = wx * rpx + wy * rpy;
            const bool circle = collide | ((dot1 < 0.0f) & (dot1 * dot1 > crSq * wLenSq));  // project on the cut-off circle (bitwise: no control flow)
            const float sq = sqrtf(circle ? wLenSq : distSq - crSq);                        // wLen, or the leg length
            const float inv = 1.0f / (circle ? sq : distSq);                                // 1 / wLen, or 1 / distSq
            // cut-off circle (time horizon, or the time step on collision)
            const float uwx = wx * inv, uwy = wy * inv;
            const float sc = cr * invT - sq;
            // legs
            const bool left = rpx * wy - rpy * wx > 0.0f;
            const float lxl = (rpx * sq - rpy * cr) * inv, lxr = -((rpx * sq + rpy * cr) * inv); // (both sides computed, then selected)
            const float lyl = (rpx * cr + rpy * sq) * inv, lyr = -((-rpx * cr + rpy * sq) * inv);
            const float lgx = left ? lxl : lxr, lgy = left ? lyl : lyr;
            const float dot2 = rvx * lgx + rvy * lgy;
            const float ldx = circle ? uwy : lgx, ldy = circle ? -uwx : lgy;
            const float ux = circle ? sc * uwx : dot2 * lgx - rvx, uy = circle ? sc * uwy : dot2 * lgy - rvy;
            o_px = fvx + 0.5f * ux; o_py = fvy + 0.5f * uy; o_dx = ldx; o_dy = ldy;
        }
        s_line[k * 64 + tid] = make_float4(o_px, o_py, o_dx, o_dy);
    }
    // preferred velocity: orca.py:97-100
    double gvx = sgx - spx, gvy = sgy - spy;
    const double speed = sqrt(gvx * gvx + gvy * gvy);
    if (speed > 1.0) { gvx = gvx / speed; gvy = gvy / speed; }
    const float optx = (float)gvx, opty = (float)gvy, radius = self_ms;
    // linearProgram2 (optimise the preferred velocity, directionOpt = false)
    float rx, ry;
    if (optx * optx + opty * opty > radius * radius) {
        const float inv = 1.0f / sqrtf(optx * optx + opty * opty);
        rx = radius * (optx * inv); ry = radius * (opty * inv);
    } else {
        rx = optx; ry = opty;
    }
    // linearProgram1 of a violated line li cuts it against every earlier line lj < li of the same agent.  An agent violates ~1.2 of
    // its lines, but some agent of the 64 violates almost every line: a loop over lj run by the whole wavefront did 80 iterations per
    // wavefront for a handful of agents each time.  Instead the (violating agent, earlier line) pairs of a line are dealt to the 64
    // lanes, and the bounds of an agent are combined in LDS with integer min / max on order-preserving keys (min and max do not
    // depend on the order of their operands: the same tLeft / tRight as the sequential loop).
    // (their four 256-byte tables sit in row NB - 1 of the line table: an agent has at most NB - 1 neighbours.  The static LDS of a workgroup
    // stays below 1/6 of the CU's: five per CU would leave the 1281st workgroup of a 4096 x 20 batch waiting for a whole generation)
    unsigned *const s_tl = reinterpret_cast<unsigned *>(s_line + (NB - 1) * 64), *const s_tr = s_tl + 64;
    int *const s_pf = reinterpret_cast<int *>(s_tr + 64), *const s_vl = s_pf + 64;
    auto okey = [](float f) { const unsigned u = __float_as_uint(f); return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u); };
    auto okey_inv = [](unsigned o) { return __uint_as_float(o ^ ((o >> 31) ? 0x80000000u : 0xffffffffu)); };
    bool failed = false;
    int line_fail = 0;
    // lane l: ceil(2^20 / l), the multiplier that divides a pair number by l; a violated line li < 32 fetches lane li's (the division by
    // the wave-uniform li, done in the loop, was 25 dependent instructions per violated line)
    const unsigned inv20_of_lane = ((1u << 20) + (unsigned)max(tid, 1) - 1u) / (unsigned)max(tid, 1);
#pragma unroll 1
    for (int li = 0; li < nmax; ++li) {
        const float4 Li = s_line[li * 64 + tid];
        const float ipx = Li.x, ipy = Li.y, idx_ = Li.z, idy = Li.w;
        const bool viol = li < nn && !failed && idx_ * (ipy - ry) - idy * (ipx - rx) > 0.0f;
        const unsigned long long vm = __ballot(viol);
        if (vm == 0ull) continue; // wave-uniform: nobody has to re-optimise on this line
        // linearProgram1 on line li against the disc ...
        const float dotProduct = ipx * idx_ + ipy * idy;
        const float discriminant = dotProduct * dotProduct + radius * radius - (ipx * ipx + ipy * ipy);
        bool ok = !(discriminant < 0.0f);
        const float sq = sqrtf(discriminant);
        float tLeft = -dotProduct - sq, tRight = -dotProduct + sq;
        bool pfail = false;
        // ... and against the earlier lines
        const int npairs = __popcll(vm) * li;
        if (npairs > 0) {
            if (viol) {
                const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(vm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)vm, 0u));
                s_vl[rank] = tid; s_tl[tid] = okey(tLeft); s_tr[tid] = okey(tRight); s_pf[tid] = 0;
            }
            __syncthreads(); // (one wavefront: orders the LDS traffic, costs a waitcnt)
            const unsigned inv20 = (unsigned)__builtin_amdgcn_readlane((int)inv20_of_lane, li); // p / li = p * inv20 >> 20 for p (li - 1) < 2^20
#pragma unroll 1
            for (int p0 = 0; p0 < npairs; p0 += 64) {
                const int p = p0 + tid;
                const bool on = p < npairs;
                const int r = on ? (int)(((unsigned)p * inv20) >> 20) : 0;
                const int lj = on ? p - r * li : 0;
                const int a = s_vl[r];
                const float4 A = s_line[li * 64 + a], B = s_line[lj * 64 + a];
                const float denominator = A.z * B.w - A.w * B.z;
                const float numerator = B.z * (A.y - B.y) - B.w * (A.x - B.x);
                const bool parallel = fabsf(denominator) <= RVO_EPS;
                const float t = numerator / denominator;
                if (on) {
                    if (parallel) { if (numerator < 0.0f) s_pf[a] = 1; }
                    else if (denominator >= 0.0f) atomicMin(&s_tr[a], okey(t));
                    else atomicMax(&s_tl[a], okey(t));
                }
            }
            __syncthreads();
            if (viol) { tLeft = okey_inv(s_tl[tid]); tRight = okey_inv(s_tr[tid]); pfail = s_pf[tid] != 0; }
            __syncthreads(); // the slots are rewritten by the next violated line
        }
        // (sequential RVO2 fails at the first prefix that crosses; the bounds are monotone, so this is the same decision)
        ok = ok && !pfail && !(tLeft > tRight);
        if (viol) {
            if (ok) {
                const float tt = idx_ * (optx - ipx) + idy * (opty - ipy);
                const float t_opt = tt < tLeft ? tLeft : (tt > tRight ? tRight : tt);
                rx = ipx + t_opt * idx_;
                ry = ipy + t_opt * idy;
            } else {
                failed = true; // linearProgram3 needed
                line_fail = li;
            }
        }
    }
    // infeasible program: hand the lines and the state linearProgram2 stopped in to the wave-cooperative linearProgram3
    int slot = -1;
    if (active && failed) {
        slot = atomicAdd(s.lp3_cnt, 1);
        Lp3Hdr hd;
        hd.agent = agent; hd.nn = nn; hd.line_fail = line_fail; hd.rx = rx; hd.ry = ry; hd.radius = radius;
        s.lp3_hdr[slot] = hd;
    } else if (active) {
        s.hact[(size_t)e * 2 * H + i] = rx;
        s.hact[(size_t)e * 2 * H + H + i] = ry;
    }
    if (__ballot(slot >= 0) != 0ull) {
#pragma unroll 1
        for (int k = 0; k < nmax; ++k) {
            const float4 ln = s_line[k * 64 + tid];
            if (slot >= 0 && k < nn) s.lp3_lines[(size_t)slot * 32 + k] = ln;
        }
    }
}

// calc_human_future_traj(method='truth') (crowd_sim_var_num.py:152-206), one roll per launch: every human acts with its own
// ORCA policy (act_joint_state -> ORCA.predict on its private simulator: frozen radii / neighbour distance) on the states
// predicted by roll k-1 and is stepped by one_step_lookahead (agent.py:185-192).  The other humans' states are passed as
// they are (no FOV / dummy substitution here).  Roll k needs all of roll k-1 of the same env -> one launch per roll.
__global__ __launch_bounds__(256) void orca_truth_kernel(EnvDev s, int k)
{
    const int lane = threadIdx.x & 63;
    const int agent = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (agent >= s.E * s.H) return;
    const int H = s.H;
    const int e = agent / H, i = agent - e * H;
    const int n = crowd_size(s, e);
    if (i >= n) return;
    const double *hum = s.hum + (size_t)e * 8 * H;
    double *trk = s.tr + ((size_t)e * (s.R + 1) + k) * 4 * H;
    const double *src = k == 1 ? hum : trk - 4 * H; // F_PX..F_VY are fields 0..3: the live state has the same [4][H] layout
    const bool isH = lane < n;
    const int lj = isH ? lane : 0;
    const double px = src[0 * H + lj], py = src[1 * H + lj], vx = src[2 * H + lj], vy = src[3 * H + lj];
    const double rad = hum[F_RAD * H + lj];
    const double spx = __shfl(px, i, 64), spy = __shfl(py, i, 64), svx = __shfl(vx, i, 64), svy = __shfl(vy, i, 64);
    const double sgx = hum[F_GX * H + i], sgy = hum[F_GY * H + i];
    const size_t ei = (size_t)e * H + i;
    float nd, self_r, self_ms, seen_r;
    if (!s.sim_valid[ei] || (s.sim_n && s.sim_n[ei] != n)) {
        // predict_method 'truth' as the observation predictor: the roll-out of a freshly reset env runs before any ORCA step, and
        // act_joint_state builds the private simulator exactly like ORCA.predict would (orca.py:83-89)
        const double safety = s.cfg.orca_safety_space;
        nd = (float)s.shared_nd[e];
        self_r = (float)(hum[F_RAD * H + i] + 0.01 + safety);
        self_ms = (float)hum[F_VPREF * H + i];
        seen_r = (float)(rad + 0.01 + safety);
        if (s.sim_seen && isH) s.sim_seen[ei * H + lane] = seen_r;
        if (lane == 0) {
            s.sim_nd[ei] = nd; s.sim_self_radius[ei] = self_r; s.sim_self_maxspeed[ei] = self_ms; s.sim_valid[ei] = 1;
            if (s.sim_n) s.sim_n[ei] = (uint8_t)n;
        }
    } else {
        nd = s.sim_nd[ei]; self_r = s.sim_self_radius[ei]; self_ms = s.sim_self_maxspeed[ei];
        seen_r = s.sim_seen ? s.sim_seen[ei * H + lj] : (float)(rad + 0.01 + s.cfg.orca_safety_space);
    }
    const bool cand = isH && lane != i;
    double gvx = sgx - spx, gvy = sgy - spy;
    const double speed = sqrt(gvx * gvx + gvy * gvy);
    if (speed > 1.0) { gvx = gvx / speed; gvy = gvy / speed; }
    float ox, oy;
    orca_wave(lane, n, cand, (float)px, (float)py, (float)vx, (float)vy, seen_r, (float)spx, (float)spy, (float)svx, (float)svy, self_r, self_ms,
              (float)gvx, (float)gvy, nd, n - 1, (float)s.cfg.orca_time_horizon, (float)s.cfg.time_step, ox, oy);
    if (lane == 0) {
        trk[0 * H + i] = spx + (double)ox * s.cfg.time_step;
        trk[1 * H + i] = spy + (double)oy * s.cfg.time_step;
        trk[2 * H + i] = (double)ox;
        trk[3 * H + i] = (double)oy;
    }
}

// The same roll-outs for humans.policy = 'social_force': act_joint_state -> SOCIAL_FORCE.predict (social_force.py:11-52) on the rolled
// states, the others being the H - 1 fellow humans with their true radii (no dummy substitution, no robot: crowd_sim_var_num.py:183-190).
// No solver and no private simulator: one wavefront per env (lane i = human i) walks all P rolls in one launch, the rolled states
// travel between the lanes by shuffles.  float64, same operation order as the step's own social-force block (env_step_kernel).
__global__ __launch_bounds__(64) void sf_truth_kernel(EnvDev s)
{
    const int e = blockIdx.x, lane = threadIdx.x;
    const int H = s.H, n = crowd_size(s, e);
    const cn_env_config &c = s.cfg;
    const double *hum = s.hum + (size_t)e * 8 * H;
    const bool isH = lane < n;
    const int lj = isH ? lane : 0;
    double px = hum[F_PX * H + lj], py = hum[F_PY * H + lj], vx = hum[F_VX * H + lj], vy = hum[F_VY * H + lj];
    const double rad = hum[F_RAD * H + lj], gx = hum[F_GX * H + lj], gy = hum[F_GY * H + lj], vpref = hum[F_VPREF * H + lj];
    for (int k = 1; k <= s.R; ++k) {
        const double dxg = gx - px, dyg = gy - py;
        const double dist_to_goal = sqrt(dxg * dxg + dyg * dyg);
        const double desired_vx = (dxg / dist_to_goal) * vpref, desired_vy = (dyg / dist_to_goal) * vpref;
        const double curr_dvx = c.sf_KI * (desired_vx - vx), curr_dvy = c.sf_KI * (desired_vy - vy);
        double ivx = 0.0, ivy = 0.0;
        for (int j = 0; j < n; ++j) {
            const double ox = __shfl(px, j, 64), oy = __shfl(py, j, 64), orad = __shfl(rad, j, 64);
            const double dx = px - ox, dy = py - oy;
            const double d = sqrt(dx * dx + dy * dy);
            const double f = c.sf_A * det_exp((rad + orad - d) / c.sf_B);
            if (j != lane) { ivx += f * (dx / d); ivy += f * (dy / d); }
        }
        const double nvx = vx + (curr_dvx + ivx) * c.time_step, nvy = vy + (curr_dvy + ivy) * c.time_step;
        const double act_norm = sqrt(nvx * nvx + nvy * nvy);
        double ax = nvx, ay = nvy;
        if (act_norm > vpref) { ax = nvx / act_norm * vpref; ay = nvy / act_norm * vpref; }
        // one_step_lookahead, agent.py:185-192 (every lane has read the old states: the shuffles above precede these writes)
        px = px + ax * c.time_step; py = py + ay * c.time_step; vx = ax; vy = ay;
        if (isH) {
            double *trk = s.tr + ((size_t)e * (s.R + 1) + k) * 4 * H;
            trk[0 * H + lane] = px; trk[1 * H + lane] = py; trk[2 * H + lane] = vx; trk[3 * H + lane] = vy;
        }
    }
}

// stand-alone batched solve (cn_orca_solve)
__global__ __launch_bounds__(256) void orca_solve_kernel(int B, int n_other, const float *self, const float *others, float nd,
                                                         int max_nb, float th, float dt, float *out)
{
    const int lane = threadIdx.x & 63;
    const int b = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (b >= B) return;
    const float *sp = self + (size_t)b * 8;
    const bool cand = lane < n_other;
    const float *o = others + ((size_t)b * n_other + (cand ? lane : 0)) * 5;
    float ox, oy;
    orca_wave(lane, n_other, cand, o[0], o[1], o[2], o[3], o[4], sp[0], sp[1], sp[2], sp[3], sp[4], sp[5], sp[6], sp[7], nd,
              max_nb, th, dt, ox, oy);
    if (lane == 0) { out[2 * b] = ox; out[2 * b + 1] = oy; }
}

} // namespace
