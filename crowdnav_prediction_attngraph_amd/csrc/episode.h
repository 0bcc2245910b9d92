// episode.h -- scenario generation on one env's wavefront (lane j = human j): placement by rejection (one wavefront, or all the
// wavefronts of a workgroup), episode generation, reset, observation writing, staging of the next episode and the post-observation
// goal changes / respawns.  The kernels that run them are in env_sim.hip, whose translation unit this is part of.
#pragma once
#include "env_dev.h"
#include "env_profile.h"
#include "det_math.h"
#include "mt19937.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// Per-env wavefront state: lane j owns human j.
// ------------------------------------------------------------------------------------------------------------------
struct Lane {
    double px, py, vx, vy, gx, gy, rad, vpref; // human j
    double l0, l1, l2, l3, l4;                  // last_human_states[j]
    uint8_t simv;
};
struct Robot { double px, py, vx, vy, gx, gy, theta, pot; };

__device__ __forceinline__ double norm2(double x, double y) { return sqrt(x * x + y * y); }
// norm2(x, y) < d, decided without the square root whenever the squared distance is not within a few ulps of d * d: sqrt is correctly
// rounded and monotone, so outside that band the comparison of the squares gives the same answer; inside it (practically never) the
// reference expression itself is evaluated.  d >= 0.
__device__ __forceinline__ bool closer_than(double x, double y, double d)
{
    const double q = x * x + y * y, dd = d * d;
    if (q < dd * (1.0 - 0x1p-48)) return true;
    if (q > dd * (1.0 + 0x1p-48)) return false;
    return sqrt(q) < d;
}

// ---- a long rejection loop over the W wavefronts of a workgroup (dense crowds, BASELINE configs[4]) ----
// In a crowd of ~50 randomised humans a placement takes 4 candidates in the median, one in 40 more than 64, and one in 10^4 runs to the bound
// of 65 536: ~1000 passes of one wavefront, 3 ms, while the other 8191 envs of the step are long done -- and with ~400 envs of a batch changing
// 25 goals each in a step, nearly every step has one.  The candidates are a pure function of the MT19937 stream (candidate j of a loop that
// starts at stream word g reads the words g + 6 j .. g + 6 j + 5, whatever its fate), and the stream is a recurrence with a lag of 227 words:
//     s[m] = s[m - 227] ^ f(s[m - 624], s[m - 623]),
// so one wavefront can run it 192 words at a time without ever waiting for anybody else.  Once a loop has run COOP_AFTER candidates on its
// own, the workgroup's other wavefronts (parked at a barrier until then) join in, in rounds of 64 (W - 1) candidates: the last wavefront is
// the PRODUCER -- while the others evaluate round r it extends the stream, in a ring of LDS blocks, as far as round r + 1 reads -- the master
// and the W - 2 helpers put 64 candidates each through a COARSE fp32 screen (coop_screen_pass: "collides for certain", with 1e-3 of slack on
// the squared thresholds; a bound-hitting loop is 65 537 candidates x ~100 points, and one CU evaluates ~400 candidates per microsecond this
// way whatever W is), and the master re-evaluates with the exact walk, in stream order, the passes that reported a candidate the screen
// could not reject: the first accepted candidate IN STREAM ORDER wins (or the first one past the bound) -- the same candidate, and the
// same staged block and position afterwards, as the serial loop, whose own cutting of the stream into passes has no influence on either.
// One workgroup barrier per round; every thread tracks the round's stream position itself, and the master only speaks up (a second
// barrier) in rounds where some wavefront reported something.
// groups of 64 candidates one evaluating wavefront screens per round, C per lane: a pair of points is read from LDS once (a broadcast read of
// 24 bytes per lane: 12 clocks of the CU's LDS pipe) and tested against C candidates (6 C packed instructions), so with C = 1 four busy SIMDs
// ask for twice what the LDS delivers
constexpr int coop_c(int W) { return W <= 4 ? 4 : (W <= 8 ? 2 : 1); }
template <int W>
struct CoopLds {
    static constexpr int NE = W - 1;                          // evaluating wavefronts (master + helpers)
    static constexpr int C = coop_c(W);
    static constexpr int NG = NE * C;                         // groups of 64 candidates per round
    static constexpr int NB1 = (384 * NG + 623) / MT_N;       // new blocks a round can need
    static constexpr int BW = MT_N * (NB1 + 1) + 227;         // one buffer: the last block of the round before, the new ones, the producer's overshoot
    int cmd;                        // 1 = a placement is published, 2 = the kernel is over
    int verdict;                    // the master's answer in a round with reports: 1 = the placement is over, 0 = next round
    int kind, n_pairs, max_att;
    int pos0, attempt0;             // position in the staged block / candidate number of the first cooperative candidate
    float circle_radius, vp;
    // the blocking points two by two, as the coarse screen reads them (one broadcast read per pair): {x0, x1, y0, y1} and the squared
    // thresholds minus the slack; pair 0 = the robot's goal and position, then the master's packed lists (goals, positions), the last
    // point twice when the count is odd
    float4 pxy[66];
    float2 plo[66];
    // round r reads buf[r & 1]: the stream LINEARLY from block b1(r - 1) (the last block round r - 1 touched; block 0 = the staged one, for
    // round 0) to block b1(r), whole blocks; the producer fills buf[(r + 1) & 1] meanwhile
    uint32_t buf[2][BW];
    unsigned long long take[2][NG]; // by round parity, per group
};
#ifdef CN_POST_DEBUG
__device__ long long g_post_dbg[8192 * 8]; // per block: ticks total, ticks in coop, coop placements, coop rounds, placements, serial passes, start tick, -
__shared__ long long g_dbg_blk[8];
#define DBG_ADD(i, v) do { if (lane == 0) g_dbg_blk[i] += (v); } while (0)
#else
#define DBG_ADD(i, v) do { } while (0)
#endif
constexpr int COOP_AFTER = 128;     // candidates a loop evaluates alone before the helpers join (98.5 % of the loops end earlier)
template <int W>
__device__ __forceinline__ CoopLds<W> &coop_lds()
{
    __shared__ CoopLds<W> q; // (only kernels instantiated with W > 1 reference it)
    return q;
}
// ONE wavefront: dst[0 .. 623] = hist[0 .. 623] (a complete block), then n_new more words of the stream behind it, 227 per iteration with a
// fixed word -> (step, lane) mapping: the lag-227 operand of a word is then the word the same lane made in the same step of the iteration
// before -- it never leaves its register -- and the other two operands (624 and 623 words back) were written at least one whole iteration
// earlier by this same wavefront (the LDS executes a wavefront's accesses in order), so they are loaded one iteration ahead and nothing in
// the loop waits for a store.  May overshoot n_new by up to 226 words (correct stream words; the buffer has the room).
__device__ __forceinline__ void coop_produce(uint32_t *dst, const uint32_t *hist, int lane, int n_new)
{
    if (hist) {
        uint32_t t[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) t[k] = hist[64 * k + (k < 9 || lane < MT_N - 576 ? lane : 0)];
#pragma unroll
        for (int k = 0; k < 9; ++k) dst[64 * k + lane] = t[k];
        if (lane < MT_N - 576) dst[576 + lane] = t[9];
        rng_sync();
    }
    // word m (relative to dst + 624) of an iteration that starts at m0: step u, lane l <-> m = m0 + 64 u + l, 64 u + l < 227
    const bool last = lane < 227 - 192;
    uint32_t *p = dst + lane; // &dst[m0 + lane], m0 = 0: operands at p[64 u], p[64 u + 1]; lag-227 operand at p[64 u + 397]; result to p[64 u + 624]
    uint32_t far[4], a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { far[u] = p[64 * u + 397]; a[u] = p[64 * u]; b[u] = p[64 * u + 1]; } // (u = 3, lanes >= 35: read but never used)
    for (int m = 0; m < n_new; m += 227, p += 227) {
        uint32_t na[4], nb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { na[u] = p[227 + 64 * u]; nb[u] = p[227 + 64 * u + 1]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t y = (a[u] & 0x80000000u) | (b[u] & 0x7fffffffu);
            far[u] = far[u] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            if (u < 3 || last) p[64 * u + MT_N] = far[u];
            a[u] = na[u]; b[u] = nb[u];
        }
        __builtin_amdgcn_wave_barrier();
    }
    rng_sync();
}

// groups p C .. p C + C - 1 (64 candidates each, C per lane) of the round whose first candidate starts at word `off` of `rb`: which candidates can
// the coarse screen NOT reject (or lie past the bound)?  -> Q.take[round & 1][group]  Candidate and squares in fp32 from the 27 high bits of each double's first word (the angle's sine and cosine from
// V_SIN_F32 / V_COS_F32, whose argument is in revolutions): the candidate is within ~1e-5 of the fp64 one, a square near md^2 ~ 1 within 3e-5
// of the true one, and "square < md^2 (1 - 1e-3)" therefore means closer than md for certain.  The other direction is not needed: whatever
// is not rejected here is evaluated by the master, exactly.
template <int W>
__device__ __forceinline__ void coop_screen_pass(CoopLds<W> &Q, const uint32_t *rb, int off, int att0, int p, int lane, int round,
                                                 int kind, int n_pairs, int max_att, float radius, float vp)
{
    typedef float f2 __attribute__((ext_vector_type(2)));
    constexpr int C = CoopLds<W>::C;
    f2 xx[C], yy[C];
    float m[C]; // min over the points of (square - lowered threshold)
#pragma unroll
    for (int cc = 0; cc < C; ++cc) {
        const uint32_t *w = rb + off + 6 * (64 * (p * C + cc) + lane);
        const float u0 = (float)(mt_temper(w[0]) >> 5) * 0x1p-27f, u1 = (float)(mt_temper(w[2]) >> 5) * 0x1p-27f, u2 = (float)(mt_temper(w[4]) >> 5) * 0x1p-27f;
        const float cs = __builtin_amdgcn_cosf(u0), sn = __builtin_amdgcn_sinf(u0);
        const float nx = kind == 0 ? u1 * 2.0f : (u1 - 0.5f) * vp, ny = kind == 0 ? u2 * 2.0f : (u2 - 0.5f) * vp;
        const float xf = radius * cs + nx, yf = radius * sn + ny;
        xx[cc] = f2{xf, xf}; yy[cc] = f2{yf, yf};
        m[cc] = 1.0f;
    }
    for (int k = 0; k < n_pairs; ++k) {
        const float4 pq = Q.pxy[k];
        const float2 lo = Q.plo[k];
#pragma unroll
        for (int cc = 0; cc < C; ++cc) {
            const f2 ax = xx[cc] - f2{pq.x, pq.y}, ay = yy[cc] - f2{pq.z, pq.w};
            const f2 d = (ax * ax + ay * ay) - f2{lo.x, lo.y};
            m[cc] = fminf(m[cc], fminf(d.x, d.y));
        }
    }
#pragma unroll
    for (int cc = 0; cc < C; ++cc) {
        const uint64_t take = __ballot(!(m[cc] < 0.0f) || att0 + 64 * (p * C + cc) + lane >= max_att);
        if (lane == 0) Q.take[round & 1][p * C + cc] = take;
    }
}

// The reference's placement loops (crowd_sim_var_num.py:116-146 positions, crowd_sim.py:415-485 goals) are rejection sampling: candidate k
// is made of the stream's next three doubles (angle, x noise, y noise), and the first candidate that keeps its distance from the robot
// and from every human of the list is taken.  One candidate costs six words of the MT19937 stream whatever its fate, so candidate k of a
// loop that starts at stream position p reads the words p + 6 k .. p + 6 k + 5: the candidates inside the current 624-word block are
// evaluated 64 AT A TIME, one per lane (each lane walks the human list itself: human j's state comes out of lane j by v_readlane), and
// the first accepted one in stream order wins -- the same candidate, the same stream position afterwards, as the one-at-a-time loop.
// A candidate whose six words straddle the end of the block rides as lane 0 of the first pass over the regenerated block.  In crowds of ~50 randomised humans these loops run for 10^2 .. 10^5 candidates (BASELINE configs[4]).
//   kind 0: position of a new human (noise = u * 2),  kind 1: new goal (noise = (u - 0.5) * vp)
//   humans 0 .. n_list - 1 except `skip` are tested with md = radius + rad_j + discomfort_dist against their position and their goal
template <int W = 1, class S>
__device__ __forceinline__ void place_by_rejection(const S &s, Rng &R, int lane, int kind, double radius, double vp, double md_r, int n_list, int skip,
                                                   const Robot &rb, const Lane &h, double &out_x, double &out_y)
{
    const auto &c = s.cfg;
    const int max_att = c.max_placement_attempts > 0 ? c.max_placement_attempts : CN_MAX_PLACEMENT_ATTEMPTS;
    auto make = [&](double u0, double u1, double u2, double &x, double &y) {
        const double angle = u0 * M_PI * 2.0;
        const double nx = kind == 0 ? (0.0 + (1.0 - 0.0) * u1) * 2.0 : (u1 - 0.5) * vp;
        const double ny = kind == 0 ? (0.0 + (1.0 - 0.0) * u2) * 2.0 : (u2 - 0.5) * vp;
        double sn, cs;
        det_sincos(angle, sn, cs);
        x = c.circle_radius * cs + nx;
        y = c.circle_radius * sn + ny;
    };
    // does candidate (x, y) of this lane collide?  `live`: lanes whose answer matters (the walk ends once all of them have collided).
    // The walk decides `norm2(d) < md` on the SQUARES: q < md^2 (1 - 2^-48) means closer, q > md^2 (1 + 2^-48) means not (closer_than's
    // argument); a square inside that band (practically never) only marks the lane, and marked lanes that found no collision are walked
    // again with the reference expression itself.  (With the square root inside the walk -- the compiler evaluates it for every lane that
    // is not clearly closer, i.e. nearly always -- a (candidate, human) pair cost ~90 fp64 instructions instead of ~20.)
    // lane j keeps human j's thresholds: md_j = radius + rad_j + discomfort_dist
    const double md_l = radius + h.rad + c.discomfort_dist, dd_l = md_l * md_l;
    const double lo_l = dd_l * (1.0 - 0x1p-48), hi_l = dd_l * (1.0 + 0x1p-48);
    const double ddr = md_r * md_r, lo_r = ddr * (1.0 - 0x1p-48), hi_r = ddr * (1.0 + 0x1p-48);
    auto collides_exact = [&](double x, double y) {
        bool coll = norm2(x - rb.px, y - rb.py) < md_r || norm2(x - rb.gx, y - rb.gy) < md_r;
        for (int j = 0; j < n_list; ++j) {
            if (j == skip) continue;
            const double jx = wv_readlane_d(h.px, j), jy = wv_readlane_d(h.py, j), jgx = wv_readlane_d(h.gx, j), jgy = wv_readlane_d(h.gy, j);
            const double md = radius + wv_readlane_d(h.rad, j) + c.discomfort_dist;
            coll = coll || norm2(x - jx, y - jy) < md || norm2(x - jgx, y - jgy) < md;
        }
        return coll;
    };
    // Which (human, point) pairs can block a candidate at all?  Every candidate lies within n_max of the circle of radius R (its noise), so a
    // point whose distance from the origin is not inside (R - n_max - md, R + n_max + md) cannot come closer than md to any of them: mid-episode
    // most humans' POSITIONS are far inside the circle and drop out; the goals sit on it.  (1e-3 of slack for the rounding of cos / sin.)
    const double n_max = kind == 0 ? 2.0 * 1.4142135623730951 : 0.70710678118654757 * vp;
    const double w_l = n_max + md_l + 1e-3, r_in = c.circle_radius - w_l, r_out = c.circle_radius + w_l;
    const double in2 = r_in > 0.0 ? r_in * r_in : -1.0, out2 = r_out * r_out;
    const bool listed = lane < n_list && lane != skip;
    const double hp2 = h.px * h.px + h.py * h.py, hg2 = h.gx * h.gx + h.gy * h.gy;
    const uint64_t pos_mask = __ballot(listed && hp2 > in2 && hp2 < out2), goal_mask = __ballot(listed && hg2 > in2 && hg2 < out2);
    // The verdicts are kept as two running minima instead of lane masks (a mask update per test is a dozen scalar instructions; a
    // v_min_f64 is one): with d = q - lo,  closer  <=>  d < 0  (an IEEE difference has the sign of the comparison), and
    // inside the band  <=>  lo <= q <= hi  <=>  max(-d, q - hi) <= 0.
    auto collides64 = [&](double x, double y, bool live) {
        double ax = x - rb.px, ay = y - rb.py, bx = x - rb.gx, by = y - rb.gy;
        double q1 = ax * ax + ay * ay, q2 = bx * bx + by * by;
        double d1 = q1 - lo_r, d2 = q2 - lo_r;
        double cmin = fmin(d1, d2);
        double bmin = fmin(fmax(-d1, q1 - hi_r), fmax(-d2, q2 - hi_r));
        for (uint64_t m = goal_mask; m; m &= m - 1) {
            const int j = __ffsll((unsigned long long)m) - 1;
            const double jx = wv_readlane_d(h.gx, j), jy = wv_readlane_d(h.gy, j), lo = wv_readlane_d(lo_l, j), hi = wv_readlane_d(hi_l, j);
            ax = x - jx; ay = y - jy;
            q1 = ax * ax + ay * ay;
            d1 = q1 - lo;
            cmin = fmin(cmin, d1);
            bmin = fmin(bmin, fmax(-d1, q1 - hi));
        }
        for (uint64_t m = pos_mask; m; m &= m - 1) {
            const int j = __ffsll((unsigned long long)m) - 1;
            const double jx = wv_readlane_d(h.px, j), jy = wv_readlane_d(h.py, j), lo = wv_readlane_d(lo_l, j), hi = wv_readlane_d(hi_l, j);
            ax = x - jx; ay = y - jy;
            q1 = ax * ax + ay * ay;
            d1 = q1 - lo;
            cmin = fmin(cmin, d1);
            bmin = fmin(bmin, fmax(-d1, q1 - hi));
        }
        bool coll = cmin < 0.0;
        const bool unsure = bmin <= 0.0;
        if (__ballot(live && unsure && !coll) != 0ull) { // some square sat inside the band: the reference expression decides (all lanes walk again)
            const bool exact = collides_exact(x, y);
            if (unsure && !coll) coll = exact;
        }
        return coll;
    };
    // fp32 SCREEN in front of that walk.  A capped loop of a dense crowd is 65 536 candidates x ~100 points, and the walk above costs ~24
    // instructions per (candidate, point) of the one wavefront an env has.  In fp32, with two points as the two halves of packed
    // instructions, a pair of tests costs ~20: candidate and points rounded to float (|coordinate| < 32: 2^-20 absolute), the
    // square from a packed multiply + fma, compared with thresholds moved apart by 2e-5 relative -- several times what the roundings can
    // move a square near md^2 (|q32 - q| <= 2 |d| 3e-6 + 3e-7 q: 4e-6 relative at |d| ~ 1).  A candidate with some square below the lower
    // threshold collides, one with every square above the upper ones does not; anything else (a few candidates per million) sends the
    // batch through the fp64 walk.  Rounding of the thresholds themselves: 6e-8 relative, inside the 2e-5.
    typedef float f2 __attribute__((ext_vector_type(2)));
    const float lor32 = (float)(ddr * (1.0 - 2e-5)), hir32 = (float)(ddr * (1.0 + 2e-5));
    const float rpx32 = (float)rb.px, rpy32 = (float)rb.py, rgx32 = (float)rb.gx, rgy32 = (float)rb.gy;
    // the points that can block (goals first, then positions) are packed into consecutive lanes once per placement -- lane k keeps point k
    // and its thresholds -- so that the walk takes them two at a time without caring which human they belong to (~65 points in a dense
    // crowd mid-episode: 33 packed steps instead of 50 human-by-human ones)
    const int n_g = __popcll(goal_mask), n_p = __popcll(pos_mask), n_pts = n_g + n_p; // <= 128: two lists of <= 64
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    auto pack = [&](uint64_t mask, int cnt, float v) {
        // lane j with its bit set sends v to lane rank(j); the others to the lanes behind the list (a full permutation: no two senders share a lane)
        const bool on = (mask >> lane) & 1ull;
        const int dst = on ? __popcll(mask & below) : cnt + __popcll(~mask & below);
        return __int_as_float(__builtin_amdgcn_ds_permute(dst << 2, __float_as_int(v)));
    };
    const float lo32 = (float)(dd_l * (1.0 - 2e-5)), hi32 = (float)(dd_l * (1.0 + 2e-5));
    const float Gx = pack(goal_mask, n_g, (float)h.gx), Gy = pack(goal_mask, n_g, (float)h.gy), Gl = pack(goal_mask, n_g, lo32), Gh = pack(goal_mask, n_g, hi32);
    const float Px = pack(pos_mask, n_p, (float)h.px), Py = pack(pos_mask, n_p, (float)h.py), Pl = pack(pos_mask, n_p, lo32), Ph = pack(pos_mask, n_p, hi32);
    (void)n_pts;
    auto collides = [&](double x, double y, bool live) {
        const float xf = (float)x, yf = (float)y;
        const f2 xx = f2{xf, xf}, yy = f2{yf, yf};
        f2 ax = xx - f2{rgx32, rpx32}, ay = yy - f2{rgy32, rpy32};
        f2 q = ax * ax + ay * ay;
        float m1 = fminf(q.x, q.y) - lor32;          // min over the tests of (square - lower threshold): < 0 -> collides for certain
        float m2 = fminf(q.x, q.y) - hir32;          // min over the tests of (square - upper threshold): > 0 -> free for certain
        for (int k = 0; k < n_g; k += 2) {
            const int k1 = k + 1 < n_g ? k + 1 : k;  // (an odd list: the last point twice)
            const f2 jx = f2{wv_readlane(Gx, k), wv_readlane(Gx, k1)}, jy = f2{wv_readlane(Gy, k), wv_readlane(Gy, k1)};
            const f2 lo = f2{wv_readlane(Gl, k), wv_readlane(Gl, k1)}, hi = f2{wv_readlane(Gh, k), wv_readlane(Gh, k1)};
            ax = xx - jx; ay = yy - jy;
            q = ax * ax + ay * ay;
            const f2 dl = q - lo, dh = q - hi;
            m1 = fminf(m1, fminf(dl.x, dl.y));
            m2 = fminf(m2, fminf(dh.x, dh.y));
        }
        for (int k = 0; k < n_p; k += 2) {
            const int k1 = k + 1 < n_p ? k + 1 : k;
            const f2 jx = f2{wv_readlane(Px, k), wv_readlane(Px, k1)}, jy = f2{wv_readlane(Py, k), wv_readlane(Py, k1)};
            const f2 lo = f2{wv_readlane(Pl, k), wv_readlane(Pl, k1)}, hi = f2{wv_readlane(Ph, k), wv_readlane(Ph, k1)};
            ax = xx - jx; ay = yy - jy;
            q = ax * ax + ay * ay;
            const f2 dl = q - lo, dh = q - hi;
            m1 = fminf(m1, fminf(dl.x, dl.y));
            m2 = fminf(m2, fminf(dh.x, dh.y));
        }
        const bool hit = m1 < 0.0f, open = m2 > 0.0f;
        if (__ballot(live && !hit && !open) != 0ull) { // a square between the moved thresholds: fp64 decides (rare; all lanes walk)
            const bool c64 = collides64(x, y, live);
            return (hit || open) ? hit : c64;
        }
        return hit;
    };
    // one pass: candidates of lanes 0 .. nb-1 read from block `blk` -- whole candidates from word `first` on, or (first < 0) the candidate that
    // straddles the block boundary as lane 0 (its nt words of the previous block in tl, the rest from the start of blk) and whole candidates
    // behind it; returns the lanes whose candidate is taken (free, or past the bound)
    auto eval_pass = [&](const uint32_t *blk, int first, int nt, const uint32_t *tl, int nb, int attempt0, double &x, double &y) -> uint64_t {
        const bool live = lane < nb;
        const int need = 6 - nt; // words of the new block that complete the straddling candidate
        uint32_t wd[6];
        if (first >= 0) {
            const uint32_t *w = blk + first + 6 * (live ? lane : 0);
#pragma unroll
            for (int k = 0; k < 6; ++k) wd[k] = w[k];
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                // lane 0: tail words, then words 0 .. need - 1 of the new block; lane a >= 1: words need + 6 (a - 1) + k
                const int idx = lane == 0 ? (k < nt ? 0 : k - nt) : need + 6 * (lane - 1) + k;
                const uint32_t v = blk[idx];
                wd[k] = (lane == 0 && k < nt) ? tl[k < 5 ? k : 4] : v;
            }
        }
        const uint32_t a0 = mt_temper(wd[0]) >> 5, b0 = mt_temper(wd[1]) >> 6, a1 = mt_temper(wd[2]) >> 5, b1 = mt_temper(wd[3]) >> 6,
                       a2 = mt_temper(wd[4]) >> 5, b2 = mt_temper(wd[5]) >> 6;
        const double u0 = ((double)a0 * 67108864.0 + (double)b0) / 9007199254740992.0;
        const double u1 = ((double)a1 * 67108864.0 + (double)b1) / 9007199254740992.0;
        const double u2 = ((double)a2 * 67108864.0 + (double)b2) / 9007199254740992.0;
        make(u0, u1, u2, x, y);
        const bool coll = collides(x, y, live);
        return __ballot(live && (!coll || attempt0 + lane >= max_att));
    };
    int attempt = 0; // number of the next candidate
    DBG_ADD(4, 1);
    for (;;) {
        if constexpr (W > 1) {
            if (attempt >= s.coop_after) {
                CoopLds<W> &Q = coop_lds<W>();
#ifdef CN_POST_DEBUG
                const long long dbg_t0 = wall_clock64();
                DBG_ADD(2, 1);
#endif
                // candidates 64 p .. 64 p + 63 of the round whose first candidate starts at word `off` of `rb`, the exact way
                auto eval_ring = [&](const uint32_t *rb, int off, int att0, int p, double &x, double &y) -> uint64_t {
                    const uint32_t *w = rb + off + 6 * (64 * p + lane);
                    uint32_t wd[6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) wd[k] = w[k];
                    const uint32_t a0 = mt_temper(wd[0]) >> 5, b0 = mt_temper(wd[1]) >> 6, a1 = mt_temper(wd[2]) >> 5, b1 = mt_temper(wd[3]) >> 6,
                                   a2 = mt_temper(wd[4]) >> 5, b2 = mt_temper(wd[5]) >> 6;
                    const double u0 = ((double)a0 * 67108864.0 + (double)b0) / 9007199254740992.0;
                    const double u1 = ((double)a1 * 67108864.0 + (double)b1) / 9007199254740992.0;
                    const double u2 = ((double)a2 * 67108864.0 + (double)b2) / 9007199254740992.0;
                    make(u0, u1, u2, x, y);
                    const bool coll = collides(x, y, true);
                    return __ballot(!coll || att0 + 64 * p + lane >= max_att);
                };
                // the points for the coarse screen, two by two
                {
                    const float lo32c = (float)(dd_l * (1.0 - 1e-3));
                    const float Gc = pack(goal_mask, n_g, lo32c), Pc = pack(pos_mask, n_p, lo32c);
                    float *xy = reinterpret_cast<float *>(Q.pxy), *lo = reinterpret_cast<float *>(Q.plo);
                    auto put = [&](int slot, float x, float y, float l) {
                        xy[(slot >> 1) * 4 + (slot & 1)] = x; xy[(slot >> 1) * 4 + 2 + (slot & 1)] = y; lo[slot] = l;
                    };
                    const int n_s = 2 + n_g + n_p;
                    const float lorc = (float)(ddr * (1.0 - 1e-3));
                    if (lane == 0) { put(0, rgx32, rgy32, lorc); put(1, rpx32, rpy32, lorc); }
                    if (lane < n_g) put(2 + lane, Gx, Gy, Gc);
                    if (lane < n_p) put(2 + n_g + lane, Px, Py, Pc);
                    if (n_s & 1) { // (n_g + n_p is odd: the last point twice)
                        if (n_p > 0 ? lane == n_p - 1 : lane == n_g - 1) put(n_s, n_p > 0 ? Px : Gx, n_p > 0 ? Py : Gy, n_p > 0 ? Pc : Gc);
                    }
                    if (lane == 0) {
                        Q.kind = kind; Q.n_pairs = (n_s + 1) >> 1; Q.max_att = max_att; Q.circle_radius = (float)c.circle_radius; Q.vp = (float)vp;
                        Q.pos0 = R.pos; Q.attempt0 = attempt; Q.cmd = 1;
                    }
                }
                rng_sync();
                __syncthreads(); // the helpers wake up
                for (int k = threadIdx.x; k < MT_N; k += 64 * W) Q.buf[0][k] = R.mt[k]; // (all threads: block 0 = the staged block)
                __syncthreads();
                __syncthreads(); // the producer has made the first round's words
                constexpr int NG = CoopLds<W>::NG;
                int g0 = R.pos, bprev = 0;
                for (int round = 0;; ++round) {
                    const uint32_t *rb = Q.buf[round & 1];
                    const int off = g0 - MT_N * bprev;
                    double x, y;
                    uint64_t take = 0ull;
                    coop_screen_pass<W>(Q, rb, off, attempt, 0, lane, round, kind, (2 + n_g + n_p + 1) >> 1, max_att, (float)c.circle_radius, (float)vp);
                    __syncthreads(); // every wavefront's report is in (and the next round's words are made)
                    unsigned long long any = 0ull;
                    for (int p = 0; p < NG; ++p) any |= Q.take[round & 1][p];
                    if (any) {
                        int win = -1;
                        for (int p = 0; p < NG && win < 0; ++p) {
                            if (Q.take[round & 1][p] == 0ull) continue;
                            take = eval_ring(rb, off, attempt, p, x, y); // what the screen could not reject: exactly
                            if (take) win = p;
                        }
                        if (lane == 0) Q.verdict = win >= 0;
                        __syncthreads(); // the others learn whether the placement goes on
                        if (win >= 0) {
                            const int f = __ffsll((unsigned long long)take) - 1;
                            out_x = wv_readlane_d(x, f); out_y = wv_readlane_d(y, f);
                            // the staged state afterwards: the block that holds the last word read and the position behind that word
                            // (624 = "twist before the next draw", as the serial loop leaves it when a candidate ends a block)
                            const int g = g0 + 6 * (64 * win + f + 1);
                            const int bi = (g - 1) / MT_N;
                            rng_sync();
                            for (int k = lane; k < MT_N; k += 64) R.mt[k] = rb[(bi - bprev) * MT_N + k];
                            rng_sync();
                            R.pos = g - bi * MT_N;
#ifdef CN_POST_DEBUG
                            DBG_ADD(1, wall_clock64() - dbg_t0);
                            DBG_ADD(3, round + 1);
#endif
                            return;
                        }
                    }
                    bprev = (g0 + 384 * NG - 1) / MT_N;
                    g0 += 384 * NG;
                    attempt += 64 * NG;
                }
            }
        }
        const int left = MT_N - R.pos; // unread words of the current block
        int nb, first;                 // candidates of this pass; word index of lane 0's first word, or -1: lane 0 is the straddling candidate
        uint32_t tl[5] = {0u, 0u, 0u, 0u, 0u}; // the straddling candidate's words of the OLD block (raw, wave-uniform)
        int nt = 0;                                        // ... and how many there are
        if (left >= 6) {
            nb = left / 6 < 64 ? left / 6 : 64;
            first = R.pos;
        } else {
            // fewer than six words left: the next candidate straddles the end of the block (or starts the next one).  Its words of this
            // block are kept in registers, the block is regenerated, and the candidate is lane 0 of a pass whose other lanes take whole
            // candidates of the new block (as a pass of its own it cost a full walk for ONE candidate, every 104 candidates).
            nt = left;
            if (nt > 0) tl[0] = R.mt[R.pos];
            if (nt > 1) tl[1] = R.mt[R.pos + 1];
            if (nt > 2) tl[2] = R.mt[R.pos + 2];
            if (nt > 3) tl[3] = R.mt[R.pos + 3];
            if (nt > 4) tl[4] = R.mt[R.pos + 4];
            rng_twist(R, lane); // (R.pos = 0)
            nb = 64;            // 1 + (624 - 6) / 6 >= 64
            first = -1;
        }
        const int need = 6 - nt;
        double x, y;
        DBG_ADD(5, 1);
        const uint64_t take = eval_pass(R.mt, first, nt, tl, nb, attempt, x, y);
        // stream position behind candidate f of this pass
        if (take) {
            const int f = __ffsll((unsigned long long)take) - 1;
            out_x = wv_readlane_d(x, f); out_y = wv_readlane_d(y, f);
            R.pos = first >= 0 ? first + 6 * (f + 1) : need + 6 * f;
            return;
        }
        R.pos = first >= 0 ? first + 6 * nb : need + 6 * (nb - 1);
        attempt += nb;
    }
}

// the other wavefronts of an env: parked at the barrier until the master publishes a placement (place_by_rejection<W>), then round by
// round.  Waves 1 .. W - 2 (helpers) put candidates 64 wave .. 64 wave + 63 through the coarse screen and report what it cannot reject (the
// master decides those); wave W - 1 (producer) makes the next round's words meanwhile.
template <int W>
__device__ __forceinline__ void coop_helper_loop(int lane, int wave)
{
    constexpr int NG = CoopLds<W>::NG;
    CoopLds<W> &Q = coop_lds<W>();
    for (;;) {
        __syncthreads(); // a placement, or the end
        if (Q.cmd == 2) return;
        const int kind = Q.kind, n_pairs = Q.n_pairs, max_att = Q.max_att;
        const float circle_radius = Q.circle_radius, vp = Q.vp;
        int g0 = Q.pos0, attempt = Q.attempt0;
        for (int k = threadIdx.x; k < MT_N; k += 64 * W) Q.buf[0][k] = g_mt_lds[k];
        __syncthreads();
        if (wave == W - 1) { // ---- producer
            int bprev = 0, b1 = (g0 + 384 * NG - 1) / MT_N; // round 0 reads blocks 0 .. b1
            coop_produce(Q.buf[0], nullptr, lane, MT_N * b1);
            __syncthreads(); // the first round's words are made
            for (int round = 0;; ++round) {
                const int b2 = (g0 + 768 * NG - 1) / MT_N; // round + 1 reads blocks b1 .. b2
#ifdef CN_POST_DEBUG
                const long long dbg_p0 = wall_clock64();
#endif
                coop_produce(Q.buf[(round + 1) & 1], Q.buf[round & 1] + MT_N * (b1 - bprev), lane, MT_N * (b2 - b1));
#ifdef CN_POST_DEBUG
                DBG_ADD(7, wall_clock64() - dbg_p0);
#endif
                __syncthreads();
                unsigned long long any = 0ull;
                for (int p = 0; p < NG; ++p) any |= Q.take[round & 1][p];
                if (any) {
                    __syncthreads();
                    if (Q.verdict) break;
                }
                g0 += 384 * NG;
                bprev = b1; b1 = b2;
            }
            continue;
        }
        __syncthreads(); // the first round's words are made
        int bprev = 0;
        for (int round = 0;; ++round) {
#ifdef CN_POST_DEBUG
            const long long dbg_e0 = wall_clock64();
#endif
            coop_screen_pass<W>(Q, Q.buf[round & 1], g0 - MT_N * bprev, attempt, wave, lane, round, kind, n_pairs, max_att, circle_radius, vp);
#ifdef CN_POST_DEBUG
            if (wave == 1) DBG_ADD(6, wall_clock64() - dbg_e0);
#endif
            __syncthreads(); // every wavefront's report is in (and the next round's words are made)
            unsigned long long any = 0ull;
            for (int p = 0; p < NG; ++p) any |= Q.take[round & 1][p];
            if (any) {
                __syncthreads(); // the master has looked at the reports
                if (Q.verdict) break;
            }
            bprev = (g0 + 384 * NG - 1) / MT_N;
            g0 += 384 * NG;
            attempt += 64 * NG;
        }
    }
}

// crowd_sim_var_num.py:116-146 generate_circle_crossing_human (+ Agent.__init__/sample_random_attributes draws).
// All lanes compute the candidate position identically; the min-distance test against the existing agents is
// lane-parallel.  n_existing = number of humans currently in self.humans (slot itself included on respawn, :455).
template <int W = 1, class S>
__device__ __forceinline__ void gen_human(const S &s, Rng &R, int lane, int slot, int n_existing, const Robot &rb, Lane &h, double &shared_nd)
{
    const auto &c = s.cfg;
    double radius = c.human_radius, vpref = c.human_v_pref;
    if (c.randomize_attributes) {
        shared_nd = rng_uniform(R, lane, 5.0, 10.0); // agent.py:21-22
        vpref = rng_uniform(R, lane, 0.5, 1.5);      // agent.py:49
        radius = rng_uniform(R, lane, 0.3, 0.5);     // agent.py:50
    }
    double px, py;
    // (unbounded in the reference: see CN_MAX_PLACEMENT_ATTEMPTS)
    // :133-136: a unicycle robot keeps new humans half a circle radius away from its start and goal
    const double md_r = c.kinematics == CN_KIN_UNICYCLE ? c.circle_radius / 2.0 : radius + c.robot_radius + c.discomfort_dist;
    place_by_rejection<W>(s, R, lane, 0, radius, 0.0, md_r, n_existing, -1, rb, h, px, py);
    if (lane == slot) {
        h.px = px; h.py = py; h.gx = -px; h.gy = -py; h.vx = 0.0; h.vy = 0.0; h.rad = radius; h.vpref = vpref;
        h.simv = 0; // new Human -> new ORCA object, sim rebuilt on next use
    }
}

// crowd_sim.py:415-450 update_human_goals_randomly (every human, goal_change_chance) and :453-485 update_human_goal (one human,
// end_goal_change_chance: `only` >= 0 selects it)
template <int W = 1, class S>
__device__ __forceinline__ void change_goals(const S &s, Rng &R, int lane, int n, const Robot &rb, Lane &h, int only = -1)
{
    const auto &c = s.cfg;
    const int H = n; // the humans present
    for (int i = only >= 0 ? only : 0; i < (only >= 0 ? only + 1 : H); ++i) {
        double vp_i = __shfl(h.vpref, i, 64);
        const double rad_i = __shfl(h.rad, i, 64);
        if (only < 0 && vp_i == 0.0) continue;
        if (vp_i == 0.0) vp_i = 1.0;
        if (rng_double(R, lane) <= (only >= 0 ? c.end_goal_change_chance : c.goal_change_chance)) {
            double gx, gy;
            place_by_rejection<W>(s, R, lane, 1, rad_i, vp_i, rad_i + c.robot_radius + c.discomfort_dist, H, i, rb, h, gx, gy);
            if (lane == i) { h.gx = gx; h.gy = gy; }
        }
    }
}

// detect_visible(robot, human, robot1=True), crowd_sim.py:513-552: inside the robot's field of view (FOV = 2*pi: iff not coincident) and
// within sensor range; `present`: the slot holds a human.  The observation (write_obs) and cn_env_get_visibility both decide with this function.
template <class C>
__device__ __forceinline__ bool robot_sees(const C &c, const Robot &rb, bool present, double hpx, double hpy, double hrad)
{
    const double dx = rb.px - hpx, dy = rb.py - hpy;
    bool vis = present && !(dx == 0.0 && dy == 0.0) && (norm2(dx, dy) - c.robot_radius - hrad <= c.sensor_range);
    if (c.robot_fov < 2.0) vis = vis && in_fov(c, c.robot_fov, rb.px, rb.py, rb.vx, rb.vy, rb.theta, hpx, hpy);
    return vis;
}

// crowd_sim_var_num.py:233-279 generate_ob / crowd_sim_pred.py:62-97 / crowd_sim_pred_real_gst.py:76-93,
// crowd_sim.py:558-572 get_num_human_in_fov, :243-273 update_last_human_states.
template <class S>
__device__ __forceinline__ void write_obs(const S &s, int e, int lane, int n, bool reset, const Robot &rb, Lane &h, const cn_obs &ob, int step_counter)
{
    const auto &c = s.cfg;
    const int H = s.H, D = s.D, P = s.P; // H observation rows (crowd_sim_var_num.py:249, crowd_sim_pred.py:78), n humans present
    const bool isH = lane < n, isRow = lane < H;
    const bool vis = robot_sees(c, rb, isH, h.px, h.py, h.rad);
    const uint64_t vmask = __ballot(vis);
    const int num_visible = __popcll(vmask);
    if (s.vis && isRow) s.vis[(size_t)e * H + lane] = vis ? 1 : 0; // human_visibility, read by the next step's 'truth' blanking
    if (s.nh && c.env_kind != CN_ENV_PRED && lane == 0) {
        // observed_human_ids (crowd_sim_var_num.py:275): who may not leave at the next crowd-size change.  CrowdSimPred's own
        // generate_ob never refreshes the list (it stays [] from reset)
        s.obs_cnt[e] = num_visible;
        s.obs_max[e] = vmask ? 63 - __clzll((long long)vmask) : -1;
    }
    const double prev_vx = h.l2, prev_vy = h.l3;
    if (vis) { h.l0 = h.px; h.l1 = h.py; h.l2 = h.vx; h.l3 = h.vy; h.l4 = h.rad; }
    else if (isH && reset) { h.l0 = 15.0; h.l1 = 15.0; h.l2 = 0.0; h.l3 = 0.0; h.l4 = 0.3; }
    else if (isH) { h.l0 = h.l0 + h.l2 * c.time_step; h.l1 = h.l1 + h.l3 * c.time_step; }
    if (lane == 0) {
        float *rn = ob.robot_node + (size_t)e * 7;
        rn[0] = (float)rb.px; rn[1] = (float)rb.py; rn[2] = (float)c.robot_radius; rn[3] = (float)rb.gx; rn[4] = (float)rb.gy;
        rn[5] = (float)c.robot_v_pref; rn[6] = (float)rb.theta;
        ob.temporal_edges[(size_t)e * 2] = (float)rb.vx; ob.temporal_edges[(size_t)e * 2 + 1] = (float)rb.vy;
        ob.detected_human_num[e] = (float)(num_visible == 0 ? 1 : num_visible);
    }
    if (c.env_kind == CN_ENV_COLLECT) {
        // crowd_sim_var_num_collect.py:100-133: humans that were visible at the last observation and are not now get fresh prediction
        // ids (ascending, in list order); row i = (frame, id, ABSOLUTE believed position) if visible, (frame, id, inf, inf) otherwise
        const bool was = isRow && s.last_obs[(size_t)e * H + lane] != 0;
        const bool out = isH && was && !vis;
        const uint64_t omask = __ballot(out);
        const int base = s.max_pid[e];
        int pid = isRow ? s.pred_id[(size_t)e * H + lane] : 0;
        if (out) pid = base + __popcll(omask & ((1ull << lane) - 1ull));
        if (isRow) {
            s.pred_id[(size_t)e * H + lane] = pid;
            s.last_obs[(size_t)e * H + lane] = vis ? 1 : 0;
            float *se = ob.spatial_edges + ((size_t)e * H + lane) * 4;
            se[0] = (float)(((double)step_counter * c.time_step) / c.time_step); // global_time / data.pred_timestep (== env.time_step)
            se[1] = (float)pid;
            se[2] = vis ? (float)h.l0 : INFINITY;
            se[3] = vis ? (float)h.l1 : INFINITY;
            if (ob.visible_masks) ob.visible_masks[(size_t)e * H + lane] = vis ? 1 : 0;
        }
        if (lane == 0 && omask) s.max_pid[e] = base + __popcll(omask);
        return;
    }
    const double ex = h.l0 - rb.px, ey = h.l1 - rb.py; // == true relative position for visible humans
    const bool do_sort = c.sort_humans && c.env_kind != CN_ENV_PRED_GST;
    int row = lane;
    if (do_sort) {
        // sorted(key = norm(first two)) is stable, invisible rows (inf) keep index order and go last
        const double key = vis ? sqrt(ex * ex + ey * ey) : INFINITY;
        int rank = 0;
        for (int m = 0; m < H; ++m) {
            // (m is wave-uniform: a pinned view reads lane m with two v_readlane instead of two ds_bpermute round trips -- the same word)
            double km;
            if constexpr (view_pinned<S>) km = wv_readlane_d(key, m);
            else km = __shfl(key, m, 64);
            rank += (km < key || (km == key && m < lane)) ? 1 : 0;
        }
        row = rank;
    }
    if (isRow) {
        float *se = ob.spatial_edges + ((size_t)e * H + row) * D;
        if (c.env_kind == CN_ENV_VARNUM) {
            se[0] = vis ? (float)ex : 15.0f;
            se[1] = vis ? (float)ey : 15.0f;
        } else {
            double *ft = s.ftraj ? s.ftraj + (size_t)e * P * 2 * H : nullptr;
            const double *tre = c.predict_truth ? s.tr + (size_t)e * (s.R + 1) * 4 * H : nullptr;
            for (int k = 0; k <= P; ++k) {
                double fx = 15.0, fy = 15.0;
                if (vis && tre && k >= 1) {
                    // sim.predict_method = 'truth' (crowd_sim_pred.py:81 -> crowd_sim_var_num.py:180-206): the humans' own ORCA rolled
                    // forward from the state just reached, computed by orca_truth_kernel between the two halves of the step
                    fx = tre[(k * s.I * 4 + 0) * H + lane]; // human_future_traj[::pred_interval] (crowd_sim_var_num.py:206)
                    fy = tre[(k * s.I * 4 + 1) * H + lane];
                } else if (vis) {
                    const double t = (double)k * c.time_step * (double)s.I; // arange(P + 1) * time_step * pred_interval (crowd_sim_var_num.py:212)
                    fx = h.px + t * prev_vx;
                    fy = h.py + t * prev_vy;
                }
                if (ft && k >= 1) { ft[((k - 1) * 2 + 0) * H + lane] = fx; ft[((k - 1) * 2 + 1) * H + lane] = fy; }
                if (c.env_kind == CN_ENV_PRED) {
                    se[2 * k] = vis ? (float)(fx - rb.px) : 15.0f;
                    se[2 * k + 1] = vis ? (float)(fy - rb.py) : 15.0f;
                } else {
                    se[2 * k] = vis ? (float)ex : 15.0f;
                    se[2 * k + 1] = vis ? (float)ey : 15.0f;
                }
            }
        }
        if (ob.visible_masks) {
            uint8_t *vm = ob.visible_masks + (size_t)e * H;
            if (do_sort) vm[lane] = lane < num_visible ? 1 : 0;
            else vm[lane] = vis ? 1 : 0;
        }
    }
}

// crowd_sim_var_num.py:303-363 reset (seed, robot, humans, potential, first observation)
// the RNG-consuming part of reset(): seed, robot, humans (crowd_sim_var_num.py:333-340, :64-146)
// (case_counter: the caller's copy of s.case_counter[e])
template <class S>
__device__ __forceinline__ void gen_episode_head(const S &s, Rng &R, int e, int lane, uint64_t case_counter, Robot &rb, int &n)
{
    const auto &c = s.cfg;
    const uint64_t offset = c.phase == CN_PHASE_TRAIN ? 2000ull : (c.phase == CN_PHASE_VAL ? 0ull : 1000ull);
    const uint64_t seed = offset + case_counter + (uint64_t)(s.seed_base + e);
    rng_seed(R, (uint32_t)seed, lane);
    double px, py, gx, gy;
    if (c.kinematics == CN_KIN_UNICYCLE) {
        // generate_robot_humans, sim2real branch :78-91: start on the arena circle, goal >= 4 m away, random heading,
        // 1 .. human_num + human_num_range humans
        const double angle = rng_uniform(R, lane, 0.0, M_PI * 2.0);
        double sn, cs;
        det_sincos(angle, sn, cs);
        px = c.arena_size * cs; py = c.arena_size * sn;
        for (;;) {
            gx = rng_uniform(R, lane, -c.arena_size, c.arena_size);
            gy = rng_uniform(R, lane, -c.arena_size, c.arena_size);
            if (norm2(px - gx, py - gy) >= 4.0) break;
        }
        rb.theta = rng_uniform(R, lane, 0.0, 2.0 * M_PI);
        n = rng_randint(R, lane, 1, c.human_num + c.human_num_range + 1);
    } else {
        for (;;) { // :97-100
            px = rng_uniform(R, lane, -c.arena_size, c.arena_size);
            py = rng_uniform(R, lane, -c.arena_size, c.arena_size);
            gx = rng_uniform(R, lane, -c.arena_size, c.arena_size);
            gy = rng_uniform(R, lane, -c.arena_size, c.arena_size);
            if (norm2(px - gx, py - gy) >= 8.0) break;
        }
        rb.theta = M_PI / 2.0;
        // :103-104 randint(human_num - range, human_num + range + 1): consumes no draw when human_num_range == 0
        n = rng_randint(R, lane, c.human_num - c.human_num_range, c.human_num + c.human_num_range + 1);
    }
    rb.px = px; rb.py = py; rb.gx = gx; rb.gy = gy; rb.vx = 0.0; rb.vy = 0.0;
}
template <class S>
__device__ __forceinline__ void gen_episode(const S &s, Rng &R, int e, int lane, uint64_t case_counter, Robot &rb, Lane &h, double &shared_nd, int &n)
{
    gen_episode_head(s, R, e, lane, case_counter, rb, n);
    for (int i = 0; i < n; ++i) gen_human(s, R, lane, i, i, rb, h, shared_nd);
    rb.pot = -fabs(norm2(rb.gx - rb.px, rb.gy - rb.py));
}

// The start of an episode from the state in (rb, h), whoever made that state -- the generator (finish_reset) or the caller
// (env_scene_kernel): belief cleared (:108), step counter and episode statistics zeroed, observation memory emptied, first observation.
// Nothing here touches the MT19937 stream, the case counter or the staged next episode.
template <class S>
__device__ __forceinline__ void start_episode(const S &s, int e, int lane, int n, Robot &rb, Lane &h, const cn_obs &ob, bool with_obs)
{
    h.l0 = h.l1 = h.l2 = h.l3 = h.l4 = 0.0;
    if (lane == 0) {
        s.step_counter[e] = 0; s.ep_ret[e] = 0.0; s.ep_cnt[e] = 0;
        if (s.nh) { s.obs_cnt[e] = 0; s.obs_max[e] = -1; } // :327 observed_human_ids = []
        if (s.max_pid) s.max_pid[e] = n; // crowd_sim_var_num_collect.py:79-81
    }
    if (s.pred_id && lane < s.H) { s.pred_id[(size_t)e * s.H + lane] = lane; s.last_obs[(size_t)e * s.H + lane] = 0; }
    if (with_obs) write_obs(s, e, lane, n, true, rb, h, ob, 0);
}

// the rest of reset(): what follows from np.random.seed and the case bookkeeping (:348), then the start of the episode
template <class S>
__device__ __forceinline__ void finish_reset(const S &s, int e, int lane, int n, uint64_t case_counter, Robot &rb, Lane &h, const cn_obs &ob, bool with_obs = true)
{
    const auto &c = s.cfg;
    const uint64_t case_size = c.phase == CN_PHASE_TRAIN ? (4294967295ull - 2000ull) : (c.phase == CN_PHASE_VAL ? c.val_size : c.test_size);
    if (lane == 0) {
        s.case_counter[e] = (case_counter + (uint64_t)c.nenv) % case_size;
        if (s.wheel) { s.wheel[(size_t)e * 4 + 2] = 0.0; s.wheel[(size_t)e * 4 + 3] = 0.0; } // np.random.seed -> _legacy_seeding: has_gauss = 0
    }
    start_episode(s, e, lane, n, rb, h, ob, with_obs);
}

// crowd_sim_var_num.py:303-363 reset.  Uses the pre-generated episode when the side stream has one ready (nx_ready and case_counter: the
// caller's copies of s.nx_ready[e] and s.case_counter[e]).  The staged episode is read in ONE batch: its MT19937 state goes straight into
// R.mt (whatever that held is dead) while the records are loaded into the registers of the episode that just ended.
template <class S>
__device__ __forceinline__ void do_reset(const S &s, Rng &R, int e, int lane, bool nx_ready, uint64_t case_counter, Robot &rb, Lane &h,
                                         double &shared_nd, int &n, const cn_obs &ob, bool with_obs = true)
{
    if (nx_ready) {
        rng_sync();
        mt_dma(R.mt, s.nx_mt + (size_t)e * MT_N, lane);
        const int pos = s.nx_mt_pos[e];
        n = s.nx_nh ? s.nx_nh[e] : s.H;
        const int H = s.H;
        const int lj = lane < H ? lane : 0;
        const double *hum = s.nx_hum + (size_t)e * 8 * H;
        h.px = hum[F_PX * H + lj]; h.py = hum[F_PY * H + lj]; h.vx = 0.0; h.vy = 0.0;
        h.gx = hum[F_GX * H + lj]; h.gy = hum[F_GY * H + lj]; h.rad = hum[F_RAD * H + lj]; h.vpref = hum[F_VPREF * H + lj];
        h.simv = 0;
        const double *r = s.nx_rob + (size_t)e * 8;
        rb.px = r[R_PX]; rb.py = r[R_PY]; rb.vx = 0.0; rb.vy = 0.0; rb.gx = r[R_GX]; rb.gy = r[R_GY]; rb.theta = r[R_THETA]; rb.pot = r[R_POT];
        shared_nd = s.nx_shared_nd[e];
        mt_dma_wait();
        R.pos = pos;
        R.loaded = true;
        rng_sync();
        if (lane == 0) s.nx_ready[e] = 0;
    } else {
        gen_episode(s, R, e, lane, case_counter, rb, h, shared_nd, n);
    }
    finish_reset(s, e, lane, n, case_counter, rb, h, ob, with_obs);
}

template <class S>
__device__ __forceinline__ void load_env(const S &s, int e, int lane, Robot &rb, Lane &h)
{
    const int H = s.H;
    const int lj = lane < H ? lane : 0;
    const double *hum = s.hum + (size_t)e * 8 * H;
    h.px = hum[F_PX * H + lj]; h.py = hum[F_PY * H + lj]; h.vx = hum[F_VX * H + lj]; h.vy = hum[F_VY * H + lj];
    h.gx = hum[F_GX * H + lj]; h.gy = hum[F_GY * H + lj]; h.rad = hum[F_RAD * H + lj]; h.vpref = hum[F_VPREF * H + lj];
    const double *l = s.lhs + (size_t)e * 5 * H;
    h.l0 = l[lj]; h.l1 = l[H + lj]; h.l2 = l[2 * H + lj]; h.l3 = l[3 * H + lj]; h.l4 = l[4 * H + lj];
    h.simv = s.sim_valid[(size_t)e * H + lj];
    const double *r = s.rob + (size_t)e * 8;
    rb.px = r[R_PX]; rb.py = r[R_PY]; rb.vx = r[R_VX]; rb.vy = r[R_VY]; rb.gx = r[R_GX]; rb.gy = r[R_GY]; rb.theta = r[R_THETA]; rb.pot = r[R_POT];
}
template <class S>
__device__ __forceinline__ void store_env(const S &s, int e, int lane, const Robot &rb, const Lane &h)
{
    const int H = s.H;
    if (lane < H) {
        double *hum = s.hum + (size_t)e * 8 * H;
        hum[F_PX * H + lane] = h.px; hum[F_PY * H + lane] = h.py; hum[F_VX * H + lane] = h.vx; hum[F_VY * H + lane] = h.vy;
        hum[F_GX * H + lane] = h.gx; hum[F_GY * H + lane] = h.gy; hum[F_RAD * H + lane] = h.rad; hum[F_VPREF * H + lane] = h.vpref;
        double *l = s.lhs + (size_t)e * 5 * H;
        l[lane] = h.l0; l[H + lane] = h.l1; l[2 * H + lane] = h.l2; l[3 * H + lane] = h.l3; l[4 * H + lane] = h.l4;
        s.sim_valid[(size_t)e * H + lane] = h.simv;
    }
    if (lane == 0) {
        double *r = s.rob + (size_t)e * 8;
        r[R_PX] = rb.px; r[R_PY] = rb.py; r[R_VX] = rb.vx; r[R_VY] = rb.vy; r[R_GX] = rb.gx; r[R_GY] = rb.gy; r[R_THETA] = rb.theta; r[R_POT] = rb.pot;
    }
}

// the body of env_pregen_kernel (env_sim.hip): one wavefront, one env; R.mt = that wavefront's 624-word LDS slice
template <int W = 1, class S>
__device__ __forceinline__ void pregen_env(const S &s, int e, int lane, long long budget, Rng &R)
{
    if (s.nx_ready[e]) return;
    const long long t0 = wall_clock64();
    const int H = s.H;
    int prog = s.nx_prog[e];
    if (prog > 0 && s.nx_case[e] != s.case_counter[e]) prog = 0;
    Robot rb{};
    Lane h{};
    h.rad = s.cfg.human_radius;
    double shared_nd = s.shared_nd[e]; // overwritten by the first Human() when randomised, unused otherwise
    int n = H;
    if (prog == 0) {
        const uint64_t case_counter = s.case_counter[e];
        gen_episode_head(s, R, e, lane, case_counter, rb, n);
        if (lane == 0) s.nx_case[e] = case_counter;
        prog = 1;
    } else {
        const int lj = lane < H ? lane : 0;
        const double *hum = s.nx_hum + (size_t)e * 8 * H;
        h.px = hum[F_PX * H + lj]; h.py = hum[F_PY * H + lj]; h.gx = hum[F_GX * H + lj]; h.gy = hum[F_GY * H + lj];
        h.rad = hum[F_RAD * H + lj]; h.vpref = hum[F_VPREF * H + lj];
        const double *r = s.nx_rob + (size_t)e * 8;
        rb.px = r[R_PX]; rb.py = r[R_PY]; rb.gx = r[R_GX]; rb.gy = r[R_GY]; rb.theta = r[R_THETA];
        shared_nd = s.nx_shared_nd[e];
        n = s.nx_nh ? s.nx_nh[e] : H;
        rng_sync();
        for (int k = lane; k < MT_N; k += 64) R.mt[k] = s.nx_mt[(size_t)e * MT_N + k];
        R.pos = s.nx_mt_pos[e];
        R.loaded = true;
        rng_sync();
    }
    bool complete = true;
    for (int i = prog - 1; i < n; ++i) {
        gen_human<W>(s, R, lane, i, i, rb, h, shared_nd);
        if (i + 1 < n && __builtin_amdgcn_readfirstlane((int)(wall_clock64() - t0 > budget))) { prog = i + 2; complete = false; break; }
    }
    if (complete) rb.pot = -fabs(norm2(rb.gx - rb.px, rb.gy - rb.py));
    if (lane < H) {
        double *hum = s.nx_hum + (size_t)e * 8 * H;
        hum[F_PX * H + lane] = h.px; hum[F_PY * H + lane] = h.py; hum[F_GX * H + lane] = h.gx; hum[F_GY * H + lane] = h.gy;
        hum[F_RAD * H + lane] = h.rad; hum[F_VPREF * H + lane] = h.vpref;
    }
    if (lane == 0) {
        double *r = s.nx_rob + (size_t)e * 8;
        r[R_PX] = rb.px; r[R_PY] = rb.py; r[R_GX] = rb.gx; r[R_GY] = rb.gy; r[R_THETA] = rb.theta; r[R_POT] = rb.pot;
        s.nx_shared_nd[e] = shared_nd;
        s.nx_mt_pos[e] = R.pos;
        if (s.nx_nh) s.nx_nh[e] = n;
        s.nx_prog[e] = complete ? 0 : prog;
    }
    rng_sync();
    for (int k = lane; k < MT_N; k += 64) s.nx_mt[(size_t)e * MT_N + k] = R.mt[k];
    __threadfence(); // the staging is complete before the flag says so (the flag's readers run in later launches; belt and braces)
    if (lane == 0 && complete) s.nx_ready[e] = 1;
}

// goal changes every 5 s and respawns of the humans that reached their goal (crowd_sim_var_num.py:446-456): after the observation
template <int W = 1, class S>
__device__ __forceinline__ void post_obs_updates(const S &s, Rng &R, int e, int lane, int n, int step_counter, const Robot &rb, Lane &h, double &shared_nd)
{
    const auto &c = s.cfg;
    const int H = n; // the humans present
    const bool isH = lane < H;
    const int period = (int)(5.0 / c.time_step + 0.5);
    if (c.random_goal_changing && (step_counter % period) == 0) {
        rng_load(R, s, e, lane);
        change_goals<W>(s, R, lane, n, rb, h);
    }
    if (c.end_goal_changing) {
        uint64_t reached = __ballot(isH && norm2(h.gx - h.px, h.gy - h.py) < h.rad);
        if (reached) rng_load(R, s, e, lane);
        while (reached) {
            const int i = __ffsll((unsigned long long)reached) - 1;
            reached &= reached - 1;
            // :451-456 respawned (holonomic robot) or given a new goal (unicycle robot)
            // (crowd_sim_pred.py:208-212 always respawns)
            if (c.kinematics == CN_KIN_UNICYCLE && c.env_kind == CN_ENV_VARNUM) change_goals<W>(s, R, lane, n, rb, h, i);
            else gen_human<W>(s, R, lane, i, H, rb, h, shared_nd);
        }
    }
}

} // namespace
