// env_sim.hip -- batched CrowdNav++ simulator on gfx950: ORCA humans, reward / termination, observation assembly,
// numpy-compatible scenario generation and auto-reset, all device resident.
//
// Compile with -ffp-contract=off: ORCA follows RVO2's fp32 operation order (no FMA), positions are fp64 like the
// Python reference, so results are reproducible bit for bit against the scalar CPU restatement used by the tests.
// The simulator is ONE translation unit: its device code is split into headers that only this file includes, so the flag covers them.
//
// Files:
//   env_dev.h    EnvDev (the per-env arrays a launch receives by value), Lp3Hdr, the F_* / R_* field enums
//   env_profile.h  compile-time config profiles: the view of EnvDev the device code reads (generic = EnvDev; ProfileTrain pins the default training class)
//   det_math.h   deterministic sin/cos, exp and log (+,-,*,/ only), the field-of-view test
//   orca.h       RVO2's linear programs and every ORCA kernel listed below (it also brings in row_plan.h, for the lane kernel)
//   mt19937.h    numpy's legacy RandomState stream (Rng), staged in LDS
//   episode.h    placement by rejection (one wavefront or a workgroup), episode generation, reset, observation writing,
//                next-episode staging (pregen_env), the post-observation goal changes / respawns
//   env_sim.hip  the episode and step kernels, the export / fill kernels, cn_env_batch, the stream and event hand-offs
//                (prefetch_orca, launch_tail, launch_post, launch_pregen, sync_side) and the cn_env_* / cn_orca_solve ABI
//
// Mapping (one wavefront = 64 lanes everywhere in the simulator; a lane is a human):
//   orca_lane_kernel   (orca.h) one LANE per (env, human i) for crowds of <= 32 agents: neighbour keys ordered by a sorting
//                      network, ORCA lines and linearProgram2 in per-lane register vectors; the agents whose program is
//                      infeasible (about a third in a dense crossing) hand their lines to
//   orca_lp3_kernel    (orca.h) two such agents per wavefront, lane k of a half = line k: RVO2's linearProgram3 (the outer loop
//                      over lines is its serial dependence; the inner clip of a line against all earlier lines is one lane-parallel
//                      min/max reduction)
//   orca_kernel        (orca.h) the whole solve one wavefront per agent (crowds of more than 32 agents)
//   orca_truth_kernel  (orca.h) the 'truth' roll-outs (sim.predict_method = 'truth') of ORCA humans: one wavefront per agent,
//                      one launch per roll
//   sf_truth_kernel    (orca.h) the same roll-outs of social-force humans: one wavefront per env walks all rolls in one launch
//   orca_solve_kernel  (orca.h) the stand-alone batched solve behind cn_orca_solve
//   env_step_kernel    one wavefront per env: robot clip + reward/collision (lane-parallel distances, ballot/any),
//                      kinematics, visibility, belief update, distance rank sort + observation scatter, goal changes,
//                      respawns and the in-launch auto-reset.  The MT19937 stream of the env lives in HBM ([E][624]) and
//                      is staged into LDS only by the (rare) wavefronts that draw from it; the 624-word twist is
//                      lane-parallel.
//   env_reset_kernel   reset (cn_env_reset);  env_pregen_kernel: next-episode staging on the side stream;
//   env_scene_kernel   an episode started from the caller's records (cn_env_set_scene): a reset without the generator;
//   env_post_kernel    the post-observation updates env_step_kernel deferred;  env_obs_kernel: second half of a split step
// Reference semantics (file:line under the reference repo) are cited at each block.
#include "common.h"
#include "env_dev.h"
#include "env_profile.h"
#include "det_math.h"
#include "orca.h"
#include "mt19937.h"
#include "episode.h"

#include <hip/hip_ext.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>

namespace {

__global__ __launch_bounds__(64) void env_reset_kernel(EnvDev s, cn_obs ob, int with_obs)
{
    const int lane = threadIdx.x;
    const int e = blockIdx.x;
    Rng R{MT_N, false};
    Robot rb{};
    Lane h{};
    h.rad = s.cfg.human_radius;
    double shared_nd = s.cfg.orca_neighbor_dist;
    int n = s.H;
    if (e == 0 && lane == 0) *s.lp3_cnt = 0; // the ORCA pass that follows starts with an empty linearProgram3 list
    const bool nx_ready = s.nx_ready[e] != 0;
    const uint64_t case_counter = s.case_counter[e];
    do_reset(s, R, e, lane, nx_ready, case_counter, rb, h, shared_nd, n, ob, with_obs != 0);
    if (!with_obs && lane == 0) s.pend[e] = 1;
    store_env(s, e, lane, rb, h);
    if (lane == 0) { s.shared_nd[e] = shared_nd; if (s.nh) s.nh[e] = n; }
    rng_store(R, s, e, lane);
}

// cn_env_set_scene: the selected envs start an episode from the caller's records (humans [E][H][8], robot [E][8]: cn_env_get_state's layout).
// One wavefront per env, a lane per human, as in env_reset_kernel; start_episode (episode.h) is the half of a reset that does not generate.
// Taken: px, py, vx, vy, gx, gy of the humans present, px, py, vx, vy, gx, gy, theta of the robot.  Kept: radius / v_pref (the private ORCA
// simulators froze them: sim_valid stays as it is), the crowd size, the MT19937 stream (never loaded here, so no rng_store), the case counter,
// the staged next episode.  An env that is not selected is neither loaded nor stored, and its observation rows are not written: write_obs
// advances the belief of every human the robot does not see (l0 += l2 * time_step) and overwrites the previous velocities the const-vel
// predictor reads, so a second observation of an unchanged state would not leave the env as it was.
__global__ __launch_bounds__(64) void env_scene_kernel(EnvDev s, const uint8_t *select, const double *humans, const double *robot, cn_obs ob, int with_obs)
{
    const int lane = threadIdx.x;
    const int e = blockIdx.x;
    if (e == 0 && lane == 0) *s.lp3_cnt = 0; // the ORCA pass that follows starts with an empty linearProgram3 list
    if (select && !select[e]) return;
    Robot rb;
    Lane h;
    load_env(s, e, lane, rb, h);
    const int H = s.H;
    const int n = crowd_size(s, e);
    if (lane < n) {
        const double *src = humans + ((size_t)e * H + lane) * 8;
        h.px = src[F_PX]; h.py = src[F_PY]; h.vx = src[F_VX]; h.vy = src[F_VY]; h.gx = src[F_GX]; h.gy = src[F_GY];
    }
    const double *r = robot + (size_t)e * 8;
    rb.px = r[R_PX]; rb.py = r[R_PY]; rb.vx = r[R_VX]; rb.vy = r[R_VY]; rb.gx = r[R_GX]; rb.gy = r[R_GY]; rb.theta = r[R_THETA];
    rb.pot = -fabs(norm2(rb.gx - rb.px, rb.gy - rb.py)); // as gen_episode
    start_episode(s, e, lane, n, rb, h, ob, with_obs != 0);
    if (!with_obs && lane == 0) s.pend[e] = 1;
    store_env(s, e, lane, rb, h);
}

// Generates the NEXT episode of every env whose staging slot is empty (side stream, overlapped with the policy forward).
// The wavefronts of this kernel keep registers on their CUs, and the policy's human-human kernel (next on the caller's stream) needs
// every register of a CU to place a workgroup there: an env whose rejection sampling runs long (the tail reaches 150 us) used to hold
// one CU back for that long and with it the whole launch.  So the work is BUDGETED: a wavefront that has not finished after
// `budget` ticks of the 100 MHz clock saves where it is -- the staging arrays hold exactly the state between two humans -- and the
// next launch resumes there.  The episode is the same whichever way it is cut; an env that resets before its staging is complete
// generates in place, as it always could, and the stale staging is restarted (nx_case).
// (Round 5 measured this generator INSIDE the ORCA tail's launch, i.e. behind the human-human kernel instead of beside the lane kernel, so
// that it no longer holds ~60 CUs when that kernel starts: the kernel got 17 us shorter (all its workgroups start within 8 us) and the
// step 4 % LONGER -- its workgroups then end together, and the 20 us in which the tail used to run on the CUs of the early finishers are
// gone; profiles/HISTORY.md section 10.)
// (W > 1: with the helper wavefronts of place_by_rejection<W>, as in env_step_kernel; not launched -- see launch_pregen)
template <int W = 1>
__global__ __launch_bounds__(64 * W) void env_pregen_kernel(EnvDev s, long long budget)
{
    const CnStampScope stamp_scope(s.stamp);
    const int lane = threadIdx.x & 63;
    if constexpr (W > 1) {
        if (threadIdx.x >= 64) { coop_helper_loop<W>(lane, __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))); return; }
    }
    Rng R{MT_N, false};
    pregen_env<W>(s, blockIdx.x, lane, budget, R);
    if constexpr (W > 1) { // release the helpers
        if (lane == 0) coop_lds<W>().cmd = 2;
        __syncthreads();
    }
}

// The deferred post-observation updates of env_step_kernel<false, 1, true>: one workgroup of W wavefronts per listed env (the list is short:
// an env changes goals every 5 s, so ~1/20 of a dephased batch, plus the envs where a human reached its goal), the placement loops on all
// W of them (place_by_rejection<W>).  Same state in, same state out as the in-kernel call: load_env / store_env are exact.
template <int W>
__global__ __launch_bounds__(64 * W) void env_post_kernel(EnvDev s)
{
    if ((int)blockIdx.x >= *s.post_cnt) return;
    const CnStampScope stamp_scope(s.stamp);
    const int lane = threadIdx.x & 63;
    if constexpr (W > 1) {
        if (threadIdx.x >= 64) { coop_helper_loop<W>(lane, __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))); return; }
    }
    const int e = s.post_list[blockIdx.x];
#ifdef CN_POST_DEBUG
    const long long dbg_start = wall_clock64();
    if (lane < 8) g_dbg_blk[lane] = 0;
#endif
    Rng R{MT_N, false};
    Robot rb;
    Lane h;
    load_env(s, e, lane, rb, h);
    double shared_nd = s.shared_nd[e];
    const int n = crowd_size(s, e);
    post_obs_updates<W>(s, R, e, lane, n, s.step_counter[e], rb, h, shared_nd);
#ifdef CN_POST_DEBUG
    if (lane == 0) g_dbg_blk[0] = wall_clock64() - dbg_start;
    if (lane < 8) g_post_dbg[blockIdx.x * 8 + lane] = g_dbg_blk[lane];
#endif
    store_env(s, e, lane, rb, h);
    if (lane == 0) s.shared_nd[e] = shared_nd;
    rng_store(R, s, e, lane);
    if constexpr (W > 1) { // release the helpers
        if (lane == 0) coop_lds<W>().cmd = 2;
        __syncthreads();
    }
}

// Second half of a step when the observation needs the 'truth' roll-outs of the state just reached (sim.predict_method = 'truth'):
// observation (reset or step form), then the post-observation updates of the envs that were not reset.
// only_pending (cn_env_set_scene): the envs that were not just given a new start are left alone, observation rows included.
__global__ __launch_bounds__(64) void env_obs_kernel(EnvDev s, cn_obs ob, int only_pending)
{
    const int lane = threadIdx.x;
    const int e = blockIdx.x;
    if (only_pending && !s.pend[e]) return;
    Rng R{MT_N, false};
    Robot rb;
    Lane h;
    load_env(s, e, lane, rb, h);
    double shared_nd = s.shared_nd[e];
    const bool was_reset = s.pend[e] != 0;
    const int n = crowd_size(s, e);
    write_obs(s, e, lane, n, was_reset, rb, h, ob, was_reset ? 0 : s.step_counter[e]);
    if (!was_reset) post_obs_updates(s, R, e, lane, n, s.step_counter[e], rb, h, shared_nd);
    if (lane == 0) s.pend[e] = 0;
    store_env(s, e, lane, rb, h);
    if (lane == 0) s.shared_nd[e] = shared_nd;
    rng_store(R, s, e, lane);
}

// crowd_sim_var_num.py:366-460 step (+ crowd_sim_pred.py:216-233 social reward) and the vec-env auto-reset
// (rl/networks/shmem_vec_env.py:139-142).  ORCA velocities for this step were produced by the ORCA kernels (orca.h).
// SPLIT = true: first half only (everything up to the kinematics and the reset bookkeeping); env_obs_kernel finishes the step after
// the roll-out kernels.
// W = 4: three helper wavefronts per env for the long placement loops of dense crowds (see CoopLds); W = 1: one wavefront per env
// Memory: the kernel is the latency chain of its slowest wavefront, so its reads are issued in two batches instead of one dependent trip
// after the other.  The GATHER at the top issues every load whose address depends only on (e, lane) and whose value no store of this launch
// produces, with no store in front of it; what the kernel changes later (step / case counter, crowd size) is used from those registers and
// never read again.  The SECOND batch goes out as soon as the outcome of the step is known: the staged episode of an env that resets, the
// env's MT19937 state where the step will draw from it (rng_prefetch).
// DEFER = true (dense crowds without a lane kernel): the observation is written, the post-observation updates -- which nothing in the
// observation depends on -- are left to env_post_kernel on the side stream, in front of the ORCA pass that needs the new goals: the
// long placement loops of the few envs that change goals then run beside the policy forward instead of in front of it.
// PF: the config profile (env_profile.h).  Everything below reads the view `s`; ProfileTrain is instantiated for <false, 1, false> only.
template <bool SPLIT, int W = 1, bool DEFER = false, class PF = ProfileGeneric>
__global__ __launch_bounds__(64 * W, W > 1 ? 2 : 4) void env_step_kernel(EnvDev s_arg, const float *actions, cn_obs ob, float *reward_out,
                                                      uint8_t *done_out, uint8_t *info_out, double *ep_ret_out, int32_t *ep_len_out, float *not_done_out)
{
    typename EnvViewOf<PF>::type s(s_arg); // generic: a reference to the argument itself
    typedef typename std::decay<decltype(s)>::type View;
    const CnStampScope stamp_scope(s.stamp);
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x;
    if constexpr (W > 1) {
        if (threadIdx.x >= 64) { coop_helper_loop<W>(lane, __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))); return; }
    }
    const auto &c = s.cfg;
    const int H = s.H;
    // ---- gather (indices of the per-slot arrays are clamped to the H slots, not to the crowd size: that is one of the loads)
    const int lj = lane < H ? lane : 0;
    int n = crowd_size(s, e);  // humans present during this step's reward / kinematics
    Rng R{MT_N, false};
    Robot rb;
    Lane h;
    load_env(s, e, lane, rb, h);
    double shared_nd = s.shared_nd[e];
    int step_counter = s.step_counter[e];
    float ax = actions[2 * e], ay = actions[2 * e + 1];
    // this step's ORCA velocity of human `lane` (social-force humans compute theirs below and do not use these)
    const float hax = s.hact[(size_t)e * 2 * H + lj], hay = s.hact[(size_t)e * 2 * H + H + lj];
    double ep_ret_in = s.ep_ret[e];
    int ep_cnt_in = s.ep_cnt[e];
    int nx_ready_in = s.nx_ready[e];
    uint64_t case_counter = s.case_counter[e];
    double desired_v = 0.0, wheel_in[4] = {0.0, 0.0, 0.0, 0.0};
    if (c.kinematics == CN_KIN_UNICYCLE && c.robot_policy == CN_ROBOT_NETWORK) {
        desired_v = s.desired_v[e];
        if (s.wheel) {
#pragma unroll
            for (int k = 0; k < 4; ++k) wheel_in[k] = s.wheel[(size_t)e * 4 + k];
            rng_prefetch(R, s, e, lane); // smooth_action's dead band draws on every step
        }
    }
    int obs_cnt = 0, obs_max = -1;
    if (c.human_num_range > 0) { obs_cnt = s.obs_cnt[e]; obs_max = s.obs_max[e]; }
    int rob_sim_valid = 0, rob_sim_n = 0;
    float rob_nd = 0.0f, rob_seen = 0.0f;
    if (c.robot_policy == CN_ROBOT_ORCA) {
        rob_sim_valid = s.rob_sim_valid[e];
        if (s.rob_sim_n) rob_sim_n = s.rob_sim_n[e];
        rob_nd = s.rob_nd[e];
        rob_seen = s.rob_seen[(size_t)e * H + lj];
    }
    int seen_before = 0; // human_visibility of the last observation
    if (c.phase == CN_PHASE_TEST) seen_before = s.vis[(size_t)e * H + lj];
    // the one wait of the gather (the wave-uniform words would otherwise each be waited for where they are loaded: see held())
    n = held_uniform(n); step_counter = held_uniform(step_counter); shared_nd = held_uniform(shared_nd); ax = held_uniform(ax); ay = held_uniform(ay);
    ep_ret_in = held_uniform(ep_ret_in); ep_cnt_in = held_uniform(ep_cnt_in); case_counter = held_uniform(case_counter);
    const bool nx_ready = held_uniform(nx_ready_in) != 0;
    const bool isH = lane < n;
    if (e == 0 && lane == 0) *s.lp3_cnt = 0; // the ORCA pass that follows starts with an empty linearProgram3 list

    // srnn.clip_action (crowd_nav/policy/srnn.py:17-34), float32 like the numpy action array
    double uni_v = 0.0, uni_r = 0.0; // ActionRot(v, r) of the unicycle robot
    double axd = 0.0, ayd = 0.0;     // float64 action of the social-force robot
    if (c.robot_policy == CN_ROBOT_SOCIAL_FORCE) {
        // SOCIAL_FORCE.predict (crowd_nav/policy/social_force.py:11-52) on the robot's beliefs, all in float64; lane j evaluates the
        // push of human j, the sum runs in list order
        const double dxg = rb.gx - rb.px, dyg = rb.gy - rb.py;
        const double dist_to_goal = sqrt(dxg * dxg + dyg * dyg);
        const double desired_vx = (dxg / dist_to_goal) * c.robot_v_pref, desired_vy = (dyg / dist_to_goal) * c.robot_v_pref;
        const double curr_dvx = c.sf_KI * (desired_vx - rb.vx), curr_dvy = c.sf_KI * (desired_vy - rb.vy);
        const double dx = rb.px - h.l0, dy = rb.py - h.l1;
        const double d = sqrt(dx * dx + dy * dy);
        const double f = c.sf_A * det_exp((c.robot_radius + h.l4 - d) / c.sf_B);
        const double fx = f * (dx / d), fy = f * (dy / d);
        double ivx = 0.0, ivy = 0.0;
        for (int j = 0; j < n; ++j) { ivx += __shfl(fx, j, 64); ivy += __shfl(fy, j, 64); }
        const double nvx = rb.vx + (curr_dvx + ivx) * c.time_step, nvy = rb.vy + (curr_dvy + ivy) * c.time_step;
        const double act_norm = sqrt(nvx * nvx + nvy * nvy);
        if (act_norm > c.robot_v_pref) { axd = nvx / act_norm * c.robot_v_pref; ayd = nvy / act_norm * c.robot_v_pref; }
        else { axd = nvx; ayd = nvy; }
    } else if (c.robot_policy == CN_ROBOT_ORCA) {
        // crowd_sim_var_num.py:371-375: action = robot.act(copy of last_human_states) -> ORCA.predict (orca.py:64-117) on the
        // robot's BELIEFS about all H humans (never-seen ones sit at the (15,15) dummy); no clip_action on this path
        float nd, seen_r;
        if (!held(rob_sim_valid) || (s.rob_sim_n && held(rob_sim_n) != n + 1)) { // orca.py:80-82: new simulator when the crowd size changed
            nd = (float)shared_nd;
            seen_r = (float)(h.l4 + 0.01 + c.orca_safety_space);
            if (isH) s.rob_seen[(size_t)e * H + lane] = seen_r;
            if (lane == 0) { s.rob_nd[e] = nd; s.rob_sim_valid[e] = 1; if (s.rob_sim_n) s.rob_sim_n[e] = (uint8_t)(n + 1); }
        } else {
            nd = held(rob_nd);
            rob_seen = held(rob_seen);
            seen_r = isH ? rob_seen : __shfl(rob_seen, 0, 64); // (lanes past the crowd carry slot 0's value, as they always did)
        }
        double gvx = rb.gx - rb.px, gvy = rb.gy - rb.py;
        const double speed = sqrt(gvx * gvx + gvy * gvy);
        if (speed > 1.0) { gvx = gvx / speed; gvy = gvy / speed; }
        orca_wave(lane, n, isH, (float)h.l0, (float)h.l1, (float)h.l2, (float)h.l3, seen_r, (float)rb.px, (float)rb.py, (float)rb.vx, (float)rb.vy,
                  (float)(c.robot_radius + 0.01 + c.orca_safety_space), (float)c.robot_v_pref, (float)gvx, (float)gvy, nd, n,
                  (float)c.orca_time_horizon, (float)c.time_step, ax, ay);
    } else if (c.kinematics == CN_KIN_UNICYCLE) {
        // srnn.py:36-43: (change of v, change of theta) clipped in float32; crowd_sim_var_num.py:379-381: the commanded speed is the
        // running sum self.desiredVelocity[0], clipped to +-v_pref (float64 from there on, as with the numpy the reference pins)
        const float dv = fminf(fmaxf(ax, (float)-0.1), (float)0.087);
        ay = fminf(fmaxf(ay, (float)-0.06), (float)0.06);
        uni_v = fmin(fmax(held(desired_v) + (double)dv, -c.robot_v_pref), c.robot_v_pref);
        uni_r = (double)ay;
        if (lane == 0) s.desired_v[e] = uni_v;
        if (s.wheel) {
            // CrowdSimPred.step (crowd_sim_pred.py:120-131) sends the command through smooth_action (crowd_sim.py:315-358): wheel speeds of
            // a Turtlebot2i (wheel radius 0.035 m, track 0.23 m) clipped to +-17.5 rad/s, low-pass filtered in the test phase, then
            // reduced towards zero by a noisy dead band N(1.8, 0.15) per wheel.  Wave-uniform; these are the first draws of the step.
            double *wh = s.wheel + (size_t)e * 4;
            const double last_left = held(wheel_in[0]), last_right = held(wheel_in[1]);
            double gauss = held(wheel_in[2]);
            bool has_gauss = held(wheel_in[3]) != 0.0;
            rng_load(R, s, e, lane);
            const double w = uni_r / c.time_step;
            double left = (2.0 * uni_v - 0.23 * w) / (2.0 * 0.035), right = (2.0 * uni_v + 0.23 * w) / (2.0 * 0.035);
            left = fmin(fmax(left, -17.5), 17.5); right = fmin(fmax(right, -17.5), 17.5);
            if (c.phase == CN_PHASE_TEST) {
                left = (1. - 0.1) * last_left + 0.1 * left;
                right = (1. - 0.1) * last_right + 0.1 * right;
            }
            const double keep_left = left, keep_right = right;
            if (left > 0) left = fmax(0., left - rng_normal(R, lane, 1.8, 0.15, gauss, has_gauss));
            else left = fmin(0., left + rng_normal(R, lane, 1.8, 0.15, gauss, has_gauss));
            if (right > 0) right = fmax(0., right - rng_normal(R, lane, 1.8, 0.15, gauss, has_gauss));
            else right = fmin(0., right + rng_normal(R, lane, 1.8, 0.15, gauss, has_gauss));
            uni_v = 0.035 / 2 * (left + right);
            uni_r = 0.035 / 0.23 * (right - left) * c.time_step;
            if (lane == 0) { wh[0] = keep_left; wh[1] = keep_right; wh[2] = gauss; wh[3] = has_gauss ? 1.0 : 0.0; }
        }
    } else {
        const float act_norm = sqrtf(ax * ax + ay * ay);
        const float vp = (float)c.robot_v_pref;
        if (act_norm > vp) { ax = ax / act_norm * vp; ay = ay / act_norm * vp; }
    }
    // humans.policy = 'social_force' (SOCIAL_FORCE.predict for every human, float64): lane i is human i and walks the list of the
    // other agents get_human_actions passes -- every other human (true state unless coincident -> the dummy at (7,7) with the
    // config radius), then the robot when robot.visible
    double sfx = 0.0, sfy = 0.0;
    if (c.humans_policy == CN_HUMANS_SOCIAL_FORCE) {
        const double dxg = h.gx - h.px, dyg = h.gy - h.py;
        const double dist_to_goal = sqrt(dxg * dxg + dyg * dyg);
        const double desired_vx = (dxg / dist_to_goal) * h.vpref, desired_vy = (dyg / dist_to_goal) * h.vpref;
        const double curr_dvx = c.sf_KI * (desired_vx - h.vx), curr_dvy = c.sf_KI * (desired_vy - h.vy);
        double ivx = 0.0, ivy = 0.0;
        for (int j = 0; j <= n; ++j) {
            if (j == n && !c.robot_visible) break;
            const int src = j < n ? j : 0; // the shuffles stay outside any conditional (they read inactive lanes as 0 otherwise)
            const double jx = __shfl(h.px, src, 64), jy = __shfl(h.py, src, 64), jr = __shfl(h.rad, src, 64);
            double ox = j < n ? jx : rb.px, oy = j < n ? jy : rb.py, orad = j < n ? jr : c.robot_radius;
            const bool hidden = c.human_fov < 2.0 ? !in_fov(c, c.human_fov, h.px, h.py, h.vx, h.vy, 0.0, ox, oy) : (ox == h.px && oy == h.py);
            if (hidden) { ox = 7.0; oy = 7.0; if (j < n) orad = c.human_radius; }
            const double dx = h.px - ox, dy = h.py - oy;
            const double d = sqrt(dx * dx + dy * dy);
            const double f = c.sf_A * det_exp((h.rad + orad - d) / c.sf_B);
            if (j != lane) { ivx += f * (dx / d); ivy += f * (dy / d); }
        }
        const double nvx = h.vx + (curr_dvx + ivx) * c.time_step, nvy = h.vy + (curr_dvy + ivy) * c.time_step;
        const double act_norm = sqrt(nvx * nvx + nvy * nvy);
        if (act_norm > h.vpref) { sfx = nvx / act_norm * h.vpref; sfy = nvy / act_norm * h.vpref; }
        else { sfx = nvx; sfy = nvy; }
    }
    // calc_reward (crowd_sim_var_num.py:465-561), pre-move positions.  "first collision in list order, break":
    // dmin is only consumed when there is no collision at all, so the lane-parallel min is equivalent.
    const double cdx = h.px - rb.px, cdy = h.py - rb.py;
    const double closest = isH ? sqrt(cdx * cdx + cdy * cdy) - h.rad - c.robot_radius : INFINITY;
    const bool collision = wv_any(closest < 0.0);
    double dmin;
    if constexpr (view_pinned<View>) dmin = wv_min_dpp(closest);
    else dmin = wv_min(closest);
    const double goal_dist = norm2(rb.px - rb.gx, rb.py - rb.gy);
    const bool reaching_goal = goal_dist < (c.kinematics == CN_KIN_UNICYCLE ? 0.6 : c.robot_radius); // :487-492
    const double global_time = (double)step_counter * c.time_step;
    double reward;
    int done, info;
    // Danger condition: the discomfort circle (train, :496-498) or, in the test phase, an intrusion into the humans' TRUE
    // future positions k = 1..P (:499-511; humans the robot did not see in its last observation are blanked to (15,15))
    const bool test_phase = c.phase == CN_PHASE_TEST;
    bool danger_cond = dmin < c.discomfort_dist;
    double min_danger = 0.0, rf_truth = 0.0;
    if (test_phase) {
        const double *tre = s.tr + (size_t)e * (s.R + 1) * 4 * H;
        const bool seen = isH && held(seen_before) != 0;
        double best = INFINITY;
        for (int k = 1; k <= s.P; ++k) {
            if (isH) {
                const double fx = (seen ? tre[(k * s.I * 4 + 0) * H + lane] : 15.0) - rb.px, fy = (seen ? tre[(k * s.I * 4 + 1) * H + lane] : 15.0) - rb.py;
                const double d = sqrt(fx * fx + fy * fy);
                if (d < c.robot_radius + c.human_radius) {
                    best = fmin(best, d);
                    const double pen = c.collision_penalty / (double)(1 << (k + 1));
                    if (pen < rf_truth) rf_truth = pen;
                }
            }
        }
        best = wv_min(best);
        danger_cond = best < INFINITY;
        min_danger = danger_cond ? best : 0.0;
    } else if (c.phase == CN_PHASE_VAL) {
        // phase 'val' (CrowdSimPred-v0): the same test on what the previous observation left in self.human_future_traj -- its const_vel /
        // truth predictions, unseen humans already blanked (ftraj)
        const double *ft = s.ftraj + (size_t)e * s.P * 2 * H;
        double best = INFINITY;
        for (int k = 1; k <= s.P; ++k)
            if (isH) {
                const double fx = ft[((k - 1) * 2 + 0) * H + lane] - rb.px, fy = ft[((k - 1) * 2 + 1) * H + lane] - rb.py;
                const double d = sqrt(fx * fx + fy * fy);
                if (d < c.robot_radius + c.human_radius) best = fmin(best, d);
            }
        best = wv_min(best);
        danger_cond = best < INFINITY;
        min_danger = danger_cond ? best : 0.0;
    }
    if (c.env_kind == CN_ENV_COLLECT) {
        // crowd_sim_var_num_collect.py:139-188: the data-collection env never ends an episode (global_time >= 40000 aside) and pays no
        // reward; a robot that reaches its goal gets a new one -- the median of the humans' positions or a uniform point of the
        // arena, each with probability 1/2 (np.random draws in this order: uniform(0, 1), then uniform(-a, a, size = 2))
        reward = 0.0; done = 0; info = CN_INFO_NOTHING;
        if (global_time >= 40000.0) { done = 1; info = CN_INFO_TIMEOUT; }
        else if (collision) info = CN_INFO_COLLISION;
        else if (goal_dist < c.robot_radius) {
            info = CN_INFO_REACHGOAL;
            rng_load(R, s, e, lane);
            if (rng_uniform(R, lane, 0.0, 1.0) < 0.5) {
                // np.median(axis = 0): the middle element of the sorted column, or the mean of the two middle ones (lane-parallel rank)
                double med[2];
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    const double v = isH ? (d == 0 ? h.px : h.py) : INFINITY;
                    int rank = 0;
                    for (int m = 0; m < n; ++m) {
                        const double vm = __shfl(v, m, 64);
                        rank += (vm < v || (vm == v && m < lane)) ? 1 : 0;
                    }
                    const uint64_t hi_m = __ballot(isH && rank == n / 2), lo_m = __ballot(isH && rank == (n - 1) / 2);
                    const double vhi = __shfl(v, __ffsll((unsigned long long)hi_m) - 1, 64), vlo = __shfl(v, __ffsll((unsigned long long)lo_m) - 1, 64);
                    med[d] = (n & 1) ? vhi : (vlo + vhi) / 2.0;
                }
                rb.gx = med[0]; rb.gy = med[1];
            } else {
                rb.gx = rng_uniform(R, lane, -c.arena_size, c.arena_size);
                rb.gy = rng_uniform(R, lane, -c.arena_size, c.arena_size);
            }
        }
    }
    else if (global_time >= c.time_limit - 1.0) { reward = 0.0; done = 1; info = CN_INFO_TIMEOUT; }
    else if (collision) { reward = c.collision_penalty; done = 1; info = CN_INFO_COLLISION; }
    else if (reaching_goal) { reward = c.success_reward; done = 1; info = CN_INFO_REACHGOAL; }
    else if (danger_cond) {
        reward = (dmin - c.discomfort_dist) * c.discomfort_penalty_factor * c.time_step;
        done = 0; info = CN_INFO_DANGER;
    } else {
        reward = (c.kinematics == CN_KIN_UNICYCLE ? 3.0 : 2.0) * (-fabs(goal_dist) - rb.pot); // :536-542 pot_factor
        rb.pot = -fabs(goal_dist);
        done = 0; info = CN_INFO_NOTHING;
    }
    if (s.min_dist && lane == 0) s.min_dist[e] = info == CN_INFO_DANGER ? min_danger : 0.0; // Danger(min_dist)
    if (c.env_kind == CN_ENV_PRED && test_phase) {
        // test phase: self.human_future_traj was just overwritten by the 'truth' roll-out, so the social reward sees it too
        reward = reward + wv_min(rf_truth);
    } else if (c.env_kind == CN_ENV_PRED) {
        // social reward from the predictions stored by the previous observation (crowd_sim_pred.py:216-233)
        const double *ft = s.ftraj + (size_t)e * s.P * 2 * H;
        double rf = 0.0;
        for (int k = 1; k <= s.P; ++k) {
            const double pen = c.collision_penalty / (double)(1 << (k + 1));
            if (isH) {
                const double fx = ft[((k - 1) * 2 + 0) * H + lane] - rb.px, fy = ft[((k - 1) * 2 + 1) * H + lane] - rb.py;
                if (sqrt(fx * fx + fy * fy) < c.robot_radius + c.human_radius && pen < rf) rf = pen;
            }
        }
        reward = reward + wv_min(rf);
    }
    if (c.kinematics == CN_KIN_UNICYCLE) {
        // :548-559 rotation penalty and reversing penalty, added to every outcome
        const double r_spin = -4.5 * (uni_r * uni_r);
        const double r_back = uni_v < 0.0 ? -2.0 * fabs(uni_v) : 0.0;
        reward = reward + r_spin + r_back;
        // differential drive, agent.py:148-165.  A rotation below 1e-4 sets R = 0, i.e. the robot does not translate on that step
        // (the reference's formula, restated as it is)
        double Rr = 0.0;
        if (!(fabs(uni_r) < 0.0001)) { const double w = uni_r / c.time_step; Rr = uni_v / w; }
        double s0, c0, s1, c1;
        det_sincos(rb.theta, s0, c0);
        det_sincos(rb.theta + uni_r, s1, c1);
        rb.px = rb.px - Rr * s0 + Rr * s1;
        rb.py = rb.py + Rr * c0 - Rr * c1;
        double th = fmod(rb.theta + uni_r, 2.0 * M_PI); // Python %: the result takes the divisor's sign
        if (th != 0.0 && th < 0.0) th += 2.0 * M_PI;
        rb.theta = th;
        det_sincos(th, s0, c0);
        rb.vx = uni_v * c0; rb.vy = uni_v * s0;
    } else if (c.robot_policy == CN_ROBOT_SOCIAL_FORCE) {
        rb.px = rb.px + axd * c.time_step; rb.py = rb.py + ayd * c.time_step;
        rb.vx = axd; rb.vy = ayd;
    } else {
        // kinematics (crowd_sim/envs/utils/agent.py:170-183, holonomic)
        rb.px = rb.px + (double)(ax * (float)c.time_step);
        rb.py = rb.py + (double)(ay * (float)c.time_step);
        rb.vx = (double)ax; rb.vy = (double)ay;
    }
    if (isH && c.humans_policy == CN_HUMANS_SOCIAL_FORCE) {
        h.px = h.px + sfx * c.time_step;
        h.py = h.py + sfy * c.time_step;
        h.vx = sfx; h.vy = sfy;
        s.hact[(size_t)e * 2 * H + lane] = (float)sfx; s.hact[(size_t)e * 2 * H + H + lane] = (float)sfy; // for cn_env_get_human_actions
    } else if (isH) {
        h.px = h.px + (double)hax * c.time_step;
        h.py = h.py + (double)hay * c.time_step;
        h.vx = (double)hax; h.vy = (double)hay;
    }
    step_counter += 1;
    const double ep_ret = ep_ret_in + reward;
    const int ep_cnt = ep_cnt_in + 1;
    const bool resetting = done && c.auto_reset;
    const int period = (int)(5.0 / c.time_step + 0.5);
    if (lane == 0) {
        reward_out[e] = (float)reward; done_out[e] = (uint8_t)done; info_out[e] = (uint8_t)info;
        ep_ret_out[e] = ep_ret; ep_len_out[e] = ep_cnt;
        if (not_done_out) not_done_out[e] = done ? 0.0f : 1.0f; // the `masks` tensor of train.py:185-186
    }
    // ---- second batch: the outcome is known, and with it what the slow paths of this env will read
    if (resetting) {
        // vec-env auto-reset: the terminal observation is replaced by the first observation of the next episode.
        // (The terminal step's own crowd-size / goal-change / respawn draws happen before np.random.seed and cannot be observed.)
        do_reset(s, R, e, lane, nx_ready, case_counter, rb, h, shared_nd, n, ob, !SPLIT);
        if (SPLIT && lane == 0) s.pend[e] = 1;
    } else {
        // (auto_reset == 0, the single-env gym object: a terminal step is an ordinary step -- terminal observation, goal
        // changes and respawns included, crowd_sim_var_num.py:430-458 -- and the caller resets explicitly)
        // the draws of an ordinary step: the crowd-size change and the goal changes every 5 s, and a human at its goal (the periodic updates
        // may move goals, so on those steps the stream is fetched whatever the ballot says; on all others the ballot is the one
        // post_obs_updates takes, on the same values).  The stream arrives while the observation is written.
        bool draws = (c.human_num_range > 0 || (!SPLIT && !DEFER && c.random_goal_changing)) && (step_counter % period) == 0;
        if (!SPLIT && !DEFER && c.end_goal_changing) draws = draws || __ballot(isH && norm2(h.gx - h.px, h.gy - h.py) < h.rad) != 0;
        if (draws) rng_prefetch(R, s, e, lane);
        if (c.human_num_range > 0 && (step_counter % period) == 0) {
            // crowd_sim_var_num.py:404-437 / crowd_sim_pred.py:165-190: every 5 s humans leave from the END of the list (only ones the
            // robot was not looking at) or new ones are appended, before the observation is generated
            rng_load(R, s, e, lane);
            if (rng_double(R, lane) < 0.5) {
                const int oc = held(obs_cnt), om = held(obs_max);
                int max_remove;
                if (c.env_kind == CN_ENV_VARNUM) {
                    max_remove = n - (c.human_num - c.human_num_range);
                    if (oc > 0 && (n - 1) - om < max_remove) max_remove = (n - 1) - om;
                } else {
                    max_remove = oc == 0 ? n - 1 : (n - 1) - om;
                    if (c.human_num_range < max_remove) max_remove = c.human_num_range;
                }
                n -= rng_randint(R, lane, 0, max_remove + 1);
            } else {
                const int add_num = rng_randint(R, lane, 0, c.human_num_range + 1);
                const int first = n;
                for (int i = first; i < first + add_num && i < H; ++i) {
                    gen_human(s, R, lane, i, i, rb, h, shared_nd);
                    if (lane == i) { h.l0 = 15.0; h.l1 = 15.0; h.l2 = 0.0; h.l3 = 0.0; h.l4 = 0.3; }
                    n = i + 1;
                }
            }
        }
        if (!SPLIT) {
            write_obs(s, e, lane, n, false, rb, h, ob, step_counter);
            if constexpr (DEFER) {
                // (a superset of the envs post_obs_updates does anything for: it evaluates `reached` after the periodic goal changes)
                bool need = c.random_goal_changing && (step_counter % period) == 0;
                if (c.end_goal_changing) need = need || __ballot(lane < n && norm2(h.gx - h.px, h.gy - h.py) < h.rad) != 0;
                if (need && lane == 0) s.post_list[atomicAdd(s.post_cnt, 1)] = e;
            } else {
                post_obs_updates<W>(s, R, e, lane, n, step_counter, rb, h, shared_nd);
            }
        }
        if (lane == 0) { s.step_counter[e] = step_counter; s.ep_ret[e] = ep_ret; s.ep_cnt[e] = ep_cnt; }
    }
    store_env(s, e, lane, rb, h);
    if (lane == 0 && s.nh) s.nh[e] = n;
    if (lane == 0) s.shared_nd[e] = shared_nd;
    rng_store(R, s, e, lane);
    if constexpr (W > 1) { // release the helpers
        if (lane == 0) coop_lds<W>().cmd = 2;
        __syncthreads();
    }
}

__global__ void export_state_kernel(EnvDev s, double *humans, double *robot)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int H = s.H;
    if (humans && idx < s.E * H * 8) {
        const int e = idx / (H * 8), r = idx % (H * 8), j = r / 8, f = r % 8;
        humans[idx] = s.hum[((size_t)e * 8 + f) * H + j];
    }
    if (robot && idx < s.E * 8) robot[idx] = s.rob[idx];
}
__global__ void export_hact_kernel(EnvDev s, float *out)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int H = s.H;
    if (idx < s.E * H * 2) {
        const int e = idx / (H * 2), r = idx % (H * 2), j = r / 2, f = r % 2;
        out[idx] = s.hact[((size_t)e * 2 + f) * H + j];
    }
}

// the robot-side detect_visible decision on the CURRENT state (robot_sees, the function write_obs decides with), one thread per slot
__global__ void export_visibility_kernel(EnvDev s, uint8_t *out)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int H = s.H;
    if (idx >= s.E * H) return;
    const int e = idx / H, j = idx % H;
    const int n = s.nh ? s.nh[e] : H;
    bool vis = false;
    if (j < n) {
        const double *r = s.rob + (size_t)e * 8;
        const Robot rb = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
        const double *h = s.hum + (size_t)e * 8 * H + j;
        vis = robot_sees(s.cfg, rb, true, h[0], h[(size_t)H], h[(size_t)6 * H]);
    }
    out[idx] = vis ? 1 : 0;
}

// cn_env_trace_append: one thread per (env, agent slot) writes record index[e] of env e from the CURRENT state -- what export_state_kernel,
// cn_env_get_human_counts and export_visibility_kernel report, rounded once to float32 -- for the envs `active` / `index` select.  A kernel of
// its own: nothing of it is compiled into the step kernels.
__global__ void trace_append_kernel(EnvDev s, const int64_t *active, const int64_t *index, int cap, float *agents, uint8_t *flags, float *goal,
                                    int32_t *length)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int H = s.H, A = H + 1;
    if (idx >= s.E * A) return;
    const int e = idx / A, a = idx % A;
    if (active && active[e] == 0) return;
    const int64_t t = index[e];
    if (t < 0 || t >= (int64_t)cap) return;
    const size_t slot = ((size_t)e * cap + (size_t)t) * A + a;
    const double *r = s.rob + (size_t)e * 8;
    float v[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    uint8_t fl = 0;
    if (a == 0) {
        v[0] = (float)r[R_PX]; v[1] = (float)r[R_PY]; v[2] = (float)r[R_VX]; v[3] = (float)r[R_VY];
        v[4] = (float)s.cfg.robot_radius; v[5] = (float)r[R_THETA];
        fl = 1;
        length[e] = (int32_t)t + 1;
        if (t == 0 && goal) { goal[(size_t)e * 2] = (float)r[R_GX]; goal[(size_t)e * 2 + 1] = (float)r[R_GY]; }
    } else if (a - 1 < crowd_size(s, e)) {
        const int j = a - 1;
        const double *h = s.hum + (size_t)e * 8 * H + j;
        const Robot rb = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
        const double px = h[(size_t)F_PX * H], py = h[(size_t)F_PY * H], rad = h[(size_t)F_RAD * H];
        v[0] = (float)px; v[1] = (float)py; v[2] = (float)h[(size_t)F_VX * H]; v[3] = (float)h[(size_t)F_VY * H];
        v[4] = (float)rad; v[5] = (float)h[(size_t)F_VPREF * H];
        fl = robot_sees(s.cfg, rb, true, px, py, rad) ? 3 : 1;
    }
    float2 *dst = reinterpret_cast<float2 *>(agents + slot * 6); // 24-byte records: 8-byte aligned
    dst[0] = make_float2(v[0], v[1]); dst[1] = make_float2(v[2], v[3]); dst[2] = make_float2(v[4], v[5]);
    flags[slot] = fl;
}

__global__ void fill_i32_kernel(int n, int v, int32_t *out)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) out[idx] = v;
}

} // namespace

struct cn_env_batch {
    EnvDev d;
    bool reset_done;
    void *blob;
    size_t blob_bytes; // the persistent state (what a snapshot holds); per-step scratch is carved behind it
    // ORCA of step t+1 only needs the simulator state left by step t, not the robot's next action: it is launched on a
    // side stream as soon as step t (or a reset) is enqueued and overlaps the caller's policy forward.
    hipStream_t side;
    hipEvent_t ev_state, ev_orca, ev_pre;
    bool orca_ready; // hact for the current state has been enqueued on `side`
    long long pregen_ticks; // time budget of one env_pregen_kernel launch (prefetch_orca)
    bool plan_ok;      // this configuration's step builds the row plan (lane kernel, crowds of <= 48: what the consumer takes)
    // the side-stream "tail" of a step (episode pre-generation + the infeasible third of the ORCA programs): launched by the step itself,
    // or -- cn_env_set_tail_deferral -- held back until the caller says that its big kernel is enqueued (cn_env_launch_tail)
    bool defer_tail, tail_pending;
    hipStream_t side2;   // deferred mode: the pre-generation runs beside the ORCA tail, not in front of it
    hipEvent_t ev_pg;
    bool pg_pending;     // ev_pg was recorded for work the next reader of the staging arrays has to wait for
    bool post_deferred;  // the step just enqueued left its post-observation updates to env_post_kernel (launch_tail runs it before ORCA)
    int lp3_blocks;      // grid of orca_lp3_kernel (lp3_grid, fixed at creation)
};

// calc_human_future_traj(method='truth'): P rolls of every human with its own policy
static int truth_rollout(cn_env_batch *env, hipStream_t st)
{
    if (env->d.cfg.humans_policy == CN_HUMANS_SOCIAL_FORCE) {
        hipLaunchKernelGGL(sf_truth_kernel, dim3(env->d.E), dim3(64), 0, st, env->d);
        CN_CHECK_LAUNCH();
        return CN_OK;
    }
    const int agents = env->d.E * env->d.H;
    for (int k = 1; k <= env->d.R; ++k) { // roll k needs all of roll k - 1 of the same env: one launch per roll (R = predict_steps * pred_interval)
        hipLaunchKernelGGL(orca_truth_kernel, dim3((agents + 3) / 4), dim3(256), 0, st, env->d, k);
        CN_CHECK_LAUNCH();
    }
    return CN_OK;
}

// sim.predict_method = 'truth': roll the humans forward P times from the state the first half of the step (or the reset) left, then
// write the observation and run the post-observation updates
static int truth_rollout_and_obs(cn_env_batch *env, const cn_obs *obs, hipStream_t st, bool only_pending = false)
{
    if (int rc = truth_rollout(env, st)) return rc;
    hipLaunchKernelGGL(env_obs_kernel, dim3(env->d.E), dim3(64), 0, st, env->d, *obs, only_pending ? 1 : 0);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

// The grid of orca_lp3_kernel.  The list length is only known on the device: a grid for a quarter of the agents (one per wavefront; the
// rest of the wavefronts exit at once, longer lists are walked with a stride) keeps enough wavefronts in flight to hide the latency of the
// cooperative routine.  CN_LP3_BLOCKS=n (read when a batch is created) takes n workgroups instead: with a small n every list is walked
// with a stride (tests/test_gpu_lp3_pairs.py).
static int lp3_grid(int agents)
{
    const char *v = getenv("CN_LP3_BLOCKS");
    const int n = v ? atoi(v) : 0;
    return n > 0 ? n : (agents + 15) / 16;
}

static bool lane_path_of(const cn_env_batch *env)
{
    const int slots = env->d.H + (env->d.cfg.robot_visible ? 1 : 0); // candidate neighbours per agent (self included)
    // (a narrowed human field of view goes through the cooperative kernel: the lane kernel has no visibility test in its inner loops)
    return env->d.cfg.humans_policy == CN_HUMANS_ORCA && slots <= 32 && env->d.cfg.human_fov >= 2.0;
}

// the batch belongs to the default training class: its step launch takes the instantiation compiled for ProfileTrain (env_profile.h);
// every other batch takes the generic one.  (orca_lane_kernel has no pinned instantiation: the profile removes three of its 49 argument
// loads and none of its 69 spilled scalars, and measured beside the generic one it was 0.2-0.8 us slower: profiles/HISTORY.md section 17)
static bool train_profile(const cn_env_batch *env) { return train_profile_of(env->d); }

// refill the next-episode staging of the envs that just consumed theirs (rare: ~1.5 % of envs per step; a 60 us chain of serial fp64
// work per such env).  It only depends on the step that just ran; nothing needs it before those envs finish their NEXT episode.
// Budget (ticks of 10 ns; cn_env_set_pregen_budget): see cn_env_set_pregen_budget in the header.
// dense crowds (the goals' exclusion zones cover the circle: BASELINE configs[4]) run their long placement loops on four wavefronts per env
static bool dense_crowd(cn_env_batch *env)
{
    const cn_env_config &cf = env->d.cfg;
    const double zone = 2.0 * (2.0 * (cf.randomize_attributes ? 0.5 : cf.human_radius) + cf.discomfort_dist) * env->d.H;
    static const int coop_env = getenv("CN_ENV_COOP") ? atoi(getenv("CN_ENV_COOP")) : -1; // 0 / 1 force (A/B), default: by density
    static const int coop_after = getenv("CN_COOP_AFTER") ? atoi(getenv("CN_COOP_AFTER")) : COOP_AFTER;
    env->d.coop_after = coop_after;
    return coop_env >= 0 ? coop_env != 0 : zone > 0.9 * 2.0 * M_PI * cf.circle_radius;
}

// Launch with an optional stop event.  An event handed to the launch completes with the kernel itself: it rides on the kernel's own
// dispatch packet, where hipEventRecord puts a marker packet behind the kernel and the stream's next kernel waits for that marker too
// (tools/event_gap_probe.hip, two 20 us kernels on one stream: nothing between them 0.9 us, a record between them 5.7 us, the first one's
// stop event instead 2.0-2.1 us; the waiting stream's kernel starts 8.4 us after the kernel's end instead of 12.5-12.9).
// The caller checks the launch with CN_CHECK_LAUNCH() as after hipLaunchKernelGGL.
template <typename... KArgs, typename... Args>
static void launch_ev(void (*kernel)(KArgs...), dim3 grid, dim3 blk, hipStream_t st, hipEvent_t stop, Args &&...args)
{
    if (stop) hipExtLaunchKernelGGL(kernel, grid, blk, 0, st, nullptr, stop, 0, static_cast<KArgs>(args)...);
    else hipLaunchKernelGGL(kernel, grid, blk, 0, st, static_cast<KArgs>(args)...);
}

// a stream that is being captured into a graph takes plain launches and event records (the nodes a capture knows), never a stop event
static bool capturing(hipStream_t st)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
}

static int launch_post(cn_env_batch *env, hipStream_t on)
{
    hipLaunchKernelGGL(env_post_kernel<4>, dim3(env->d.E), dim3(256), 0, on, stamped(env->d, CN_K_OTHER));
    CN_CHECK_LAUNCH();
#ifdef CN_POST_DEBUG
    {
        static int calls = 0;
        (void)hipStreamSynchronize(on);
        int cnt = 0;
        (void)hipMemcpy(&cnt, env->d.post_cnt, 4, hipMemcpyDeviceToHost);
        static long long host[8192 * 8];
        (void)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_post_dbg), sizeof(long long) * 8 * (size_t)cnt);
        int worst = 0;
        for (int i = 0; i < cnt; ++i) if (host[i * 8] > host[worst * 8]) worst = i;
        if (++calls % 4 == 0 && cnt > 0) {
            const long long *w = host + worst * 8;
            fprintf(stderr, "[post] envs %d | worst block: %.1f us (coop %.1f us, %lld coop placements, %lld rounds: producer busy %.1f us, helper 1 screening %.1f us; %lld placements, %lld serial passes)\n",
                    cnt, w[0] * 0.01, w[1] * 0.01, w[2], w[3], w[7] * 0.01, w[6] * 0.01, w[4], w[5]);
        }
    }
#endif
    return CN_OK;
}

static int launch_pregen(cn_env_batch *env, hipStream_t on)
{
    // (one wavefront per env also for dense crowds: a NEW episode's humans are placed in 4 candidates on average -- positions, with noise of up to
    // 2 m, against goals on the far side -- it is the goal changes mid-episode that run long)
    hipLaunchKernelGGL(env_pregen_kernel<1>, dim3(env->d.E), dim3(64), 0, on, stamped(env->d, CN_K_PREGEN), env->pregen_ticks);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

// The side-stream tail of the ORCA pass for the state the caller's stream has reached at this point: whatever the lane kernel could not
// finish (the infeasible programs -> linearProgram3), or the whole pass for configurations without a lane kernel; the 'truth' roll-outs of
// the test phase; and, in deferred mode, the episode pre-generation.  Ends with ev_orca, which the next step / reader waits for.
// state_bound: ev_state already is the stop event of the last launch on `main` (prefetch_orca's lane kernel, nothing enqueued since);
// otherwise it is recorded here, behind whatever `main` holds.
static int launch_tail(cn_env_batch *env, hipStream_t main, bool state_bound = false)
{
    const int agents = env->d.E * env->d.H;
    const bool lane_path = lane_path_of(env);
    if (!state_bound) CN_HIP(hipEventRecord(env->ev_state, main));
    CN_HIP(hipStreamWaitEvent(env->side, env->ev_state, 0));
    if (env->defer_tail && lane_path) {
        // beside the ORCA tail and the caller's robot-node kernel, on a stream of its own (behind the tail on ONE stream the two chains add
        // up to ~105 us and the next step waits for them: measured 0.36 ms per step instead of 0.28)
        CN_HIP(hipStreamWaitEvent(env->side2, env->ev_state, 0));
        if (int rc = launch_pregen(env, env->side2)) return rc;
        CN_HIP(hipEventRecord(env->ev_pg, env->side2));
        env->pg_pending = true;
    }
    if (env->post_deferred) { // the goal changes / respawns of the step just enqueued: the ORCA pass below reads the new goals
        if (int rc = launch_post(env, env->side)) return rc;
        env->post_deferred = false;
    }
    // ev_orca is the stop event of the ORCA launch where that is the side stream's last one (not while capturing; not in the test phase: the
    // roll-outs follow; not for social-force humans: no launch)
    const bool orca_bound = env->d.cfg.humans_policy == CN_HUMANS_ORCA && env->d.cfg.phase != CN_PHASE_TEST && !capturing(main);
    const hipEvent_t ev_last = orca_bound ? env->ev_orca : nullptr;
    if (env->d.cfg.humans_policy == CN_HUMANS_ORCA) { // social-force humans act inside env_step_kernel (one lane per human, no solver)
        if (lane_path) {
            // the infeasible programs are finished by the cooperative routine on the side stream, next to the policy forward (grid: lp3_grid)
            launch_ev(orca_lp3_kernel, dim3(env->lp3_blocks), dim3(256), env->side, ev_last, stamped(env->d, CN_K_ORCA_LP3));
            CN_CHECK_LAUNCH();
        } else {
            launch_ev(orca_kernel, dim3((agents + 3) / 4), dim3(256), env->side, ev_last, stamped(env->d, CN_K_ORCA_LP3));
            CN_CHECK_LAUNCH();
        }
    }
    if (env->d.cfg.phase == CN_PHASE_TEST) // 'truth' roll-out for the next step's Danger decision
        if (int rc = truth_rollout(env, env->side)) return rc;
    if (!orca_bound) CN_HIP(hipEventRecord(env->ev_orca, env->side));
    env->orca_ready = true;
    env->tail_pending = false;
    return CN_OK;
}

// everything the library has in flight (or holds back) for the current state is ordered before what `st` gets next
static int sync_side(cn_env_batch *env, hipStream_t st)
{
    if (env->tail_pending) { if (int rc = launch_tail(env, st)) return rc; }
    if (env->orca_ready) CN_HIP(hipStreamWaitEvent(st, env->ev_orca, 0));
    if (env->pg_pending) { CN_HIP(hipStreamWaitEvent(st, env->ev_pg, 0)); env->pg_pending = false; }
    return CN_OK;
}

// pre_bound: ev_pre already is the stop event of the last launch on `main` (cn_env_step's step kernel); otherwise it is recorded here
static int prefetch_orca(cn_env_batch *env, hipStream_t main, const cn_obs *obs, bool pre_bound = false)
{
    const float *plan_det = obs ? obs->detected_human_num : nullptr;
    int32_t *row_plan = obs ? obs->row_plan : nullptr;
    const int agents = env->d.E * env->d.H;
    const int slots = env->d.H + (env->d.cfg.robot_visible ? 1 : 0);
    const bool lane_path = lane_path_of(env);
    const bool defer = env->defer_tail && lane_path;
    if (!defer) {
        // With ev_pre / ev_state bound to the launches (the front of hh_fused 6.7 us shorter, this kernel's start 3.7 us earlier), medians of
        // three 200-step runs per budget in one call: 44 us 0.2535, 40 us 0.2519, 38 us 0.2522, 36 us 0.2545, 34 us 0.2592, 32 us 0.2617 ms per
        // step; env_step on its own clock does not move: the budget stays at 40 us (profiles/HISTORY.md section 18).
        // Round 5: 40 us.  With the placement loops 64 candidates at a time an episode is generated in ~30 us, and the lane kernel in front of
        // the policy got shorter (42 us): same box, 200 steps each -- 55 us 0.2866 / 0.2860 ms per step (human-human kernel 153 us on its own
        // clock: a quarter of its workgroups wait for this kernel's CUs), 45 us 0.2825, 40 us 0.2799 (139 us), 35 us 0.2903, 30 us 0.3001 (the
        // ORCA tail then reaches the CUs early); env_step stays at 25 us down to 30 us: no env runs out of staged episodes any more.
        // Rounds 3-4 (notes kept):
        // beside the lane kernel, before the policy kernels take the whole LDS of every CU.  Budget: the lane kernel below takes ~50 us at
        // 4096 envs x 20 humans and the policy comes right behind it.  55 us cuts the long tail of the rejection sampling (up to 150 us)
        // and still lets the usual 60-odd new episodes of a step finish in one go.  Measured inside one box, human-human kernel of the
        // policy: unbounded 0.138-0.139 ms, 65 us 0.139, 55 us 0.133, 45 us 0.135, 30 us 0.161 -- shorter is NOT better in this mode: the
        // ORCA tail kernel is queued behind this one, and when it starts before the policy's kernel has its workgroups on the CUs, that
        // kernel waits for them (the deferred mode removes exactly this coupling)
        if (!pre_bound) CN_HIP(hipEventRecord(env->ev_pre, main));
        if (env->post_deferred) {
            // the side stream starts with the deferred goal changes, which the ORCA pass and with it the next step wait for: the
            // pre-generation (whose workgroups mostly wait for the CUs the policy's kernel holds) goes beside them
            CN_HIP(hipStreamWaitEvent(env->side2, env->ev_pre, 0));
            if (int rc = launch_pregen(env, env->side2)) return rc;
            CN_HIP(hipEventRecord(env->ev_pg, env->side2));
            env->pg_pending = true;
        } else {
            CN_HIP(hipStreamWaitEvent(env->side, env->ev_pre, 0));
            if (int rc = launch_pregen(env, env->side)) return rc;
        }
    }
    bool state_bound = false;
    if (lane_path) {
        // one lane per agent, on the CALLER's stream: the policy forward the caller enqueues next starts behind this kernel, not
        // beside it (see orca_lane_kernel), and a same-stream hand-over costs 1-2 us where an event across streams costs 8-13
        // (tools/event_gap_probe.hip; in the step 15 us from env_step's end to the pre-generation's start)
        int32_t *plan = (plan_det && env->plan_ok && ((uintptr_t)plan_det & 15u) == 0) ? row_plan : nullptr;
        if (plan) row_plan = nullptr; // built below
        const int pg = plan ? rp_groups(env->d.E) : 0;
        const dim3 grid((agents + 63) / 64 + pg), blk(64);
        const EnvDev dl = stamped(env->d, CN_K_ORCA_LANE);
        unsigned long long *pst = cn_stamp_slot(CN_K_ROW_PLAN);
        // the tail below is released by this launch's own stop event when it is the last thing on `main` in front of launch_tail: no
        // memset of an unfilled plan behind it, the tail not held back, no capture
        state_bound = !row_plan && !defer && !capturing(main);
        auto lane = slots <= 8 ? orca_lane_kernel<8, 8> : slots <= 20 ? orca_lane_kernel<20, 32> : orca_lane_kernel<32, 32>;
        launch_ev(lane, grid, blk, main, state_bound ? env->ev_state : nullptr, dl, plan_det, plan, pg, pst);
        CN_CHECK_LAUNCH();
    }
    // a caller's plan buffer that this step does not fill must not keep the previous observation's plan
    if (row_plan) CN_HIP(hipMemsetAsync(row_plan, 0, 4, main));
    if (defer) { env->tail_pending = true; env->orca_ready = false; return CN_OK; } // cn_env_launch_tail, or the next call into this batch
    return launch_tail(env, main, state_bound);
}

extern "C" void cn_env_config_default(cn_env_config *c)
{
    // crowd_nav/configs/config.py:16-120 with the non-randomised training preset (BASELINE configs[1])
    *c = cn_env_config{};
    c->human_num = 20; c->predict_steps = 5; c->env_kind = CN_ENV_VARNUM;
    c->randomize_attributes = 0; c->random_goal_changing = 0; c->end_goal_changing = 1; c->sort_humans = 1;
    c->phase = CN_PHASE_TRAIN; c->nenv = 1; c->val_size = 100; c->test_size = 500; c->auto_reset = 1;
    c->time_step = 0.25; c->time_limit = 50.0;
    c->success_reward = 10.0; c->collision_penalty = -20.0; c->discomfort_dist = 0.25; c->discomfort_penalty_factor = 10.0;
    c->circle_radius = 6.0 * std::sqrt(2.0); c->arena_size = 6.0;
    c->human_radius = 0.3; c->human_v_pref = 1.0; c->robot_radius = 0.3; c->robot_v_pref = 1.0; c->sensor_range = 5.0;
    c->robot_fov = 2.0; c->human_fov = 2.0;
    c->goal_change_chance = 0.5; c->end_goal_change_chance = 1.0;
    c->orca_neighbor_dist = 10.0; c->orca_safety_space = 0.15; c->orca_time_horizon = 5.0; c->orca_time_horizon_obst = 5.0;
    c->sf_A = 2.0; c->sf_B = 1.0; c->sf_KI = 1.0; // config.py:126-128
}

extern "C" int cn_env_obs_width(const cn_env_config *cfg)
{
    if (cfg->env_kind == CN_ENV_COLLECT) return 4; // pred_info: frame id, prediction id, px, py
    return cfg->env_kind == CN_ENV_VARNUM ? 2 : 2 * (cfg->predict_steps + 1);
}

extern "C" int cn_env_create(const cn_env_config *cfg, int num_envs, int64_t seed, int64_t first_env_index, cn_env_batch **out)
{
    if (int rc = cn_require_device()) return rc;
    CN_REQUIRE(cfg && out, "cn_env_create: null argument");
    CN_REQUIRE(num_envs > 0, "cn_env_create: num_envs must be positive");
    CN_REQUIRE(cfg->human_num_range >= 0 && cfg->human_num_range < cfg->human_num, "cn_env_create: human_num_range must be in [0, human_num)");
    const int HM = cfg->human_num + cfg->human_num_range; // observation rows / lanes per env
    CN_REQUIRE(cfg->human_num >= 1 && HM <= CN_MAX_HUMANS, "cn_env_create: human_num + human_num_range must be in [1,%d]", CN_MAX_HUMANS);
    CN_REQUIRE(cfg->kinematics == CN_KIN_HOLONOMIC || (cfg->kinematics == CN_KIN_UNICYCLE && cfg->env_kind != CN_ENV_COLLECT && cfg->robot_policy == CN_ROBOT_NETWORK),
               "cn_env_create: kinematics must be holonomic, or unicycle with a network-driven robot outside CrowdSimVarNumCollect-v0 (the ORCA / "
               "social-force robot policies return ActionXY: crowd_sim_var_num.py:78-91, :379-381)");
    CN_REQUIRE(cfg->humans_policy == CN_HUMANS_ORCA || cfg->humans_policy == CN_HUMANS_SOCIAL_FORCE, "cn_env_create: unknown humans_policy %d", cfg->humans_policy);
    CN_REQUIRE(cfg->robot_fov > 0.0 && cfg->human_fov > 0.0, "cn_env_create: robot_fov / human_fov are in units of pi and must be positive (2 = all round)");
    CN_REQUIRE(cfg->predict_steps >= 1 && cfg->predict_steps <= CN_MAX_PRED, "cn_env_create: predict_steps must be in [1,%d]", CN_MAX_PRED);
    CN_REQUIRE(cfg->pred_interval >= 0 && cfg->pred_interval <= 16, "cn_env_create: pred_interval must be in [0,16] (0 = 1)");
    CN_REQUIRE(cfg->env_kind >= CN_ENV_VARNUM && cfg->env_kind <= CN_ENV_COLLECT, "cn_env_create: unknown env_kind %d", cfg->env_kind);
    CN_REQUIRE(cfg->env_kind != CN_ENV_COLLECT || (cfg->human_num_range == 0 && cfg->kinematics == CN_KIN_HOLONOMIC && cfg->phase == CN_PHASE_TRAIN &&
                                                   cfg->robot_policy == CN_ROBOT_ORCA && !cfg->predict_truth),
               "cn_env_create: CrowdSimVarNumCollect-v0 runs with a fixed crowd size, a holonomic ORCA-driven robot and phase train "
               "(what collect_data.py sets up; the reference's pred_info needs human_num_range == 0)");
    CN_REQUIRE(cfg->phase == CN_PHASE_TRAIN || cfg->phase == CN_PHASE_TEST || (cfg->phase == CN_PHASE_VAL && cfg->env_kind == CN_ENV_PRED),
               "cn_env_create: phase must be train or test, or val with CrowdSimPred-v0 (the other env classes fail in phase 'val': "
               "crowd_sim_var_num.py:501 reads self.human_future_traj, which they only assign in the test phase)");
    CN_REQUIRE(cfg->nenv >= 1, "cn_env_create: nenv (total env count) must be >= 1");
    CN_REQUIRE(cfg->robot_policy >= CN_ROBOT_NETWORK && cfg->robot_policy <= CN_ROBOT_SOCIAL_FORCE, "cn_env_create: unknown robot_policy %d", cfg->robot_policy);
    CN_REQUIRE(!cfg->robot_visible || HM <= CN_MAX_HUMANS - 1,
               "cn_env_create: robot_visible needs human_num + human_num_range <= %d (the robot is one more ORCA neighbour)", CN_MAX_HUMANS - 1);
    CN_REQUIRE(!cfg->robot_visible || cfg->env_kind != CN_ENV_PRED || cfg->predict_truth,
               "cn_env_create: robot_visible in CrowdSimPred-v0 needs sim.predict_method = 'truth' (with 'const_vel' the reference itself "
               "fails: crowd_sim_var_num.py:174 assigns H previous human states to H + 1 rows)");
    CN_REQUIRE(!cfg->predict_truth || cfg->env_kind == CN_ENV_PRED,
               "cn_env_create: predict_truth (sim.predict_method = 'truth') is CrowdSimPred-v0");
    CN_REQUIRE(cfg->time_step > 0 && std::fabs(5.0 / cfg->time_step - std::round(5.0 / cfg->time_step)) < 1e-9,
               "cn_env_create: time_step must divide 5 s");
    cn_env_batch *b = new (std::nothrow) cn_env_batch{};
    CN_REQUIRE(b, "cn_env_create: out of host memory");
    EnvDev &d = b->d;
    d.cfg = *cfg;
    d.E = num_envs; d.H = HM; d.D = cn_env_obs_width(cfg); d.P = cfg->predict_steps;
    d.I = cfg->pred_interval > 1 ? cfg->pred_interval : 1; d.R = d.P * d.I;
    d.seed_base = seed + first_env_index;
    const size_t E = num_envs, H = HM;
    // one allocation, carved (all sub-buffers 256-byte aligned)
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~size_t(255); return o; };
    const size_t o_hum = carve(E * 8 * H * 8), o_rob = carve(E * 8 * 8), o_lhs = carve(E * 5 * H * 8);
    const size_t o_ft = cfg->env_kind == CN_ENV_PRED ? carve(E * d.P * 2 * H * 8) : 0;
    const size_t o_sc = carve(E * 4), o_cc = carve(E * 8), o_er = carve(E * 8), o_ec = carve(E * 4), o_nd = carve(E * 8);
    const size_t o_sv = carve(E * H), o_snd = carve(E * H * 4), o_ssr = carve(E * H * 4), o_ssm = carve(E * H * 4);
    const size_t o_seen = cfg->randomize_attributes ? carve(E * H * H * 4) : 0;
    const size_t o_mt = carve(E * MT_N * 4), o_mp = carve(E * 4), o_ha = carve(E * 2 * H * 4);
    const size_t o_nxh = carve(E * 8 * H * 8), o_nr = carve(E * 8 * 8), o_nn = carve(E * 8), o_nm = carve(E * MT_N * 4), o_np = carve(E * 4), o_ny = carve(E),
                 o_npg = carve(E * 4), o_ncs = carve(E * 8);
    const bool test_phase = cfg->phase == CN_PHASE_TEST;
    const bool truth_obs = cfg->predict_truth != 0;
    const bool rob_orca = cfg->robot_policy == CN_ROBOT_ORCA;
    const size_t o_rsv = rob_orca ? carve(E) : 0, o_rnd = rob_orca ? carve(E * 4) : 0, o_rsn = rob_orca ? carve(E * H * 4) : 0;
    const size_t o_tr = (test_phase || truth_obs) ? carve(E * (d.R + 1) * 4 * H * 8) : 0, o_vis = (test_phase || truth_obs) ? carve(E * H) : 0, o_md = carve(E * 8);
    const size_t o_pend = carve(E);
    const bool unicycle = cfg->kinematics == CN_KIN_UNICYCLE;
    const bool var_n = cfg->human_num_range > 0 || unicycle; // a unicycle episode holds randint(1, H + 1) humans
    const size_t o_nh = var_n ? carve(E * 4) : 0, o_nxnh = var_n ? carve(E * 4) : 0, o_oc = var_n ? carve(E * 4) : 0, o_om = var_n ? carve(E * 4) : 0;
    // agent count each private simulator was built for: the crowd size varies, or (robot.visible with 'truth' roll-outs) the real step
    // passes H others + the robot while the roll-outs pass the H - 1 fellow humans only -> two rebuilds per step (orca.py:80-82)
    const bool need_simn = var_n || (cfg->robot_visible && (test_phase || truth_obs));
    const size_t o_simn = need_simn ? carve(E * H) : 0, o_rsimn = (var_n && rob_orca) ? carve(E) : 0;
    const size_t o_dv = unicycle ? carve(E * 8) : 0;
    const bool wheel_model = unicycle && cfg->env_kind != CN_ENV_VARNUM; // CrowdSimPred.step's smooth_action
    const size_t o_wh = wheel_model ? carve(E * 4 * 8) : 0;
    const bool lane_orca = HM + (cfg->robot_visible ? 1 : 0) <= 32 && cfg->humans_policy == CN_HUMANS_ORCA && cfg->human_fov >= 2.0;
    const bool collect = cfg->env_kind == CN_ENV_COLLECT;
    const size_t o_pid = collect ? carve(E * H * 4) : 0, o_mpid = collect ? carve(E * 4) : 0, o_lobs = collect ? carve(E * H) : 0;
    const size_t state_bytes = off; // everything below is per-step scratch of the ORCA pass: not part of a snapshot
    const size_t o_pc = carve(4), o_pl = carve(E * 4); // envs with deferred post-observation updates (env_post_kernel)
    const size_t o_pa = carve(4); // arrival counter of the row-plan builders (row_plan.h): zero here, reset by the last builder of every build
    const size_t o_l3c = carve(4), o_l3h = lane_orca ? carve(E * H * sizeof(Lp3Hdr)) : 0, o_l3l = lane_orca ? carve(E * H * 32 * sizeof(float4)) : 0;
    char *base = nullptr;
    hipError_t herr = hipMalloc((void **)&base, off);
    if (herr != hipSuccess) { delete b; cn_set_error("cn_env_create: hipMalloc(%zu) failed: %s", off, hipGetErrorString(herr)); return CN_ERR_HIP; }
    herr = hipMemset(base, 0, off);
    if (herr != hipSuccess) { (void)hipFree(base); delete b; cn_set_error("cn_env_create: hipMemset failed: %s", hipGetErrorString(herr)); return CN_ERR_HIP; }
    b->blob = base;
    b->blob_bytes = state_bytes;
    d.hum = (double *)(base + o_hum); d.rob = (double *)(base + o_rob); d.lhs = (double *)(base + o_lhs);
    d.ftraj = cfg->env_kind == CN_ENV_PRED ? (double *)(base + o_ft) : nullptr;
    d.step_counter = (int32_t *)(base + o_sc); d.case_counter = (uint64_t *)(base + o_cc);
    d.ep_ret = (double *)(base + o_er); d.ep_cnt = (int32_t *)(base + o_ec); d.shared_nd = (double *)(base + o_nd);
    d.sim_valid = (uint8_t *)(base + o_sv); d.sim_nd = (float *)(base + o_snd); d.sim_self_radius = (float *)(base + o_ssr);
    d.sim_self_maxspeed = (float *)(base + o_ssm);
    d.sim_seen = cfg->randomize_attributes ? (float *)(base + o_seen) : nullptr;
    d.mt = (uint32_t *)(base + o_mt); d.mt_pos = (int32_t *)(base + o_mp); d.hact = (float *)(base + o_ha);
    d.nx_hum = (double *)(base + o_nxh); d.nx_rob = (double *)(base + o_nr); d.nx_shared_nd = (double *)(base + o_nn);
    d.nx_mt = (uint32_t *)(base + o_nm); d.nx_mt_pos = (int32_t *)(base + o_np); d.nx_ready = (uint8_t *)(base + o_ny);
    d.plan_arrive = (int32_t *)(base + o_pa);
    d.post_cnt = (int32_t *)(base + o_pc); d.post_list = (int32_t *)(base + o_pl);
    d.nx_prog = (int32_t *)(base + o_npg); d.nx_case = (uint64_t *)(base + o_ncs);
    d.tr = (test_phase || truth_obs) ? (double *)(base + o_tr) : nullptr; d.vis = (test_phase || truth_obs) ? (uint8_t *)(base + o_vis) : nullptr;
    d.pend = (uint8_t *)(base + o_pend);
    d.nh = var_n ? (int32_t *)(base + o_nh) : nullptr; d.nx_nh = var_n ? (int32_t *)(base + o_nxnh) : nullptr;
    d.obs_cnt = var_n ? (int32_t *)(base + o_oc) : nullptr; d.obs_max = var_n ? (int32_t *)(base + o_om) : nullptr;
    d.desired_v = unicycle ? (double *)(base + o_dv) : nullptr;
    d.wheel = wheel_model ? (double *)(base + o_wh) : nullptr;
    d.pred_id = collect ? (int32_t *)(base + o_pid) : nullptr; d.max_pid = collect ? (int32_t *)(base + o_mpid) : nullptr;
    d.last_obs = collect ? (uint8_t *)(base + o_lobs) : nullptr;
    d.lp3_cnt = (int32_t *)(base + o_l3c);
    d.lp3_hdr = lane_orca ? (Lp3Hdr *)(base + o_l3h) : nullptr; d.lp3_lines = lane_orca ? (float4 *)(base + o_l3l) : nullptr;
    d.sim_n = need_simn ? (uint8_t *)(base + o_simn) : nullptr; d.rob_sim_n = (var_n && rob_orca) ? (uint8_t *)(base + o_rsimn) : nullptr;
    d.min_dist = (double *)(base + o_md);
    d.rob_sim_valid = rob_orca ? (uint8_t *)(base + o_rsv) : nullptr; d.rob_nd = rob_orca ? (float *)(base + o_rnd) : nullptr;
    d.rob_seen = rob_orca ? (float *)(base + o_rsn) : nullptr;
    b->reset_done = false;
    b->orca_ready = false;
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest); // side work yields to the caller's stream (critical path)
    if (hipStreamCreateWithPriority(&b->side, hipStreamNonBlocking, prio_least) != hipSuccess || hipEventCreateWithFlags(&b->ev_state, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&b->ev_orca, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&b->ev_pre, hipEventDisableTiming) != hipSuccess ||
        hipStreamCreateWithPriority(&b->side2, hipStreamNonBlocking, prio_least) != hipSuccess || hipEventCreateWithFlags(&b->ev_pg, hipEventDisableTiming) != hipSuccess) {
        (void)hipFree(base); delete b; cn_set_error("cn_env_create: stream/event creation failed"); return CN_ERR_HIP;
    }
    // the row plan is built by the lane kernel's extra workgroup: only configs that run that kernel have one (and the consumer, the
    // two-team human-human kernel, takes crowds of <= 48 humans)
    b->plan_ok = lane_orca && HM <= RP_HMAX && num_envs <= RP_EMAX;
    b->pregen_ticks = 4000; // 40 us: see prefetch_orca
    b->lp3_blocks = lp3_grid(num_envs * HM);
    *out = b;
    return CN_OK;
}

extern "C" int cn_env_set_pregen_budget(cn_env_batch *env, int64_t ticks_10ns)
{
    CN_REQUIRE(env && ticks_10ns >= 0, "cn_env_set_pregen_budget: null handle or negative budget");
    env->pregen_ticks = ticks_10ns;
    return CN_OK;
}

extern "C" int64_t cn_row_plan_words(int num_envs) { return num_envs > 0 ? (int64_t)rp_words(num_envs) : 0; }

// The row-plan builder on its own, for counts the caller supplies: the rowplan::build the lane kernel hosts, one workgroup per group.
// (No batch: the groups' arrival counter is header word 7, cleared in front of the launch and left at zero by the last group.)
__global__ __launch_bounds__(64) void row_plan_kernel(int E, int H, const float *det, int32_t *plan)
{
    __shared__ rowplan::Lds lds;
    rowplan::build((int)blockIdx.x, (int)gridDim.x, E, H, rp_workgroups(E, H), det, plan, lds);
}

extern "C" int cn_row_plan_build(int num_envs, int rows, const float *detected_human_num, int32_t *row_plan, void *stream)
{
    if (int rc = cn_require_device()) return rc;
    CN_REQUIRE(num_envs > 0 && rows >= 1 && detected_human_num && row_plan, "cn_row_plan_build: null argument or empty batch");
    CN_REQUIRE((((uintptr_t)detected_human_num | (uintptr_t)row_plan) & 15u) == 0, "cn_row_plan_build: both buffers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    CN_HIP(hipMemsetAsync(row_plan, 0, RP_HDR * sizeof(int32_t), st));
    // (a batch the builder does not take -- more than RP_EMAX envs or RP_HMAX rows, a size that is no multiple of four -- leaves word 0 zero)
    if (num_envs > RP_EMAX) return CN_OK;
    hipLaunchKernelGGL(row_plan_kernel, dim3(rp_groups(num_envs)), dim3(64), 0, st, num_envs, rows, detected_human_num, row_plan);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_env_destroy(cn_env_batch *env)
{
    if (!env) return CN_OK;
    (void)hipStreamSynchronize(env->side);
    if (env->side2) { (void)hipStreamSynchronize(env->side2); (void)hipStreamDestroy(env->side2); }
    if (env->ev_pg) (void)hipEventDestroy(env->ev_pg);
    (void)hipEventDestroy(env->ev_state); (void)hipEventDestroy(env->ev_orca); (void)hipEventDestroy(env->ev_pre); (void)hipStreamDestroy(env->side);
    if (env->blob) CN_HIP(hipFree(env->blob));
    delete env;
    return CN_OK;
}

// who: prefix of the message ("" as cn_env_reset / cn_env_step always reported it, "cn_env_set_scene: " for the call that names itself)
static int check_obs(const cn_obs *obs, const char *who = "")
{
    CN_REQUIRE(obs && obs->robot_node && obs->temporal_edges && obs->spatial_edges && obs->detected_human_num,
               "%sobservation pointers must be non-null (visible_masks may be null)", who);
    // the plan builder (row_plan.h) writes the plan as int4 (and reads detected_human_num as float4: a count view at an odd offset, e.g. a
    // storage row of a batch whose size is not a multiple of four, simply gets no plan -- prefetch_orca)
    CN_REQUIRE(!obs->row_plan || ((uintptr_t)obs->row_plan & 15u) == 0,
               "%scn_obs.row_plan must be 16-byte aligned and hold cn_row_plan_words(E) int32 words", who);
    return CN_OK;
}

extern "C" int cn_env_reset(cn_env_batch *env, const cn_obs *obs, void *stream)
{
    CN_REQUIRE(env, "cn_env_reset: null handle");
    if (int rc = check_obs(obs)) return rc;
    hipStream_t st = (hipStream_t)stream;
    // VecEnv.reset() resets every env; case counters keep running (crowd_sim_var_num.py:348)
    if (int rc = sync_side(env, st)) return rc; // an in-flight prefetch reads the old state
    const bool split = env->d.cfg.predict_truth != 0;
    hipLaunchKernelGGL(env_reset_kernel, dim3(env->d.E), dim3(64), 0, st, env->d, *obs, split ? 0 : 1);
    CN_CHECK_LAUNCH();
    if (split) { if (int rc = truth_rollout_and_obs(env, obs, st)) return rc; }
    env->reset_done = true;
    return prefetch_orca(env, st, obs);
}

extern "C" int cn_env_set_scene(cn_env_batch *env, const uint8_t *select, const double *humans, const double *robot, const cn_obs *obs, void *stream)
{
    // every refusal in front of the first launch (and of the first read of *env: the pointers are looked at first)
    CN_REQUIRE(env, "cn_env_set_scene: null handle");
    CN_REQUIRE(humans && robot, "cn_env_set_scene: humans [E,H,8] and robot [E,8] are required (device, float64, cn_env_get_state's layout)");
    if (int rc = check_obs(obs, "cn_env_set_scene: ")) return rc;
    CN_REQUIRE(env->reset_done, "cn_env_set_scene: the batch was never reset (a scene keeps the radii, speed limits, crowd size and private "
               "simulators the env's last reset made: call cn_env_reset first)");
    CN_REQUIRE(env->d.cfg.env_kind != CN_ENV_COLLECT, "cn_env_set_scene: CrowdSimVarNumCollect-v0 takes no scenes");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = sync_side(env, st)) return rc; // an in-flight prefetch reads the old state
    const bool split = env->d.cfg.predict_truth != 0;
    hipLaunchKernelGGL(env_scene_kernel, dim3(env->d.E), dim3(64), 0, st, env->d, select, humans, robot, *obs, split ? 0 : 1);
    CN_CHECK_LAUNCH();
    if (split) { if (int rc = truth_rollout_and_obs(env, obs, st, true)) return rc; }
    // the velocities prefetched for the replaced state are dropped, those of the whole batch with them: one ORCA pass serves every env, and
    // on an unchanged env it is a pure function of state the scene left alone
    env->orca_ready = false;
    return prefetch_orca(env, st, obs);
}

extern "C" int cn_env_step(cn_env_batch *env, const float *actions, const cn_obs *obs, float *reward, uint8_t *done,
                           uint8_t *info, double *ep_return, int32_t *ep_len, float *not_done, void *stream)
{
    CN_REQUIRE(env, "cn_env_step: null handle");
    if (!env->reset_done) { cn_set_error("cn_env_step: call cn_env_reset first"); return CN_ERR_STATE; }
    if (int rc = check_obs(obs)) return rc;
    CN_REQUIRE(actions && reward && done && info && ep_return && ep_len, "cn_env_step: null output/input pointer");
    hipStream_t st = (hipStream_t)stream;
    if (!env->orca_ready && !env->tail_pending) { if (int rc = prefetch_orca(env, st, nullptr)) return rc; }
    if (int rc = sync_side(env, st)) return rc; // human velocities for the current state (computed on the side stream; a held-back tail goes out now)
    bool pre_bound = false;
    if (env->d.cfg.predict_truth) {
        hipLaunchKernelGGL(env_step_kernel<true>, dim3(env->d.E), dim3(64), 0, st, stamped(env->d, CN_K_ENV_STEP), actions, *obs, reward, done, info, ep_return, ep_len, not_done);
        CN_CHECK_LAUNCH();
        if (int rc = truth_rollout_and_obs(env, obs, st)) return rc;
    } else {
        const bool coop = dense_crowd(env);
        // without a lane kernel the next consumer of the goals is the ORCA pass on the side stream: the updates go there, in front of it
        // (with one, that kernel follows on the caller's stream and the loops stay in the step kernel, on four wavefronts)
        const bool defer = coop && !lane_path_of(env) && env->d.cfg.humans_policy == CN_HUMANS_ORCA;
        auto step = env_step_kernel<false>;
        int threads = 64;
        if (defer) {
            CN_HIP(hipMemsetAsync(env->d.post_cnt, 0, 4, st));
            step = env_step_kernel<false, 1, true>;
            env->post_deferred = true;
        }
        else if (coop) { step = env_step_kernel<false, 4>; threads = 256; }
        else if (train_profile(env)) step = env_step_kernel<false, 1, false, ProfileTrain>;
        // prefetch_orca follows at once: where it releases the pre-generation (the tail not held back), this launch's stop event does
        pre_bound = !(env->defer_tail && lane_path_of(env)) && !capturing(st);
        launch_ev(step, dim3(env->d.E), dim3(threads), st, pre_bound ? env->ev_pre : nullptr, stamped(env->d, CN_K_ENV_STEP), actions, *obs, reward, done, info,
                  ep_return, ep_len, not_done);
        CN_CHECK_LAUNCH();
    }
    return prefetch_orca(env, st, obs, pre_bound); // next step's ORCA overlaps whatever the caller enqueues next (the policy forward)
}

extern "C" int cn_env_join(cn_env_batch *env, void *stream)
{
    CN_REQUIRE(env, "cn_env_join: null handle");
    return sync_side(env, (hipStream_t)stream);
}

extern "C" int cn_env_get_state(cn_env_batch *env, double *humans, double *robot, void *stream)
{
    CN_REQUIRE(env, "cn_env_get_state: null handle");
    if (int rc = sync_side(env, (hipStream_t)stream)) return rc; // ORCA also (re)builds sim_* lazily
    const int n = env->d.E * env->d.H * 8;
    hipLaunchKernelGGL(export_state_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, env->d, humans, robot);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_env_get_human_actions(cn_env_batch *env, float *out, void *stream)
{
    CN_REQUIRE(env && out, "cn_env_get_human_actions: null argument");
    // the velocities applied by the LAST step were overwritten by the prefetch for the next one: report the prefetched
    // ones (= the velocities the next step will apply), ordered behind the side stream
    if (int rc = sync_side(env, (hipStream_t)stream)) return rc;
    const int n = env->d.E * env->d.H * 2;
    hipLaunchKernelGGL(export_hact_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, env->d, out);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_env_get_human_counts(cn_env_batch *env, int32_t *out, void *stream)
{
    CN_REQUIRE(env && out, "cn_env_get_human_counts: null argument");
    hipStream_t st = (hipStream_t)stream;
    if (env->d.nh) {
        CN_HIP(hipMemcpyAsync(out, env->d.nh, (size_t)env->d.E * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    } else {
        hipLaunchKernelGGL(fill_i32_kernel, dim3((env->d.E + 255) / 256), dim3(256), 0, st, env->d.E, env->d.H, out);
        CN_CHECK_LAUNCH();
    }
    return CN_OK;
}

extern "C" int cn_env_get_visibility(cn_env_batch *env, uint8_t *out, void *stream)
{
    CN_REQUIRE(env && out, "cn_env_get_visibility: null argument");
    if (int rc = sync_side(env, (hipStream_t)stream)) return rc; // ordered like cn_env_get_state
    const int n = env->d.E * env->d.H;
    hipLaunchKernelGGL(export_visibility_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, env->d, out);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_env_trace_append(cn_env_batch *env, const int64_t *active, const int64_t *index, int cap, float *agents, uint8_t *flags,
                                   float *goal, int32_t *length, void *stream)
{
    CN_REQUIRE(env, "cn_env_trace_append: null handle");
    CN_REQUIRE(cap >= 1, "cn_env_trace_append: cap=%d records per env (at least 1)", cap);
    CN_REQUIRE(index && agents && flags && length, "cn_env_trace_append: index, agents, flags and length are required");
    CN_REQUIRE(((uintptr_t)agents & 7u) == 0, "cn_env_trace_append: agents must be 8-byte aligned");
    if (int rc = sync_side(env, (hipStream_t)stream)) return rc; // ordered like cn_env_get_state
    const int n = env->d.E * (env->d.H + 1);
    hipLaunchKernelGGL(trace_append_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, env->d, active, index, cap, agents, flags, goal,
                       length);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_env_set_case_counters(cn_env_batch *env, const uint64_t *counters, void *stream)
{
    CN_REQUIRE(env && counters, "cn_env_set_case_counters: null argument");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = sync_side(env, st)) return rc; // the side stream may be pre-generating episodes
    CN_HIP(hipMemcpyAsync(env->d.case_counter, counters, (size_t)env->d.E * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    CN_HIP(hipMemsetAsync(env->d.nx_ready, 0, (size_t)env->d.E, st)); // staged episodes were generated for the old counters
    return CN_OK;
}

// ---- checkpointing (train.py:213-219 only saves the policy; a bit-exact --resume also needs the simulator) ----------
// The whole persistent state of a batch is ONE device blob (agent records, beliefs, counters, private ORCA simulators, the
// numpy MT19937 streams, the staged next episodes, the prefetched ORCA velocities): a snapshot is that blob behind a small
// header that pins the layout it was taken from.
struct SnapHeader {
    uint64_t magic, blob_bytes;
    int32_t E, H, D, P;
    int64_t seed_base;
    cn_env_config cfg;
    int32_t reset_done, pad;
};
constexpr uint64_t SNAP_MAGIC = 0x434e454e56303034ull; // "CNENV004" (round 4: cn_env_config gained fields since 002/003, the blob nx_prog / nx_case / wheel)
constexpr uint64_t SNAP_MAGIC_MASK = 0xffffffffff000000ull; // "CNENV" + three digits

extern "C" int64_t cn_env_snapshot_bytes(const cn_env_batch *env)
{
    return env ? (int64_t)(sizeof(SnapHeader) + env->blob_bytes) : 0;
}

extern "C" int cn_env_save(cn_env_batch *env, void *dst, void *stream)
{
    CN_REQUIRE(env && dst, "cn_env_save: null argument");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = sync_side(env, st)) return rc; // the side stream owns hact / sim_* / nx_* until then
    SnapHeader h{};
    h.magic = SNAP_MAGIC; h.blob_bytes = env->blob_bytes; h.E = env->d.E; h.H = env->d.H; h.D = env->d.D; h.P = env->d.P;
    h.seed_base = env->d.seed_base; h.cfg = env->d.cfg; h.reset_done = env->reset_done ? 1 : 0;
    CN_HIP(hipMemcpyAsync(dst, &h, sizeof(h), hipMemcpyHostToDevice, st));
    CN_HIP(hipMemcpyAsync((char *)dst + sizeof(h), env->blob, env->blob_bytes, hipMemcpyDeviceToDevice, st));
    CN_HIP(hipStreamSynchronize(st)); // `h` lives on this stack frame
    return CN_OK;
}

extern "C" int cn_env_load(cn_env_batch *env, const void *src, void *stream)
{
    CN_REQUIRE(env && src, "cn_env_load: null argument");
    hipStream_t st = (hipStream_t)stream;
    SnapHeader h{};
    CN_HIP(hipMemcpyAsync(&h, src, sizeof(h), hipMemcpyDeviceToHost, st));
    CN_HIP(hipStreamSynchronize(st));
    CN_REQUIRE((h.magic & SNAP_MAGIC_MASK) == (SNAP_MAGIC & SNAP_MAGIC_MASK), "cn_env_load: not a cn_env snapshot (bad magic)");
    CN_REQUIRE(h.magic == SNAP_MAGIC, "cn_env_load: snapshot from another layout version (CNENV%c%c%c; this library reads and writes CNENV004): "
               "snapshots do not carry over between library versions", (char)(h.magic >> 16), (char)(h.magic >> 8), (char)h.magic);
    CN_REQUIRE(h.blob_bytes == env->blob_bytes && h.E == env->d.E && h.H == env->d.H && h.D == env->d.D && h.P == env->d.P &&
                   h.seed_base == env->d.seed_base && std::memcmp(&h.cfg, &env->d.cfg, sizeof(cn_env_config)) == 0,
               "cn_env_load: the snapshot was taken from a batch with a different shape, seed, shard or configuration "
               "(E=%d H=%d seed_base=%lld vs E=%d H=%d seed_base=%lld)", h.E, h.H, (long long)h.seed_base, env->d.E, env->d.H, (long long)env->d.seed_base);
    CN_HIP(hipStreamSynchronize(env->side)); // nothing of ours may still be writing the blob
    CN_HIP(hipStreamSynchronize(env->side2));
    env->pg_pending = false;
    CN_HIP(hipMemcpyAsync(env->blob, (const char *)src + sizeof(h), env->blob_bytes, hipMemcpyDeviceToDevice, st));
    CN_HIP(hipMemsetAsync(env->d.lp3_cnt, 0, sizeof(int32_t), st)); // scratch of the ORCA pass (normally cleared by the step / reset kernels)
    env->reset_done = h.reset_done != 0;
    // the snapshot holds the prefetched velocities of its state, but the event that orders them is gone: recompute on demand
    // (orca_kernel / env_pregen_kernel are pure functions of the restored state, so the continuation is bit-identical)
    env->orca_ready = false;
    env->tail_pending = false;
    return CN_OK;
}

extern "C" int cn_env_set_tail_deferral(cn_env_batch *env, int enabled)
{
    CN_REQUIRE(env, "cn_env_set_tail_deferral: null handle");
    env->defer_tail = enabled != 0;
    return CN_OK;
}

extern "C" int cn_env_launch_tail(cn_env_batch *env, void *stream)
{
    CN_REQUIRE(env, "cn_env_launch_tail: null handle");
    if (!env->tail_pending) return CN_OK; // nothing held back (mode off, no step since, or already out)
    return launch_tail(env, (hipStream_t)stream);
}

extern "C" int cn_env_get_danger_min_dist(cn_env_batch *env, double *out, void *stream)
{
    CN_REQUIRE(env && out, "cn_env_get_danger_min_dist: null argument");
    CN_HIP(hipMemcpyAsync(out, env->d.min_dist, (size_t)env->d.E * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CN_OK;
}

extern "C" int cn_orca_solve(int B, int n_other, const float *self, const float *others, float neighbor_dist, int max_neighbors,
                             float time_horizon, float time_step, float *out_vel, void *stream)
{
    if (int rc = cn_require_device()) return rc;
    CN_REQUIRE(B >= 0 && n_other >= 0 && n_other <= 63, "cn_orca_solve: n_other must be in [0,63]");
    CN_REQUIRE(self && out_vel && (others || n_other == 0), "cn_orca_solve: null pointer");
    if (B == 0) return CN_OK;
    hipLaunchKernelGGL(orca_solve_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, B, n_other, self, others,
                       neighbor_dist, max_neighbors, time_horizon, time_step, out_vel);
    CN_CHECK_LAUNCH();
    return CN_OK;
}
