// env_dev.h -- the simulator's device state: EnvDev (every per-env array of a batch, passed to each launch by value), the
// linearProgram3 hand-off record Lp3Hdr, and the field indices of the human and robot records.  Part of env_sim.hip's translation unit.
#pragma once
#include "common.h"

namespace {

constexpr int MT_N = 624;
constexpr float RVO_EPS = 0.00001f;

struct Lp3Hdr { int32_t agent, nn, line_fail; float rx, ry, radius; };

struct EnvDev {
    cn_env_config cfg;
    int E, H, D, P;
    int I, R;          // pred_interval (crowd_sim.py:180) and the 'truth' roll count R = P * I (buffer_len, :181); slice k * I of `tr` is prediction k
    int64_t seed_base; // thisSeed of env 0 of this batch
    // humans [E][8][H] double: px,py,vx,vy,gx,gy,radius,v_pref
    double *hum;
    // robot [E][8] double: px,py,vx,vy,gx,gy,theta,potential
    double *rob;
    double *lhs;   // last_human_states [E][5][H]
    double *ftraj; // [E][P][2][H] predicted positions k=1..P (const_vel), only for CN_ENV_PRED
    int32_t *step_counter; // [E]
    uint64_t *case_counter; // [E]
    double *ep_ret;         // [E] running episode return
    int32_t *ep_cnt;        // [E] running episode length
    double *shared_nd;      // [E] config.orca.neighbor_dist
    uint8_t *sim_valid;     // [E][H]
    float *sim_nd, *sim_self_radius, *sim_self_maxspeed; // [E][H]
    float *sim_seen; // [E][H][H] or nullptr (non-randomised: radii never change)
    uint32_t *mt;    // [E][624]
    int32_t *mt_pos; // [E]
    float *hact;     // [E][2][H] ORCA velocities of this step
    // next-episode staging: episode k+1 of env e is a pure function of (seed, e, k), so it is generated ahead of time on
    // the side stream (env_pregen_kernel) and a finishing env only copies it in (the serial MT19937 seeding + rejection
    // sampling of 20 humans would otherwise be the tail of env_step_kernel)
    double *nx_hum;     // [E][8][H]
    double *nx_rob;     // [E][8]
    double *nx_shared_nd; // [E]
    uint32_t *nx_mt;    // [E][624]
    int32_t *nx_mt_pos; // [E]
    int32_t *post_cnt, *post_list; // [1], [E] envs whose post-observation updates (goal changes, respawns) this step deferred to env_post_kernel
    int32_t *plan_arrive; // [1] row-plan builders' arrival counter (library-owned: the caller's plan buffer may hold anything)
    int coop_after;       // candidates a placement loop evaluates on one wavefront before the env's helper wavefronts join (env_step_kernel<false, 4>)
    uint8_t *nx_ready;  // [E]
    int32_t *nx_prog;   // [E] pre-generation in progress: 0 = not started, k + 1 = seed, robot and the first k humans are staged
    uint64_t *nx_case;  // [E] the case counter that staging was started for (a reset in between makes it stale)
    // test phase only (crowd_sim_var_num.py:386-388, :499-511): the humans' true future states rolled out with their own
    // ORCA policies, the robot's visibility flags of the last observation, and Danger's min_dist of the last step
    // robot.policy == 'orca': the robot's own rvo2 simulator, created at its first use and kept across episodes (orca.py:80-89)
    uint8_t *rob_sim_valid; // [E]
    float *rob_nd;          // [E]   neighbour distance frozen at creation
    float *rob_seen;        // [E][H] believed radii (+0.01 + safety space) frozen at creation
    double *tr;       // [E][R+1][4][H] px,py,vx,vy of roll k = 0..R; slice 0 unused (k = 1 reads the live state)
    uint8_t *vis;     // [E][H]
    double *min_dist; // [E]
    uint8_t *pend;    // [E] predict_truth only: 1 = the env was reset by the first half of the step (observation still to be written)
    // sim.human_num_range > 0 only (all null otherwise): H is then human_num + human_num_range = the lane stride and the number of
    // observation rows, and the crowd of env e is its first nh[e] slots (crowd_sim_var_num.py:103-104, :404-437)
    int32_t *nh;        // [E] len(self.humans)
    int32_t *nx_nh;     // [E] ... of the staged next episode
    int32_t *obs_cnt;   // [E] len(self.observed_human_ids)
    int32_t *obs_max;   // [E] max(self.observed_human_ids), -1 when empty
    uint8_t *sim_n;     // [E][H] agent count human i's private simulator was built for (orca.py:80-82 rebuilds on a change)
    uint8_t *rob_sim_n; // [E] ... the robot's (robot.policy == 'orca')
    // CrowdSimVarNumCollect-v0 only (crowd_sim_var_num_collect.py): prediction ids for the GST dataset
    int32_t *pred_id;   // [E][H] self.human_pred_id
    int32_t *max_pid;   // [E]    self.max_human_id
    uint8_t *last_obs;  // [E][H] self.last_human_observability
    int32_t *lp3_cnt;   // [1] agents of this step's ORCA pass whose linear program was infeasible (orca_lane_kernel -> orca_lp3_kernel)
    struct Lp3Hdr *lp3_hdr; // [E*H] where linearProgram2 stopped
    float4 *lp3_lines;  // [E*H][32] their ORCA lines (point, direction) in neighbour order
    double *desired_v;  // [E] unicycle robot only: self.desiredVelocity[0] (crowd_sim.py:82: set at construction, never reset)
    double *wheel;      // [E][4] unicycle robot in CrowdSimPred / PredRealGST: smooth_action's last_left, last_right (crowd_sim.py:84-85, never
                        // reset) and RandomState's cached normal deviate: value, has_gauss as 0 / 1 (cleared by every np.random.seed)
    unsigned long long *stamp; // launch stamps of THIS launch (common.h: cn_stamp_slot), set on the by-value copy a launch passes; NULL = none
};
// the by-value kernel argument of one launch, with the stamp slot of `kernel_id` for the current step (measurement aid)
static EnvDev stamped(const EnvDev &d, int kernel_id) { EnvDev c = d; c.stamp = cn_stamp_slot(kernel_id); return c; }

template <class S>
__device__ __forceinline__ int crowd_size(const S &s, int e) { return s.nh ? s.nh[e] : s.H; }

// The reference's rejection sampling of human positions / goals is unbounded; after this many attempts the last candidate is
// accepted (same constant and rule in the oracle: oracle/crowdsim_oracle.h ORC_MAX_PLACEMENT_ATTEMPTS).
constexpr int CN_MAX_PLACEMENT_ATTEMPTS = 1 << 16;

enum { F_PX = 0, F_PY, F_VX, F_VY, F_GX, F_GY, F_RAD, F_VPREF };
enum { R_PX = 0, R_PY, R_VX, R_VY, R_GX, R_GY, R_THETA, R_POT };

} // namespace
