// env_profile.h -- compile-time config profiles of the simulator's step kernel.  Part of env_sim.hip's translation unit.
//
// env_step_kernel serves every configuration of cn_env_config, and nothing of a configuration changes while a
// batch exists: a setting the batch never takes still costs its run-time test, the scalar registers that keep its words alive across
// the common path and the spills those cause.  A PROFILE pins a set of settings at compile time.  The device code never reads EnvDev
// directly: it reads a VIEW with EnvDev's member names (EnvViewOf<PF>::type), whose members are
//   ProfileGeneric   EnvDev itself: every member is the run-time word (the code of a kernel that has no profile);
//   ProfileTrain     EnvTrain: a `static constexpr` where the profile pins the setting, a reference to the run-time word where it
//                    does not.  A test of a pinned member folds, and the block behind it goes away.
// The device helpers (episode.h, mt19937.h, det_math.h) are templates over the view type and spell `s.member` / `c.member` as ever.
// The host chooses once per launch (train_profile, env_sim.hip): a batch that misses ANY predicate takes the generic instantiation.
#pragma once
#include "env_dev.h"

namespace {

struct ProfileGeneric {};
// The default training class (BASELINE configs[1]: CrowdSimVarNum-v0, ORCA humans with fixed attributes, a network-driven holonomic
// robot the humans do not react to, phase train, a fixed crowd size, no narrowed field of view).  Everything train_profile() tests.
struct ProfileTrain {};

struct CfgTrain {
    static constexpr int32_t env_kind = CN_ENV_VARNUM;          // (not CrowdSimPred-v0: its observation loop and ftraj would stay live)
    static constexpr int32_t randomize_attributes = 0;          // no per-human radii: sim_seen == nullptr
    static constexpr int32_t phase = CN_PHASE_TRAIN;
    static constexpr int32_t robot_policy = CN_ROBOT_NETWORK;
    static constexpr int32_t robot_visible = 0;
    static constexpr int32_t predict_truth = 0;
    static constexpr int32_t human_num_range = 0;
    static constexpr int32_t kinematics = CN_KIN_HOLONOMIC;
    static constexpr int32_t humans_policy = CN_HUMANS_ORCA;
    // both fields of view are >= 2 (x pi); the code only ever asks `fov < 2.0` before it uses the value, so 2 stands for all of them
    static constexpr double robot_fov = 2.0, human_fov = 2.0;
    const int32_t &human_num, &predict_steps, &random_goal_changing, &end_goal_changing, &sort_humans, &nenv;
    const uint32_t &val_size, &test_size;
    const int32_t &auto_reset, &max_placement_attempts, &pred_interval;
    const double &time_step, &time_limit, &success_reward, &collision_penalty, &discomfort_dist, &discomfort_penalty_factor;
    const double &circle_radius, &arena_size, &human_radius, &human_v_pref, &robot_radius, &robot_v_pref, &sensor_range;
    const double &goal_change_chance, &end_goal_change_chance;
    const double &orca_neighbor_dist, &orca_safety_space, &orca_time_horizon, &orca_time_horizon_obst;
    const double &sf_A, &sf_B, &sf_KI;
    __host__ __device__ explicit CfgTrain(const cn_env_config &c)
        : human_num(c.human_num), predict_steps(c.predict_steps), random_goal_changing(c.random_goal_changing),
          end_goal_changing(c.end_goal_changing), sort_humans(c.sort_humans), nenv(c.nenv), val_size(c.val_size), test_size(c.test_size),
          auto_reset(c.auto_reset), max_placement_attempts(c.max_placement_attempts), pred_interval(c.pred_interval),
          time_step(c.time_step), time_limit(c.time_limit), success_reward(c.success_reward), collision_penalty(c.collision_penalty),
          discomfort_dist(c.discomfort_dist), discomfort_penalty_factor(c.discomfort_penalty_factor), circle_radius(c.circle_radius),
          arena_size(c.arena_size), human_radius(c.human_radius), human_v_pref(c.human_v_pref), robot_radius(c.robot_radius),
          robot_v_pref(c.robot_v_pref), sensor_range(c.sensor_range), goal_change_chance(c.goal_change_chance),
          end_goal_change_chance(c.end_goal_change_chance), orca_neighbor_dist(c.orca_neighbor_dist), orca_safety_space(c.orca_safety_space),
          orca_time_horizon(c.orca_time_horizon), orca_time_horizon_obst(c.orca_time_horizon_obst), sf_A(c.sf_A), sf_B(c.sf_B), sf_KI(c.sf_KI)
    {
    }
};

struct EnvTrain {
    const CfgTrain cfg;
    static constexpr int D = 2; // cn_env_obs_width of CrowdSimVarNum-v0
    const int &E, &H, &P, &I, &R;
    const int64_t &seed_base;
    // the arrays cn_env_create leaves null for every configuration of this class
    static constexpr double *ftraj = nullptr, *tr = nullptr, *desired_v = nullptr, *wheel = nullptr;
    static constexpr float *sim_seen = nullptr, *rob_nd = nullptr, *rob_seen = nullptr;
    static constexpr uint8_t *vis = nullptr, *sim_n = nullptr, *rob_sim_n = nullptr, *rob_sim_valid = nullptr, *last_obs = nullptr;
    static constexpr int32_t *nh = nullptr, *nx_nh = nullptr, *obs_cnt = nullptr, *obs_max = nullptr, *pred_id = nullptr, *max_pid = nullptr;
    double *const &hum, *const &rob, *const &lhs;
    int32_t *const &step_counter;
    uint64_t *const &case_counter;
    double *const &ep_ret;
    int32_t *const &ep_cnt;
    double *const &shared_nd;
    uint8_t *const &sim_valid;
    float *const &sim_nd, *const &sim_self_radius, *const &sim_self_maxspeed;
    uint32_t *const &mt;
    int32_t *const &mt_pos;
    float *const &hact;
    double *const &nx_hum, *const &nx_rob, *const &nx_shared_nd;
    uint32_t *const &nx_mt;
    int32_t *const &nx_mt_pos, *const &post_cnt, *const &post_list, *const &plan_arrive;
    const int &coop_after;
    uint8_t *const &nx_ready;
    int32_t *const &nx_prog;
    uint64_t *const &nx_case;
    double *const &min_dist;
    uint8_t *const &pend;
    int32_t *const &lp3_cnt;
    Lp3Hdr *const &lp3_hdr;
    float4 *const &lp3_lines;
    unsigned long long *const &stamp;
    __host__ __device__ explicit EnvTrain(const EnvDev &d)
        : cfg(d.cfg), E(d.E), H(d.H), P(d.P), I(d.I), R(d.R), seed_base(d.seed_base), hum(d.hum), rob(d.rob), lhs(d.lhs),
          step_counter(d.step_counter), case_counter(d.case_counter), ep_ret(d.ep_ret), ep_cnt(d.ep_cnt), shared_nd(d.shared_nd),
          sim_valid(d.sim_valid), sim_nd(d.sim_nd), sim_self_radius(d.sim_self_radius), sim_self_maxspeed(d.sim_self_maxspeed), mt(d.mt),
          mt_pos(d.mt_pos), hact(d.hact), nx_hum(d.nx_hum), nx_rob(d.nx_rob), nx_shared_nd(d.nx_shared_nd), nx_mt(d.nx_mt),
          nx_mt_pos(d.nx_mt_pos), post_cnt(d.post_cnt), post_list(d.post_list), plan_arrive(d.plan_arrive), coop_after(d.coop_after),
          nx_ready(d.nx_ready), nx_prog(d.nx_prog), nx_case(d.nx_case), min_dist(d.min_dist), pend(d.pend), lp3_cnt(d.lp3_cnt),
          lp3_hdr(d.lp3_hdr), lp3_lines(d.lp3_lines), stamp(d.stamp)
    {
    }
};

// does the batch belong to ProfileTrain's class?  (host; the pointer tests restate what cn_env_create derives from the config)
static bool train_profile_of(const EnvDev &d)
{
    const cn_env_config &c = d.cfg;
    return c.env_kind == CfgTrain::env_kind && c.randomize_attributes == CfgTrain::randomize_attributes && c.phase == CfgTrain::phase &&
           c.robot_policy == CfgTrain::robot_policy && c.robot_visible == CfgTrain::robot_visible && c.predict_truth == CfgTrain::predict_truth &&
           c.human_num_range == CfgTrain::human_num_range && c.kinematics == CfgTrain::kinematics && c.humans_policy == CfgTrain::humans_policy &&
           c.robot_fov >= 2.0 && c.human_fov >= 2.0 && d.D == EnvTrain::D &&
           !d.ftraj && !d.tr && !d.desired_v && !d.wheel && !d.sim_seen && !d.rob_nd && !d.rob_seen && !d.vis && !d.sim_n && !d.rob_sim_n &&
           !d.rob_sim_valid && !d.last_obs && !d.nh && !d.nx_nh && !d.obs_cnt && !d.obs_max && !d.pred_id && !d.max_pid;
}

// `typename EnvViewOf<PF>::type s(arg);` at the top of a kernel: the generic view IS the argument (a reference to it)
template <class PF> struct EnvViewOf;
template <> struct EnvViewOf<ProfileGeneric> { typedef const EnvDev &type; };
template <> struct EnvViewOf<ProfileTrain> { typedef const EnvTrain type; };

// a helper may take a cheaper, bit-identical instruction sequence where the view is pinned and leave the generic code as it is
template <class S> constexpr bool view_pinned = false;
template <> constexpr bool view_pinned<EnvTrain> = true;

} // namespace
