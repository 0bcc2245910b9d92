/*
 * crowdnav_hip.h -- C ABI of libcrowdnav_hip.so, the MI355X (gfx950) implementation of the CrowdNav++ hot path.
 *
 * The reference (Shuijing725/CrowdNav_Prediction_AttnGraph) is pure Python; its only native boundary on this path is
 * the third-party `rvo2` module.  There is therefore no existing FFI to bind to: this header defines the boundary a
 * maintainer would bind from the reference's Python (ctypes stub in INTEGRATION.md), one entry point per reference
 * interface it replaces:
 *
 *   cn_env_create/destroy      <- rl/networks/envs.py:97-140 make_vec_envs (+ :36-94 make_env: thisSeed = seed + rank,
 *                                 nenv, phase) and crowd_sim/envs/crowd_sim.py:88-202 configure()
 *   cn_env_reset               <- VecEnv.reset(): rl/networks/shmem_vec_env.py:74-79 -> crowd_sim_var_num.py:303-363
 *   cn_env_step                <- VecEnv.step(): shmem_vec_env.py:136-142 (auto-reset) -> crowd_sim_var_num.py:366-460
 *                                 / crowd_sim_pred.py:100-214, incl. ORCA humans (crowd_nav/policy/orca.py:64-117,
 *                                 i.e. rvo2.PyRVOSimulator.doStep) and bench.Monitor episode stats (envs.py:70-73)
 *   cn_orca_solve              <- rvo2: PyRVOSimulator.addAgent / setAgentPosition,Velocity,PrefVelocity / doStep / getAgentVelocity(0) (orca.py:80-114)
 *   cn_policy_create/destroy/set_weights <- rl/networks/model.py:16-46 Policy.__init__ / load_state_dict
 *   cn_policy_act              <- rl/networks/model.py:56-74 Policy.act (-> selfAttn_srnn_temp_node.py:360-449)
 *   cn_policy_get_value        <- rl/networks/model.py:76-80 Policy.get_value
 *   cn_srnn_create/destroy/set_weights <- rl/networks/model.py:16-46 Policy.__init__ with base='srnn' / load_state_dict
 *   cn_srnn_act                <- rl/networks/model.py:56-74 Policy.act (-> srnn_model.py:389-468 SRNN.forward, infer=True)
 *   cn_srnn_seq_fwd / _bwd      <- rl/ppo/ppo.py evaluate_actions on that base: the edge-GRU sequence of srnn_model.py:418-433 and its backward
 *   cn_srnn_attn_fwd / _bwd     <- ... the EdgeAttention of srnn_model.py:256-323 over that sequence's edge states and its backward
 *   cn_srnn_get_value          <- rl/networks/model.py:76-80 Policy.get_value on that base
 *   cn_gae                     <- rl/networks/storage.py:123-132 RolloutStorage.compute_returns (use_gae branch)
 *   cn_adv_stats / cn_adv_normalize <- rl/ppo/ppo.py:37-39 advantage normalisation (split so that N GPUs can
 *                                 all-reduce the three partial sums in between)
 *   cn_ppo_loss_fwd / cn_ppo_loss_bwd <- rl/ppo/ppo.py:66-84 clipped surrogate + clipped value loss (and their gradients)
 *   cn_adam_clip_step          <- rl/ppo/ppo.py:86-93 nn.utils.clip_grad_norm_ + torch.optim.Adam.step (ppo.py:32) over one flat bucket
 *   cn_linear_* / cn_hh_attention_* / cn_hr_attention_* / cn_gru_* / cn_embed0_*
 *                              <- the operators of Policy.evaluate_actions (rl/networks/model.py:82-90) as autograd runs
 *                                 them forward and backward inside PPO.update (rl/ppo/ppo.py:60-95)
 *   cn_env_get_danger_min_dist / cn_env_set_case_counters
 *                              <- test phase: Danger(min_dist) (crowd_sim_var_num.py:499-533) and the per-case seeding that
 *                                 rl/evaluation.py's protocol relies on (crowd_sim_var_num.py:316-318,337)
 *   cn_env_snapshot_bytes / cn_env_save / cn_env_load
 *                              <- (new) simulator state for a bit-exact --resume (train.py:105-108 restores the policy only)
 *   cn_gst_*                   <- gst_updated wrapper + VecPretextNormalize (CrowdSimPredRealGST-v0)
 *
 * Conventions: every function returns 0 on success and a negative cn_status otherwise (no C++ exception crosses the
 * ABI); cn_last_error() returns a thread-local message (the buffer is `thread_local`: concurrent callers on different
 * threads never see each other's text).  All tensor arguments are raw DEVICE pointers owned by the
 * caller (PyTorch allocates them); the library owns only the opaque handles (persistent per-env simulator state incl.
 * the numpy-compatible MT19937 streams, and the policy workspace / folded weights).  `stream` is a hipStream_t passed
 * as void*; all work is enqueued on it and nothing synchronises with the host.  A handle is re-entrant across handles,
 * not thread-safe on one handle.  There is no CPU fallback: every entry point fails if no gfx950 device is present.
 */
#ifndef CROWDNAV_HIP_H
#define CROWDNAV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    CN_OK = 0,
    CN_ERR_INVALID = -1,   /* bad argument / unsupported configuration */
    CN_ERR_HIP = -2,       /* a HIP runtime call failed (see cn_last_error) */
    CN_ERR_NO_DEVICE = -3, /* no gfx950 device visible */
    CN_ERR_STATE = -4      /* call sequence error (e.g. step before reset, weights not set) */
} cn_status;

enum { CN_ENV_VARNUM = 0, CN_ENV_PRED = 1, CN_ENV_PRED_GST = 2, CN_ENV_COLLECT = 3 };   /* gym ids CrowdSimVarNum-v0 / CrowdSimPred-v0 /
                                                                                          * CrowdSimPredRealGST-v0 / CrowdSimVarNumCollect-v0 */
enum { CN_PHASE_TRAIN = 0, CN_PHASE_VAL = 1, CN_PHASE_TEST = 2 };
enum { CN_INFO_NOTHING = 0, CN_INFO_TIMEOUT = 1, CN_INFO_COLLISION = 2, CN_INFO_REACHGOAL = 3, CN_INFO_DANGER = 4 }; /* crowd_sim/envs/utils/info.py */

enum { CN_ROBOT_NETWORK = 0, CN_ROBOT_ORCA = 1, CN_ROBOT_SOCIAL_FORCE = 2 };
enum { CN_KIN_HOLONOMIC = 0, CN_KIN_UNICYCLE = 1 };   /* action_space.kinematics */
enum { CN_HUMANS_ORCA = 0, CN_HUMANS_SOCIAL_FORCE = 1 }; /* humans.policy */
#define CN_MAX_HUMANS 64 /* one wavefront lane per human */
#define CN_MAX_PRED 8

/* Mirrors the fields of crowd_nav/configs/config.py that the path reads (same names, same meaning). */
typedef struct {
    int32_t human_num;            /* sim.human_num */
    int32_t predict_steps;        /* sim.predict_steps */
    int32_t env_kind;             /* CN_ENV_* */
    int32_t randomize_attributes; /* env.randomize_attributes */
    int32_t random_goal_changing; /* humans.random_goal_changing */
    int32_t end_goal_changing;    /* humans.end_goal_changing */
    int32_t sort_humans;          /* args.sort_humans */
    int32_t phase;                /* CN_PHASE_TRAIN, CN_PHASE_TEST (seeds 1000 + case, 'truth' roll-out, future-zone Danger) or, CrowdSimPred-v0 only,
                                   * CN_PHASE_VAL (seeds 0 + case, Danger from the previous observation's predictions) */
    int32_t nenv;                 /* TOTAL number of envs across all GPUs: the case_counter stride (crowd_sim_var_num.py:348) */
    uint32_t val_size, test_size;
    int32_t robot_policy;         /* CN_ROBOT_NETWORK: cn_env_step's action drives the robot; CN_ROBOT_ORCA: robot.policy = 'orca'
                                   * (crowd_sim_var_num.py:371-375), ORCA on the robot's beliefs, the action argument is ignored;
                                   * CN_ROBOT_SOCIAL_FORCE: robot.policy = 'social_force' (crowd_nav/policy/social_force.py), likewise */
    int32_t robot_visible;        /* robot.visible: every human's ORCA / social force sees the robot as one more neighbour (crowd_sim.py:695-699);
                                   * human_num + human_num_range <= 63; not with CrowdSimPred-v0 + const_vel predictions (the reference fails there) */
    int32_t auto_reset;           /* 1 (default): vec-env semantics, a finished env is reset inside cn_env_step and `obs` holds the
                                   * reset observation (shmem_vec_env.py:139-142); 0: single gym env semantics
                                   * (crowd_sim_var_num.py:366-460 alone): the terminal observation is returned, cn_env_reset restarts */
    int32_t predict_truth;        /* CrowdSimPred-v0 with sim.predict_method = 'truth' (crowd_sim_pred.py:81, crowd_sim_var_num.py:180-206): the
                                   * observation carries the humans' TRUE future positions (their own ORCA rolled forward predict_steps
                                   * times from the state just reached) instead of constant-velocity extrapolations */
    int32_t max_placement_attempts; /* bound of the reference's UNBOUNDED rejection sampling of human positions / goals
                                   * (crowd_sim_var_num.py:116-146, crowd_sim.py:415-450): after this many attempts the last
                                   * candidate is accepted; 0 = 65536.  Dense randomised crowds have seeds where the reference
                                   * loop runs for minutes, and a batch waits for its slowest env.
                                   * SEMANTIC DEVIATION from the reference (which never gives up): an episode / goal change whose
                                   * loop reaches the bound places that human at a position that still violates the minimum
                                   * distance.  The C oracle has the same bound, so the bit-exact tests hold; none of the
                                   * reference-generated traces or shipped evaluation logs reaches it (20 humans: < 300 attempts
                                   * at worst); it matters for crowds of ~50 randomised humans (BASELINE configs[4]). */
    int32_t human_num_range;      /* sim.human_num_range: the crowd holds human_num - range .. human_num + range humans (drawn at reset,
                                   * changed every 5 s: crowd_sim_var_num.py:103-104, :404-437, crowd_sim_pred.py:165-190); observations
                                   * always have human_num + human_num_range rows, which must be <= CN_MAX_HUMANS */
    int32_t kinematics;           /* CN_KIN_* (action_space.kinematics); unicycle: network-driven robot; in CrowdSimPred-v0 / PredRealGST-v0 the command
                                   * passes through smooth_action's noisy wheel model (crowd_sim.py:315-358) */
    int32_t humans_policy;        /* CN_HUMANS_* (humans.policy) */
    int32_t pred_interval;        /* int(data.pred_timestep // env.time_step) (crowd_sim.py:180-181): prediction k lies k * pred_interval simulation steps
                                   * ahead -- const_vel offsets (crowd_sim_var_num.py:212); 'truth': predict_steps * pred_interval rolls of which every
                                   * pred_interval-th is kept (:181, :206).  0 = 1 (every shipped config); at most 16 */
    double time_step, time_limit;
    double success_reward, collision_penalty, discomfort_dist, discomfort_penalty_factor;
    double circle_radius, arena_size;
    double human_radius, human_v_pref;
    double robot_radius, robot_v_pref, sensor_range;
    double goal_change_chance, end_goal_change_chance;
    double orca_neighbor_dist, orca_safety_space, orca_time_horizon, orca_time_horizon_obst;
    double sf_A, sf_B, sf_KI;     /* config.sf.* (crowd_nav/policy/social_force.py) */
    double robot_fov, human_fov;  /* robot.FOV, humans.FOV in units of pi (crowd_sim.py:122-123, detect_visible :513-552); 2 = all round */
} cn_env_config;

/* CN_ENV_COLLECT (crowd_sim/envs/crowd_sim_var_num_collect.py, driven by collect_data.py): the dataset generator of the GST predictor.
 * spatial_edges is then pred_info [E,H,4] = (frame id, prediction id, absolute px, py of the robot's belief; +inf for humans the
 * robot does not see); reward is 0, an episode never ends, a robot at its goal draws a new one. */
/* Observation tensors exactly as VecPyTorch returns them (float32, contiguous):
 * robot_node [E,1,7], temporal_edges [E,1,2], spatial_edges [E,H,D] (D = 2 or 2*(predict_steps+1)),
 * detected_human_num [E,1], visible_masks [E,H] (uint8 0/1; may be NULL). */
typedef struct {
    float *robot_node;
    float *temporal_edges;
    float *spatial_edges;
    float *detected_human_num;
    uint8_t *visible_masks;
    int32_t *row_plan; /* optional (may be NULL), cn_row_plan_words(E) int32: derived data of detected_human_num that cn_env_reset / cn_env_step
                        * write beside the observation and cn_policy_act reads with it -- the row offsets of the compacted (env, human) rows
                        * and a packing of the envs into equally filled tiles for the fused human-human kernel (csrc/row_plan.h).  Valid only
                        * together with the observation it was written with.  Not part of the reference's observation: without it (NULL, or
                        * a config whose step does not build one) the policy derives the same row offsets itself and walks the envs in order.
                        * The buffer needs NO initialisation (any content, e.g. a fresh hipMalloc): every reset / step either writes a complete
                        * plan or clears word 0, and the builders' cross-workgroup counter lives in the batch's own memory. */
} cn_obs;

typedef struct cn_env_batch cn_env_batch;
typedef struct cn_policy cn_policy;

/* Bumped whenever a struct layout, a signature or the snapshot format changes (round 4: cn_obs.row_plan, cn_env_config.robot_fov /
 * human_fov, the profiling entry points, snapshot layout CNENV004); the ctypes binding refuses a library that reports another number. */
#define CN_ABI_VERSION 407
const char *cn_last_error(void);
int cn_version(void);
int cn_device_count(void);

void cn_env_config_default(cn_env_config *cfg);
/* num_envs envs on the current device; env i gets thisSeed = seed + first_env_index + i (global env index, so that
 * trajectories do not depend on how many GPUs the batch is sharded over). */
int cn_env_create(const cn_env_config *cfg, int num_envs, int64_t seed, int64_t first_env_index, cn_env_batch **out);
int cn_env_destroy(cn_env_batch *env);
int cn_env_obs_width(const cn_env_config *cfg);
/* Episodes are generated ahead of the reset that needs them (crowd_sim_var_num.py:303-363: seed, robot, humans by rejection sampling), on a
 * side stream beside the ORCA kernel.  One launch of that generator works for at most `ticks_10ns` x 10 ns per env and resumes in the next
 * step (default 4000 = 40 us): its wavefronts hold registers the policy's kernel, next on the caller's stream, needs.  The episodes do not
 * depend on the budget (0 = one human per launch); an env that resets before its next episode is complete generates it in place. */
int cn_env_set_pregen_budget(cn_env_batch *env, int64_t ticks_10ns);
/* Deferred tail.  A step leaves two pieces of work for its successor on the library's side stream: the ORCA programs the lane kernel could not
 * finish (a third of them: the linearProgram3 fallback) and the pre-generation of the next episodes.  By default cn_env_step enqueues them itself,
 * i.e. BEFORE whatever the caller enqueues next -- and when that is the policy's human-human kernel, which needs whole CUs, every wavefront of
 * the tail that got a CU first holds one of its workgroups back.  With deferral on, cn_env_step holds the tail back (configurations with the lane
 * kernel only) until cn_env_launch_tail(env, stream) -- to be called right after the big kernel went out on `stream`: the tail is ordered behind
 * that point and then runs beside the robot-node kernel.  cn_policy_set_post_hh_hook makes cn_policy_act call it at exactly that place.  A tail
 * nobody launched goes out with the next call that needs its results (cn_env_step, cn_env_reset, cn_env_save, the getters): results never depend
 * on the mode, only the timeline does. */
int cn_env_set_tail_deferral(cn_env_batch *env, int enabled);
int cn_env_launch_tail(cn_env_batch *env, void *stream);
/* int32 words of a cn_obs.row_plan buffer for a batch of num_envs envs */
int64_t cn_row_plan_words(int num_envs);
/* The row plan of an observation with these detected_human_num [num_envs] float32 (device, 16-byte aligned) and `rows` rows per env, into
 * row_plan (cn_row_plan_words(num_envs) int32, device, 16-byte aligned): what cn_env_reset / cn_env_step write, for counts of the caller's.
 * Word 0 stays zero where the builder does not take the batch. */
int cn_row_plan_build(int num_envs, int rows, const float *detected_human_num, int32_t *row_plan, void *stream);
int cn_env_reset(cn_env_batch *env, const cn_obs *obs, void *stream);
/* actions [E,2] float32 (raw policy output; clipped inside like srnn.clip_action).  Outputs: reward [E] float32,
 * done [E] uint8, info [E] uint8 (CN_INFO_*), ep_return [E] float64 and ep_len [E] int32 (valid where done: the
 * bench.Monitor episode sum / length), not_done [E] float32 = 1 - done (the `masks` of train.py:185-186; may be NULL).
 * Envs that finish are reset in the same launch and `obs` holds the reset observation for them (shmem_vec_env.py:139-142). */
int cn_env_step(cn_env_batch *env, const float *actions, const cn_obs *obs, float *reward, uint8_t *done, uint8_t *info,
                double *ep_return, int32_t *ep_len, float *not_done, void *stream);
/* Orders everything the library has in flight on its internal side stream (ORCA of the current state, next-episode pre-generation)
 * before whatever is enqueued on `stream` next.  cn_env_step does this itself; a caller needs it before reading simulator state from
 * another stream, or to close a hipGraph capture of a block of steps (a capture may not end with unjoined work on a forked stream).
 * Experimental: the only in-tree graph caller is the probe tools/graph_probe.py (replay measured slower than eager launches). */
int cn_env_join(cn_env_batch *env, void *stream);
/* Debug/test access to the simulator state: copies humans [E,H,8] (px,py,vx,vy,gx,gy,radius,v_pref) and robot [E,8]
 * (px,py,vx,vy,gx,gy,theta,potential) as float64 into caller DEVICE buffers (either may be NULL). */
int cn_env_get_state(cn_env_batch *env, double *humans, double *robot, void *stream);
/* Scenes: the selected envs of a batch start a NEW episode from a state of the caller's -- a crossing built by hand, a recorded state, what
 * cn_env_get_state gave a moment or a process ago.  What cn_env_get_state gives, this call takes.
 *   select [E] uint8 (device), or NULL for every env.
 *   humans [E,H,8] and robot [E,8] float64 (device) in the layout of cn_env_get_state.
 * TAKEN from each selected env's rows: px, py, vx, vy, gx, gy of the first cn_env_get_human_counts human slots; px, py, vx, vy, gx, gy, theta
 * of the robot.
 * NOT TAKEN: human columns 6 and 7 (radius, v_pref) -- the env keeps what its last reset (or a respawn since) made them: every human's
 * private ORCA simulator froze its own radius and speed limit and the radii it saw when it was built, and the neighbour distance of a
 * randomised crowd was drawn with them, so other values would need those simulators rebuilt (refused: out of scope, like a change of the
 * crowd size -- the crowd size stays the env's).  Robot column 7 (the potential) is recomputed as -||p - g||.
 * For a selected env this is the start of an episode, with the bookkeeping of a reset that had generated exactly this state:
 *   zeroed     the step counter (global time), the episode return and length;
 *   reset      the potential; the observation memory a reset initialises -- the robot's beliefs about the humans (last_human_states) and with
 *              them the previous velocities the const_vel predictor reads, the observed-human list of a varying crowd, human_visibility; and,
 *              with sim.predict_method = 'truth', the roll-out of the new state behind the observation (as in cn_env_reset);
 *   kept       the env's MT19937 stream where it stands (cached normal deviate included: the episode's random events -- goal changes,
 *              respawns, crowd-size changes -- draw from it), its case counter and its pre-generated NEXT episode: the auto-reset that ends
 *              the scene's episode starts the episode the env would have started next; the private simulators; a unicycle robot's commanded
 *              speed and wheel filter (the reference never resets them either).
 * The call then (1) writes the observation of the new state into the selected envs' rows of `obs` in reset form and builds the row plan of the
 * whole `obs`, (2) drops the prefetched ORCA velocities of the whole batch and (3) prefetches again as cn_env_reset does.
 * An env that is NOT selected keeps its state bit for bit, and its rows of `obs` are LEFT UNTOUCHED: writing an observation advances the
 * belief about every human the robot does not see and replaces the velocities the const_vel predictor extrapolates, so it cannot be done
 * twice for one state.  Pass the buffer that holds the batch's newest observation (what the last cn_env_reset / cn_env_step wrote) and `obs`
 * is a complete observation of the batch afterwards, row plan included.
 * No allocation, no host synchronisation.  CN_ERR_INVALID naming the call, before any launch: a NULL handle, humans, robot or obs (or a NULL
 * required member of obs), a batch that was never reset, CrowdSimVarNumCollect-v0.  The values themselves are the caller's to check (the
 * Python binding does: HipEnvBatch.set_scene(check=True)). */
int cn_env_set_scene(cn_env_batch *env, const uint8_t *select, const double *humans, const double *robot, const cn_obs *obs, void *stream);
/* ORCA velocities of the humans for the CURRENT state (the ones the next cn_env_step will apply; they are computed
 * ahead of time on an internal side stream, overlapped with the caller's policy forward), [E,H,2] float32 */
int cn_env_get_human_actions(cn_env_batch *env, float *out, void *stream);
/* Danger(min_dist) of the last step (crowd_sim_var_num.py:499-533): in the test phase the smallest distance between the
 * robot and an intruded TRUE future position of a visible human (humans rolled forward predict_steps times with their
 * own ORCA policies, calc_human_future_traj('truth') :152-206); 0 for every other info and in the train phase.
 * out [E] float64 (device). */
int cn_env_get_danger_min_dist(cn_env_batch *env, double *out, void *stream);
/* len(self.humans) of every env: out [E] int32 (device).  Constant human_num unless sim.human_num_range > 0; the slots beyond it in
 * cn_env_get_state / cn_env_get_human_actions hold no human. */
int cn_env_get_human_counts(cn_env_batch *env, int32_t *out, void *stream);
/* The robot-side detect_visible(robot, human, robot1=True) decision (crowd_sim.py:513-552) on the CURRENT state, by the device function the
 * observation decides with: configured sensor range and robot_fov, heading from the velocity or from theta by kinematics.  It is what the
 * reference's render colours its humans by (crowd_sim_pred.py:236-370, crowd_sim_var_num.py render: `self.human_visibility`).
 * out [E,H] uint8 (device), 0 in the slots beyond the env's crowd size.  Ordered like cn_env_get_state. */
int cn_env_get_visibility(cn_env_batch *env, uint8_t *out, void *stream);
/* Episode traces: append the CURRENT state of selected envs to caller-owned DEVICE buffers in ONE launch, with no allocation and no host
 * synchronisation -- the recording half of the per-episode trajectory figure the reference announces (test.py:31 --render_traj,
 * rl/networks/envs.py:226 VecPyTorch.render_traj) and never delivers; cn_trace_metrics and cn_render_trajectories below consume it.
 * Acts on every env e with (active == NULL || active[e] != 0) and 0 <= index[e] < cap: writes record index[e] of env e and sets
 * length[e] = index[e] + 1; every other env's buffers are left untouched.  active / index [E] int64 are meant to be the CN_EVAL_ACTIVE and
 * CN_EVAL_STEPS arrays of the cn_eval_accumulate state block as they are.  With A = H + 1 agent slots (H = the H of cn_env_get_state):
 *   agents [E,cap,A,6] float32, 8-byte aligned.  Slot 0 is the robot: px, py, vx, vy, radius (the configured one), theta.  Slot 1 + h is human
 *          slot h of cn_env_get_state: px, py, vx, vy, radius, v_pref.  Every value is the float64 state rounded once to float32; slots at or
 *          beyond the env's crowd size are written as zeros.
 *   flags  [E,cap,A] uint8.  Bit 0: the slot holds an agent (the robot: always; human slot h: h < cn_env_get_human_counts).  Bit 1: the
 *          cn_env_get_visibility decision, by the same device function; 0 in the robot's own slot.
 *   goal   [E,2] float32 (may be NULL): the robot's goal, written when index[e] == 0.
 *   length [E] int32.
 * Called once before every cn_env_step with index = the steps taken so far, record t of an episode is the state its t-th step was taken
 * FROM: record 0 is the reset state and length == the episode's step count.  The state AFTER the final step is not recorded: cn_env_step
 * replaces it with the next episode's start in the same launch, so no caller ever sees it.  Ordered like cn_env_get_state. */
int cn_env_trace_append(cn_env_batch *env, const int64_t *active, const int64_t *index, int cap, float *agents, uint8_t *flags, float *goal,
                        int32_t *length, void *stream);
/* Overwrite the per-env case counters (crowd_sim_var_num.py:316-318 `case_counter[phase] = test_case`, :337
 * rand_seed = offset[phase] + case_counter + thisSeed): the NEXT reset of env e generates the scenario of that case.
 * counters [E] uint64 (device).  Lets a batch replay chosen test cases (one per env) instead of consecutive ones. */
int cn_env_set_case_counters(cn_env_batch *env, const uint64_t *counters, void *stream);

/* Checkpointing of the simulator (the reference saves only the policy, train.py:213-219; resuming a run bit-exactly also needs
 * the env state: agent records, beliefs, case counters, private ORCA simulators, the numpy MT19937 streams).  A snapshot is an
 * opaque DEVICE buffer of cn_env_snapshot_bytes() bytes; cn_env_load only accepts a snapshot taken from a batch with the same
 * configuration, shape, seed and shard (first_env_index).  Both synchronise `stream` (they are not on the hot path). */
int64_t cn_env_snapshot_bytes(const cn_env_batch *env);
int cn_env_save(cn_env_batch *env, void *dst, void *stream);
int cn_env_load(cn_env_batch *env, const void *src, void *stream);

/* ---- rendering: n scenes -> n RGBA8 images in one launch ----
 * Replaces the drawing of the reference's render() (crowd_sim_pred.py:236-370, crowd_sim_var_num.py render) for the vec-env slot
 * render(mode='rgb_array') / get_images() (rl/vec_env/vec_env.py:121).  No matplotlib look: the image is DEFINED by the rule below, in fp32
 * with every operation rounded once and only + - *, comparisons and int -> float conversions per pixel, so a float32 restatement
 * reproduces every pixel.  All inputs are caller-owned device buffers, converted f64 -> f32 by round-to-nearest first:
 *   humans [n,H,8] and robot [n,8] in the layout of cn_env_get_state; counts [n] int32 humans present (the first counts[i] slots; NULL = H
 *   everywhere; slots at or beyond it are never read); visible [n,H] uint8, 1 = drawn as seen by the robot (NULL = all); robot_heading [n,2]
 *   float32 direction of the robot's heading mark, any length, 0,0 = none (NULL = the robot's velocity); dots [n,max_dots,2] float32 absolute
 *   positions with dot_counts [n] int32 (dots NULL = none; dot_counts NULL = max_dots everywhere), max_dots <= 1024; ring_radius <= 0 = no
 *   sensor ring; 16 <= size <= 1024, size % 4 == 0; out [n,size,size] RGBA8 words R | G<<8 | B<<16 | 255<<24, 16-byte aligned.
 * With S = size, L = half_width: pitch q = (2*L)/S; pixel (row i, col j) has centre x = (j + 0.5f)*q - L, y = L - (i + 0.5f)*q (row 0 is the
 * top).  For a shape centred at c: dx = x - cx, dy = y - cy, d2 = dx*dx + dy*dy.  w = 0.5f*q, hw = 0.75f*q, t = 1.5f*q.  Layers, later over
 * earlier:
 *   0 background white (255,255,255)
 *   1 sensor ring around the robot: lo = R - w, hi = R + w, d2 >= lo*lo && d2 <= hi*hi, grey (160,160,160)
 *   2 the robot's goal: |dx| + |dy| <= 0.3f, red (220,0,0)
 *   3 dots 0..dot_counts[i]-1: d2 <= 0.12f*0.12f, green (0,160,0)
 *   4 humans 0..counts[i]-1: outline d2 <= r*r && (r - t <= 0 || d2 >= (r-t)*(r-t)), blue (0,0,255) if visible else red (255,0,0); then the
 *     heading mark along the velocity v: s2 = vx*vx + vy*vy, none if s2 <= 1e-12f, dot = dx*vx + dy*vy, cr = dx*vy - dy*vx,
 *     dot >= 0 && dot*dot <= (r*r)*s2 && cr*cr <= (hw*hw)*s2, dark red (160,0,0)
 *   5 the robot: d2 <= rr*rr gold (255,215,0), then its heading mark by the same rule along robot_heading.
 * One launch, no atomics, no host synchronisation. */
int cn_render_scenes(int n, int H, const double *humans, const double *robot, const int32_t *counts, const uint8_t *visible,
                     const float *robot_heading, const float *dots, const int32_t *dot_counts, int max_dots, float robot_radius,
                     float ring_radius, int size, float half_width, uint32_t *out, void *stream);

/* ---- recorded episodes: metrics and the trajectory figure ----
 * Both read n traces in the layout of cn_env_trace_append (agents [n,cap,A,6] float32, flags [n,cap,A] uint8, length [n] int32; caller-owned
 * device buffers, 2 <= A <= CN_MAX_HUMANS + 1, 1 <= cap <= 65536) and use L = clamp(length, 0, cap) records of each.  They stand in for the
 * reference's test.py:31 --render_traj / rl/networks/envs.py:226 render_traj(path, episode_num), which forwards to an env method no env class
 * defines.  A trace ends with the state the final step was taken from (see cn_env_trace_append): neither pretends to know the state after it.
 * (CN_ABI_VERSION is unchanged: these are additions, no existing signature or struct layout moved.)
 *
 * cn_trace_metrics: out [n,CN_TRACE_METRICS] float64.  Positions, velocities and radii are widened to float64 first; every operation below is
 * a single correctly rounded fp64 operation (no contraction), norms are sqrt(x*x + y*y), and every sum runs over the records in ascending
 * order starting from 0.0 -- a rerun, or a loop in the same order elsewhere, gives the same bits.  A human slot is PRESENT in a record when
 * its flag bit 0 is set; its clearance there is ||p_robot - p_human|| - r_robot - r_human (the subtractions in that order).
 *   CN_TRACE_RECORDS                  L
 *   CN_TRACE_PATH_LENGTH              sum over t = 1..L-1 of ||p_robot[t] - p_robot[t-1]||: the L - 1 recorded segments, no jump to a next episode
 *   CN_TRACE_MIN_CLEARANCE            minimum clearance over all records and present humans; +inf if there is none
 *   CN_TRACE_INTRUSION_STEPS          records in which some present human has clearance < discomfort_dist
 *   CN_TRACE_VISIBLE_INTRUSION_STEPS  the same, counting only humans whose flag bit 1 (visible) is set
 *   CN_TRACE_MEAN_SPEED               (sum over t = 0..L-1 of ||v_robot[t]||) / L; 0 for L == 0
 *   CN_TRACE_MEAN_ACCEL               (sum over t = 1..L-1 of ||v_robot[t] - v_robot[t-1]||) / ((L-1) * time_step); 0 for L < 2
 *   CN_TRACE_MEAN_CROWD               (sum over t of the present humans of record t) / L; 0 for L == 0 */
enum { CN_TRACE_RECORDS = 0, CN_TRACE_PATH_LENGTH = 1, CN_TRACE_MIN_CLEARANCE = 2, CN_TRACE_INTRUSION_STEPS = 3,
       CN_TRACE_VISIBLE_INTRUSION_STEPS = 4, CN_TRACE_MEAN_SPEED = 5, CN_TRACE_MEAN_ACCEL = 6, CN_TRACE_MEAN_CROWD = 7, CN_TRACE_METRICS = 8 };
int cn_trace_metrics(int n, int cap, int A, const float *agents, const uint8_t *flags, const int32_t *length, double time_step,
                     double discomfort_dist, double *out, void *stream);
/* cn_render_trajectories: n recorded episodes -> n RGBA8 images in one launch, each episode as ONE picture.  Pixel grid, fp32 arithmetic
 * (every operation rounded once; only + - *, comparisons and int -> float conversions per pixel) and output format are those of
 * cn_render_scenes: S = size (16..1024, S % 4 == 0), L_w = half_width, q = (2*L_w)/S, pixel (row i, col j) has centre x = (j + 0.5f)*q - L_w,
 * y = L_w - (i + 0.5f)*q; for a mark centred at c: dx = x - cx, dy = y - cy, d2 = dx*dx + dy*dy; t = 1.5f*q.  goal [n,2] float32; stride >= 1;
 * out [n,S,S] RGBA8 words R | G<<8 | B<<16 | 255<<24, 16-byte aligned.  With L = clamp(length, 0, cap), D = max(L - 1, 1), the shade of
 * record k is s = (k*160)/D in integer arithmetic (0 for the first record, 160 for the last), and record k is a STAMP when k % stride == 0
 * or k == L - 1.  Three shapes of radius r (a record's radius field): TRAIL d2 <= (0.4f*r)*(0.4f*r); OUTLINE d2 <= r*r && (r - t <= 0 ||
 * d2 >= (r-t)*(r-t)); DISC d2 <= r*r.  Layers, later over earlier:
 *   0 background white (255,255,255)
 *   1 the goal: |dx| + |dy| <= 0.3f, red (220,0,0)
 *   2 humans: for k = 0..L-1, for slots a = 1..A-1 with flag bit 0 set, in that order: TRAIL, then on a stamp OUTLINE, both in
 *     (200-s, 200-s, 255) if flag bit 1 (visible) is set, else (255, 200-s, 200-s)
 *   3 the robot (slot 0, whatever its flag): for k = 0..L-1: TRAIL, then on a stamp OUTLINE, then for k == L - 1 DISC, all in (255, 215-s, 0).
 * L == 0 gives white plus the goal.  One launch, no atomics, no host synchronisation; n * ceil(S/32)^2 must stay below 2^24. */
int cn_render_trajectories(int n, int cap, int A, const float *agents, const uint8_t *flags, const int32_t *length, const float *goal,
                           int stride, int size, float half_width, uint32_t *out, void *stream);

/* Stand-alone batched ORCA solve (the rvo2 replacement): B independent agents, each with n_other neighbours.
 * self [B,8] = px,py,vx,vy,radius,max_speed,pref_vx,pref_vy ; others [B,n_other,5] = px,py,vx,vy,radius (float32);
 * out_vel [B,2].  n_other <= 63.  Parameters as PyRVOSimulator.addAgent. */
int cn_orca_solve(int B, int n_other, const float *self, const float *others, float neighbor_dist, int max_neighbors,
                  float time_horizon, float time_step, float *out_vel, void *stream);

/* ---- policy (selfAttn_merge_srnn + DiagGaussian head) ---- */
/* Device pointers to the fp32 parameters, named after the reference state_dict keys (model.py / SURVEY.md 8a-P0). */
typedef struct {
    const float *robot_linear_w, *robot_linear_b;                 /* base.robot_linear.0 [256,9] */
    const float *emb0_w, *emb0_b;                                 /* base.spatial_attn.embedding_layer.0 [128,D] */
    const float *emb2_w, *emb2_b;                                 /* base.spatial_attn.embedding_layer.2 [512,128] */
    const float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b;               /* base.spatial_attn.{q,k,v}_linear [512,512] */
    const float *in_proj_w, *in_proj_b;                           /* base.spatial_attn.multihead_attn.in_proj_* [1536,512] */
    const float *out_proj_w, *out_proj_b;                         /* ...multihead_attn.out_proj [512,512] */
    const float *spatial_linear_w, *spatial_linear_b;             /* base.spatial_linear.0 [256,512] */
    const float *attn_temporal_w, *attn_temporal_b;               /* base.attn.temporal_edge_layer.0 [64,256] */
    const float *attn_spatial_w, *attn_spatial_b;                 /* base.attn.spatial_edge_layer.0 [64,256] */
    const float *enc_w, *enc_b;                                   /* base.humanNodeRNN.encoder_linear [64,256] */
    const float *edge_embed_w, *edge_embed_b;                     /* base.humanNodeRNN.edge_attention_embed [64,256] */
    const float *gru_w_ih, *gru_w_hh, *gru_b_ih, *gru_b_hh;       /* base.humanNodeRNN.gru.* [384,128],[384,128],[384],[384] */
    const float *out_w, *out_b;                                   /* base.humanNodeRNN.output_linear [256,128] */
    const float *actor0_w, *actor0_b, *actor2_w, *actor2_b;       /* base.actor.{0,2} [256,256] */
    const float *critic0_w, *critic0_b, *critic2_w, *critic2_b;   /* base.critic.{0,2} [256,256] */
    const float *critic_linear_w, *critic_linear_b;               /* base.critic_linear [1,256] */
    const float *fc_mean_w, *fc_mean_b;                           /* dist.fc_mean [2,256] */
    const float *logstd;                                          /* dist.logstd._bias [2,1] */
} cn_policy_weights;

/* H humans, D = spatial edge width, max_envs = largest batch any later call will pass. */
int cn_policy_create(int human_num, int edge_width, int max_envs, cn_policy **out);
/* The four network-size flags of the reference (arguments.py:155-181): rnn_size R = human_node_rnn_size (GRU hidden size), embedding_size M =
 * human_node_embedding_size (encoder_linear, edge_attention_embed; the GRU input is 2M), attention_size A, output_size O =
 * human_node_output_size (output_linear, both trunks, the heads).  human_human_edge_rnn_size is not a dimension: the reference itself runs
 * with 256 only.  Device box: R in {64, 128, 192, 256}, M in {64, 128}, O a multiple of 64 in [64, 512], 1 <= A <= 256; anything else is
 * CN_ERR_INVALID.  The default is {128, 64, 64, 256}.  Under dims the tensors of cn_policy_weights have these shapes (the others keep theirs):
 *   attn_temporal_w / attn_spatial_w [A,256] (_b [A])     enc_w [M,256] (_b [M])      edge_embed_w [M,256] (_b [M])
 *   gru_w_ih [3R,2M]   gru_w_hh [3R,R]   gru_b_ih / gru_b_hh [3R]                     out_w [O,R] (_b [O])
 *   actor0 / actor2 / critic0 / critic2 _w [O,O] (_b [O])   critic_linear_w [1,O]     fc_mean_w [2,O]
 * and hxs_in / hxs_out are [E,R], the actor_feat tap [E,O] in cn_policy_act / cn_policy_get_value / cn_policy_get_taps.  A never reaches a kernel
 * as a dimension: it disappears in the fold u = Ws^T (Wt r + bt) and survives as the score scale (float)((double)H / sqrt((double)A)).
 * dims == NULL or the default tuple: the handle of cn_policy_create -- the same kernels, the same launches, the same bits.  Any other tuple:
 * gemm mode 2 runs the robot-node half on a kernel with run-time sizes (csrc/rn_sized.hip), modes 0 / 1 the separate launches with their
 * buffers and leading dimensions taken from dims; the human-human block in front of out_sp [rows,256] does not depend on dims. */
typedef struct { int rnn_size, embedding_size, attention_size, output_size; } cn_policy_dims;
int cn_policy_create_sized(int human_num, int edge_width, int max_envs, const cn_policy_dims *dims, cn_policy **out);
int cn_policy_destroy(cn_policy *p);
/* Snapshot the weights (copies + pre-folds the affine pairs q/k/v_linear∘in_proj and out_proj∘spatial_linear).
 * Call again after every optimiser step that changed them. */
int cn_policy_set_weights(cn_policy *p, const cn_policy_weights *w, void *stream);
/* One rollout-time forward for E envs.  hxs_in/out [E,128] (human_node_rnn; [E,R] under cn_policy_dims), masks [E,1].  eps [E,2] standard-normal
 * noise or NULL for the deterministic mode() action.  Outputs value [E,1], action [E,2], logp [E,1]. */
int cn_policy_act(cn_policy *p, int E, const cn_obs *obs, const float *hxs_in, const float *masks, const float *eps,
                  float *value, float *action, float *logp, float *hxs_out, void *stream);
int cn_policy_get_value(cn_policy *p, int E, const cn_obs *obs, const float *hxs_in, const float *masks, float *value,
                        void *stream);
/* Test taps of the last act/get_value call: hh_out [E,H,512] is not materialised by the folded pipeline, so the taps
 * are spatial_lin [E,H,256], hr_attn [E,H], hr_out [E,256], robot_emb [E,256], actor_feat [E,256] ([E,O] under cn_policy_dims) (NULL to skip). */
int cn_policy_get_taps(cn_policy *p, int E, float *spatial_lin, float *hr_attn, float *hr_out, float *robot_emb,
                       float *actor_feat, void *stream);
/* Fused mode (cn_policy_set_gemm_mode 2): the robot-node kernel writes the taps above only while they are enabled (default 1);
 * rollout loops switch them off (17 MB of stores per 4096-env forward that nothing reads). */
int cn_policy_set_taps(cn_policy *p, int enabled);
/* fn(arg, stream) is called by cn_policy_act / cn_policy_get_value (fused mode) right after the human-human kernel was enqueued on `stream` and
 * before the robot-node kernel: the place for side work that must not reach the CUs before that kernel -- see cn_env_set_tail_deferral; pass
 * fn = (int (*)(void *, void *))cn_env_launch_tail and arg = the env batch.  A non-zero return aborts the forward with that status.  fn = NULL
 * removes the hook (do so before destroying what `arg` points to). */
int cn_policy_set_post_hh_hook(cn_policy *p, int (*fn)(void *arg, void *stream), void *arg);
/* Arithmetic of the three large human-human GEMMs (embedding_layer.2, folded q|k|v, folded out_proj∘spatial_linear):
 *   2 (default) = split precision (each fp32 operand as bf16 hi + lo, three bf16 MFMAs per term, fp32 accumulation; products
 *                 exact to ~2^-16 relative; outputs within 2e-5 of the fp32 path, bar 1e-4) with the whole human-human block as ONE
 *                 persistent kernel (activations never leave LDS / registers) and everything after it as ONE robot-node kernel;
 *   1           = the same split-precision arithmetic as separate launches (embedding / q|k|v / out_proj GEMMs, attention kernels,
 *                 per-env GEMMs);
 *   0           = exact fp32 on v_mfma_f32_32x32x2_f32, separate launches.
 * Everything outside the three large GEMMs always runs in exact fp32. */
int cn_policy_set_gemm_mode(cn_policy *p, int mode);
/* args.use_self_attn (arguments.py:189; selfAttn_srnn_temp_node.py:340-345, :402-414).  enabled = 1 (default): the human-human block is
 * SpatialEdgeSelfAttn + spatial_linear.  enabled = 0: no human-human attention -- spatial_linear is Sequential(Linear(D, 128), ReLU,
 * Linear(128, 256), ReLU) applied to the spatial edges themselves; cn_policy_set_weights then reads
 *   emb0_w / emb0_b               = base.spatial_linear.0 [128,D]
 *   spatial_linear_w / _b         = base.spatial_linear.2 [256,128]
 * and ignores emb2_*, q_*, k_*, v_*, in_proj_*, out_proj_* (they may be NULL).  Call before cn_policy_set_weights; changing it
 * invalidates the weight snapshot.  The robot-node part (robot-human attention, GRU, heads) is the same in both variants. */
int cn_policy_set_self_attention(cn_policy *p, int enabled);
/* args.sort_humans = False (arguments.py:206; selfAttn_srnn_temp_node.py:378-383, :402-414): the observation's humans are NOT sorted by
 * distance and both attention modules mask by `visible_masks` instead of by the detected count (all-invisible samples keep human 0).  Both
 * modules are permutation-equivariant over the humans and masked humans contribute exactly nothing, so the masked form equals the counted
 * form on the observation with the visible humans moved to the front (stable), which is what this entry point produces:
 *   spatial_edges [B,H,D], visible_masks [B,H] (bytes, non-zero = visible)  ->  out_edges [B,H,D] (visible rows first, the others behind
 *   them, each group in index order), out_detected [B] (float: max(1, number visible))
 * feed those to cn_policy_act / cn_hh_block_fwd / cn_rn_seq_fwd in place of the raw observation.  One wavefront per sample, H <= 64. */
int cn_obs_compact_visible(int B, int H, int D, const float *spatial_edges, const uint8_t *visible_masks, float *out_edges, float *out_detected,
                           void *stream);
/* Dominant-kernel timing support for bench.py: `every` = 0 switches it off, n >= 1 brackets every n-th forward's dominant kernel
 * (the fused human-human kernel, or the QKV projection of the separate-launch modes) with a pair of hipEvents on `stream`;
 * cn_policy_get_profile returns the accumulated device time [0], the bracketed launches [0] and their live rows [1].  An event
 * record costs a few microseconds of dispatch gap on the stream it sits on, hence the stride. */
int cn_policy_set_profiling(cn_policy *p, int every);
int cn_policy_get_profile(cn_policy *p, double *ms_out /*[8]*/, int64_t *launches_out /*[8]*/);
/* The same brackets one by one (bench.py reports their median / min / max): copies up to `cap` per-launch durations [ms], oldest first,
 * into ms_out (host memory) and returns how many there are (waits for the brackets still in flight); cn_policy_reset_profile drops
 * the samples and the sums but keeps the stride -- the events stay warm (a timing event's first record on a queue switches the
 * queue's profiling on, a one-off cost of some hundred microseconds that must not fall into a timed window). */
int cn_policy_get_profile_samples(cn_policy *p, float *ms_out, int cap);
int cn_policy_reset_profile(cn_policy *p);

/* ---- DS-RNN baseline policy (base='srnn': rl/networks/srnn_model.py + DiagGaussian head) ----
 * The network every table of the paper compares against (config.py robot.policy: "For baseline: srnn").  Unlike the attention-graph
 * network its edge state is LIVE: two edge GRUs (one temporal edge, H spatial edges, hidden 256) carry `human_human_edge_rnn`
 * [E,H+1,256], slot 0 the temporal edge, from step to step; the attention runs over ALL H slots, padded humans included
 * (detected_human_num and visible_masks are not read).  Only the `args.env_type == 'crowd_sim'` branch of srnn_model.py:378 (robot node
 * width 7) exists here.  A forward is two launches whatever E and H: the edge-GRU kernel and the node kernel.
 * Device pointers to the fp32 parameters, named after the reference state_dict keys; the three modules that never reach the output
 * (base.humanNodeRNN.edge_embed, base.human_node_final_linear, base.spatial_linear) are not in it. */
typedef struct {
    const float *enc_s_w, *enc_s_b;                               /* base.humanhumanEdgeRNN_spatial.encoder_linear [64,D] */
    const float *gru_s_w_ih, *gru_s_w_hh, *gru_s_b_ih, *gru_s_b_hh; /* base.humanhumanEdgeRNN_spatial.gru.* [768,64],[768,256],[768],[768] */
    const float *enc_t_w, *enc_t_b;                               /* base.humanhumanEdgeRNN_temporal.encoder_linear [64,2] */
    const float *gru_t_w_ih, *gru_t_w_hh, *gru_t_b_ih, *gru_t_b_hh; /* base.humanhumanEdgeRNN_temporal.gru.* */
    const float *attn_temporal_w, *attn_temporal_b;               /* base.attn.temporal_edge_layer.0 [64,256] */
    const float *attn_spatial_w, *attn_spatial_b;                 /* base.attn.spatial_edge_layer.0 [64,256] */
    const float *node_enc_w, *node_enc_b;                         /* base.humanNodeRNN.encoder_linear [64,3] */
    const float *edge_embed_w, *edge_embed_b;                     /* base.humanNodeRNN.edge_attention_embed [64,512] */
    const float *node_gru_w_ih, *node_gru_w_hh, *node_gru_b_ih, *node_gru_b_hh; /* base.humanNodeRNN.gru.* [384,128] x 2, [384] x 2 */
    const float *out_w, *out_b;                                   /* base.humanNodeRNN.output_linear [256,128] */
    const float *actor0_w, *actor0_b, *actor2_w, *actor2_b;       /* base.actor.{0,2} [256,256] */
    const float *critic0_w, *critic0_b, *critic2_w, *critic2_b;   /* base.critic.{0,2} [256,256] */
    const float *critic_linear_w, *critic_linear_b;               /* base.critic_linear [1,256] */
    const float *robot_linear_w, *robot_linear_b;                 /* base.robot_linear [3,7] */
    const float *fc_mean_w, *fc_mean_b;                           /* dist.fc_mean [2,256] */
    const float *logstd;                                          /* dist.logstd._bias [2,1] */
} cn_srnn_weights;
typedef struct cn_srnn cn_srnn;

/* 1 <= human_num <= CN_MAX_HUMANS; edge_width = whatever the env gives (2 for CrowdSimVarNum-v0, 12 for the Pred envs); max_envs = the
 * largest batch any later call will pass.  No CPU fallback: CN_ERR_NO_DEVICE without a gfx950 device. */
int cn_srnn_create(int human_num, int edge_width, int max_envs, cn_srnn **out);
int cn_srnn_destroy(cn_srnn *p);
/* Snapshot the weights (copies them, splits the two edge GRUs' W_hh into bf16 hi / lo planes).  Call again after every optimiser step. */
int cn_srnn_set_weights(cn_srnn *p, const cn_srnn_weights *w, void *stream);
/* One rollout-time forward for E envs (srnn_model.py:389-468 with infer=True, then model.py:64-71).  Reads obs->robot_node,
 * obs->temporal_edges and obs->spatial_edges only.  node_hxs_in/out [E,128], edge_hxs_in/out [E,H+1,256], masks [E,1] (both states are
 * multiplied by it first, as RNNBase._forward_gru does), eps [E,2] standard-normal noise or NULL for the deterministic mode() action.
 * Outputs value [E,1], action [E,2], logp [E,1].  edge_hxs_out MAY be edge_hxs_in itself (exactly the same pointer, not a partial overlap)
 * and node_hxs_out may be node_hxs_in: every workgroup reads its own rows before it writes them.  The rollout passes two storage rows. */
int cn_srnn_act(cn_srnn *p, int E, const cn_obs *obs, const float *node_hxs_in, const float *edge_hxs_in, const float *masks, const float *eps,
                float *value, float *action, float *logp, float *node_hxs_out, float *edge_hxs_out, void *stream);
/* The bits of cn_srnn_act's `value` (the same two kernels; the new edge state goes to a buffer of the handle, allocated by the first call). */
int cn_srnn_get_value(cn_srnn *p, int E, const cn_obs *obs, const float *node_hxs_in, const float *edge_hxs_in, const float *masks, float *value,
                      void *stream);
/* Test taps of the last act / get_value call (NULL skips one): edge_out [E,H+1,256] (copied from where that call wrote it: the caller's
 * edge_hxs_out must still hold it), attn [E,H] (softmax over all H slots), weighted [E,256], node_out [E,256] (output_linear),
 * actor_feat [E,256]. */
int cn_srnn_get_taps(cn_srnn *p, int E, float *edge_out, float *attn, float *weighted, float *node_out, float *actor_feat, void *stream);
/* Arithmetic of the edge GRUs' recurrent product ([rows, 256] x W_hh^T, 4/5 of the edge-GRU FLOPs):
 *   1 (default) = split precision (each fp32 operand as bf16 hi + lo, lo*hi + hi*lo + hi*hi on v_mfma_f32_16x16x32_bf16, fp32 accumulation;
 *                 outputs within 1e-4 of the reference, the project's bar);
 *   0           = exact fp32 on v_mfma_f32_16x16x4_f32.
 * The input-side product ([rows, 64] x W_ih^T) is exact fp32 MFMA in BOTH modes: its operand, the edge embedding, is not bounded (unseen
 * humans are padded with 15 m, embeddings reach 10 .. 30) and as a split product it alone was 1.1e-4 off the reference.  Everything else
 * (encoders, gates, attention, node GRU, trunks, heads) always runs in fp32. */
int cn_srnn_set_gemm_mode(cn_srnn *p, int mode);

/* ---- DS-RNN baseline: the edge-GRU sequence of PPO.update (srnn_model.py:418-433 over a T-step minibatch) and its backward ----
 * For t = 0 .. T-1 both edge GRUs compute h_t = GRU(ReLU(enc x_t), mask_t * h_{t-1}) with the kernel and the arithmetic of cn_srnn_act
 * (rows gathered per weight set, one launch per step, the handle's weight snapshot, split planes and gemm mode: call cn_srnn_set_weights
 * after every optimiser step).  No atomics on data, fixed summation orders, equal arguments give equal bits, and a row's h does not depend
 * on which rows share its tile.  temporal_edges [T,N,2], spatial_edges [T,N,H,D], edge_h0 [N,H+1,256], masks [T,N], h_all [T,N,H+1,256].
 *
 * workspace: cn_srnn_seq_workspace_bytes(T, N, H, D) bytes.  The forward leaves the gates r, z, n and W_hn (mask * h) + b_hn and the 64-wide
 * post-ReLU embedding of every row and step there; the backward overwrites the gates IN PLACE with dr, dz, dn, dn * r (what the weight
 * gradients are summed from) and adds d_e and one [N,H+1,256] carry.  The function runs on the host and needs no device; it returns 0 for a
 * shape the kernels refuse: H outside [1,64], D outside [1,64], T < 1, N < 1, or T * N * (H+1) * 1024 saved floats past 32-bit element
 * offsets.  workspace_bytes is what the caller allocated (checked against the shape).
 *
 * cn_srnn_seq_bwd: d_h_all [T,N,H+1,256] is the gradient of h_all (read only).  BPTT for t = T-1 .. 0, one launch per step, then the weight
 * gradients of each set as sums over all its rows and steps: the rows are cut into at most CN_SRNN_SEQ_CHUNKS ranges whose partial products
 * land in `partials` (CN_SRNN_SEQ_PARTIALS_BYTES bytes, whatever the shape) and are added in range order.  grads: the twelve gradients, in
 * cn_srnn_weights field order for the two edge RNNs, each OVERWRITTEN.  d_edge_h0 [N,H+1,256] (the carry of step -1) may be NULL. */
typedef struct {
    float *enc_s_w, *enc_s_b, *gru_s_w_ih, *gru_s_w_hh, *gru_s_b_ih, *gru_s_b_hh;
    float *enc_t_w, *enc_t_b, *gru_t_w_ih, *gru_t_w_hh, *gru_t_b_ih, *gru_t_b_hh;
} cn_srnn_edge_grads;
#define CN_SRNN_SEQ_CHUNKS 64
#define CN_SRNN_SEQ_PARTIALS_BYTES ((int64_t)CN_SRNN_SEQ_CHUNKS * (768 * 256 + 1024 * 80 + 64 * 80) * 4)
int64_t cn_srnn_seq_workspace_bytes(int T, int N, int H, int D);
int cn_srnn_seq_fwd(cn_srnn *p, int T, int N, const float *temporal_edges, const float *spatial_edges, const float *edge_h0, const float *masks,
                    float *h_all, void *workspace, int64_t workspace_bytes, void *stream);
int cn_srnn_seq_bwd(cn_srnn *p, int T, int N, const float *temporal_edges, const float *spatial_edges, const float *edge_h0, const float *masks,
                    const float *h_all, const float *d_h_all, void *workspace, int64_t workspace_bytes, const cn_srnn_edge_grads *grads,
                    float *d_edge_h0, void *partials, void *stream);

/* ---- DS-RNN baseline: the edge attention of PPO.update (EdgeAttention, srnn_model.py:256-323, over the saved edge states) and its backward ----
 * h_all [B, H+1, 256] (B = T*N samples, read in place: slot 0 the temporal edge t, slots 1 .. H the spatial edges s_j), Wt / Ws [64,256] the
 * temporal_edge_layer / spatial_edge_layer weights, bt [64].  Per sample
 *   te = Wt t + bt;  u = Ws^T te;  score_j = (H / 8) (u . s_j);  a = softmax_j(score) over all H slots, no mask;  weighted = sum_j a_j s_j
 * which is the reference's te . (Ws s_j + bs) without the term te . bs, the same for every j: the softmax does not see it, so the bias of
 * spatial_edge_layer is no argument and its gradient is exactly zero.  No [B,H,64] or [B,H,256] temporary exists: the forward reads h_all once,
 * the backward reads it once and writes d_h_all once.  Plain fp32, one wavefront per sample, fixed summation orders, no atomics: equal
 * arguments give equal bits, and a sample's outputs do not depend on B or on the other samples.  No workspace.
 *
 * cn_srnn_attn_fwd writes weighted [B,256], attn [B,H] and, for the backward, te [B,64] and u [B,256].
 * cn_srnn_attn_bwd takes d_weighted [B,256] and d_t_direct [B,256] (a gradient that reaches t by another route; may be NULL) and writes
 * every element of d_h_all [B,H+1,256] exactly once (nothing to zero beforehand): slot 0 = Wt^T d_te + d_t_direct, slot 1 + j =
 * a_j d_weighted + (H / 8) d_score_j u; plus d_u [B,256] and d_te [B,64], from which the caller sums the weight gradients over the B rows
 * (dWs = te^T d_u, dWt = d_te^T t, dbt = column sums of d_te: cn_linear_wgrad at N = 64, K = 256, t read in place with ldx = (H+1) * 256).
 * Box: 1 <= H <= CN_MAX_HUMANS, B >= 1, edge width 256, attention size 64, the [.,256] operands 16-byte aligned; outside it CN_ERR_INVALID
 * naming the call, and nothing is launched.  (CN_ABI_VERSION is unchanged: these are additions, no existing signature or struct layout moved.) */
int cn_srnn_attn_fwd(int B, int H, const float *h_all, const float *Wt, const float *bt, const float *Ws, float *weighted, float *attn, float *te,
                     float *u, void *stream);
int cn_srnn_attn_bwd(int B, int H, const float *h_all, const float *Wt, const float *Ws, const float *attn, const float *u, const float *d_weighted,
                     const float *d_t_direct, float *d_h_all, float *d_u, float *d_te, void *stream);

/* ---- device-side launch stamps (measurement aid for bench.py / tools; not part of the reference's interface) ----
 * The kernels of the rollout step (CN_PROF_K_*) stamp the device's 100 MHz wall clock when their first workgroups start and when their
 * wavefronts end, into a caller-owned DEVICE ring of steps x CN_PROF_KERNELS slots of CN_PROF_SLOT_WORDS uint64.  A slot is 2 x 64
 * sub-slots of 16 words (one cache line each: same-address atomics serialise): word 16 b of the first half is a candidate for the
 * start (the minimum counts; initialise the slot's first half to all ones), word 16 (64 + b) one for the end (the maximum counts;
 * initialise to 0); word 1 of the slot carries a per-kernel count (the human-human kernel's live rows; initialise to 0).  Unlike an event
 * bracket on the stream the stamps cost no dispatch gap and do not include the time a launch waits for the host, and because the
 * clock is global the slots of a step also give its timeline.  cn_prof_set_stamps installs the ring for the whole process (NULL, 0
 * removes it) with a bit mask of the kernels to stamp; cn_prof_next_step moves to the next row (the first call selects row 0; rows
 * beyond `steps` are not stamped) and returns the row index.  Host-side state: call both from the thread that enqueues the step. */
enum { CN_PROF_K_ENV_STEP = 0, CN_PROF_K_ORCA_LANE = 1, CN_PROF_K_HH_FUSED = 2, CN_PROF_K_RN_FUSED = 3, CN_PROF_K_ORCA_LP3 = 4, CN_PROF_K_PREGEN = 5,
       CN_PROF_K_ROW_PLAN = 6, CN_PROF_K_OTHER = 7, CN_PROF_KERNELS = 8, CN_PROF_SLOT_WORDS = 2048 };
int cn_prof_set_stamps(uint64_t *ring, int steps, unsigned kernel_mask);
int cn_prof_next_step(void);

/* ---- the human-human block of evaluate_actions' forward as ONE launch (training path; crowds of <= 48 humans) ----
 * rl/networks/selfAttn_srnn_temp_node.py:63-91 + :408 on the compacted live rows, i.e. what cn_embed0_fwd -> cn_linear_fwd (embedding_layer.2,
 * ReLU) -> cn_linear_fwd (folded q|k|v) -> cn_hh_attention_fwd -> cn_linear_fwd (folded out_proj∘spatial_linear, ReLU) compute in five
 * launches with every activation passing through HBM twice; here the rollout's fused kernel runs on the training weights and writes each
 * activation the backward kernels need exactly once: e0 [R,128], x [R,512] (both post-ReLU), qkv [R,1536] (q unscaled; q_scale = 0.125
 * multiplies the scores), attn [R,512], out_sp [R,256] (post-ReLU).  spatial_edges [B,H,D] dense, row_off [B+1] (exclusive prefix of the
 * detected humans, R = row_off[B]); weights fp32 row-major ([512,128], [1536,512], [256,512]; biases 16-byte aligned); workspace =
 * cn_hh_block_workspace_bytes() bytes for the fragment-ordered bf16 hi/lo images, rebuilt on every call (the weights change every
 * optimiser step).  Same bf16x3 arithmetic as cn_linear_fwd.  The backward is the existing per-layer kernels on these outputs. */
int64_t cn_hh_block_workspace_bytes(void);
int cn_hh_block_fwd(int B, int H, int D, const float *spatial_edges, const int *row_off, const float *emb0_w, const float *emb0_b,
                    const float *emb2_w, const float *emb2_b, const float *qkv_w, const float *qkv_b, const float *os_w, const float *os_b,
                    float q_scale, void *workspace, float *e0, float *x, float *qkv, float *attn, float *out_sp, void *stream);

/* ---- the robot-node sequence of evaluate_actions' forward and backward as ONE call each (training path) ----
 * Everything behind the human-human block in rl/networks/model.py:82-90 -> selfAttn_srnn_temp_node.py:395-449 + srnn_model.py:35-105 +
 * distributions.py:36-44 for a [T, N] rollout slice (B = T * N samples, T-major): robot_linear -> [u | encoder_linear] -> robot-human attention over
 * the compacted out_sp rows -> edge_attention_embed -> GRU over the T steps with the done mask -> actor / critic trunks -> critic_linear and the
 * log-probability of the GIVEN actions under the DiagGaussian head.  Together with cn_hh_block_fwd (+ the per-layer backward kernels) this is
 * the train-mode policy forward of the boundary: no library GEMM and no framework pointwise kernel is left between the observation and
 * (value, log-prob).  Weights are the fp32 training weights as the host composes them (two affine pairs folded by the caller, whose autograd
 * carries the gradients of the folded matrices back to the factors): te = [spatial_edge_layer^T temporal_edge_layer ; encoder_linear],
 * ac0 = (actor.0 ; critic.0) o output_linear.  bf16x3 split-precision products (cn_linear_fwd_act) forward and for dX -- edge_attention_embed's
 * 64-output forward on the exact-fp32 kernel --, bf16x3 split-K for the weight gradients.
 * cn_rn_seq_fwd writes every activation the backward needs into the caller's `saved` buffers; cn_rn_seq_bwd takes d_value / d_logp [B] and
 * returns d_out_sp [R,256] (gradient into the human-human block), d_h0 [N,128] and the gradient of every weight (fixed summation orders). */
typedef struct {
    const float *rl_w, *rl_b;               /* robot_linear.0 [256,9], [256] */
    const float *te_w, *te_b;               /* [320,256], [320]: rows 0..255 u = Ws^T (Wt . + bt), rows 256..319 encoder_linear */
    const float *edge_w, *edge_b;           /* edge_attention_embed [64,256], [64] */
    const float *wih, *bih, *whh, *bhh;     /* GRU [384,128], [384] */
    const float *ac0_w, *ac0_b;             /* [512,128], [512]: (actor.0 ; critic.0) o output_linear */
    const float *a2_w, *a2_b, *c2_w, *c2_b; /* actor.2, critic.2 [256,256], [256] */
    const float *cl_w, *cl_b, *fm_w, *fm_b, *logstd; /* critic_linear [1,256],[1]; dist.fc_mean [2,256],[2]; dist.logstd [2] */
} cn_rn_weights;
typedef struct { /* gradients, same shapes as cn_rn_weights (device buffers, overwritten) */
    float *rl_w, *rl_b, *te_w, *te_b, *edge_w, *edge_b, *wih, *bih, *whh, *bhh, *ac0_w, *ac0_b, *a2_w, *a2_b, *c2_w, *c2_b, *cl_w, *cl_b, *fm_w, *fm_b, *logstd;
} cn_rn_grads;
typedef struct { /* activations kept for the backward (device buffers of the caller) */
    float *rs;    /* [B,256] relu(robot_linear) */
    float *z;     /* [B,384] u (256) | relu(enc) (64) | relu(edge) (64) */
    float *hr;    /* [B,256] attended human features */
    float *attn;  /* [B,H]   robot-human attention weights */
    float *gi;    /* [B,384] x W_ih^T + b_ih */
    float *hs;    /* [B,128] GRU outputs (hs[(T-1) N ..] is the final hidden state) */
    float *hms;   /* [B,128] masked previous states */
    float *gates; /* [B,512] r, z, n, gh_n */
    float *a1;    /* [B,512] tanh of the first trunk layers (actor | critic) */
    float *a2;    /* [B,512] tanh of the second trunk layers (actor | critic) */
} cn_rn_saved;
int64_t cn_rn_seq_workspace_floats(int T, int N);   /* scratch of cn_rn_seq_bwd */
int64_t cn_rn_seq_fwd_workspace_floats(void);       /* scratch of cn_rn_seq_fwd (the split planes of this step's weights) */
int cn_rn_seq_fwd(int T, int N, int H, const float *robot_node /*[B,7]*/, const float *temporal_edges /*[B,2]*/, const float *out_sp /*[R,256]*/,
                  const int *row_off /*[B+1]*/, const float *h0 /*[N,128]*/, const float *masks /*[B]*/, const float *actions /*[B,2]*/,
                  const cn_rn_weights *w, const cn_rn_saved *saved, float *workspace, float *value /*[B]*/, float *logp /*[B]*/, void *stream);
int cn_rn_seq_bwd(int T, int N, int H, const float *robot_node, const float *temporal_edges, const float *out_sp, const int *row_off, const float *masks,
                  const float *actions, const cn_rn_weights *w, const cn_rn_saved *saved, const float *d_value /*[B]*/, const float *d_logp /*[B]*/,
                  float *workspace, float *d_out_sp /*[R,256]*/, float *d_h0 /*[N,128]*/, const cn_rn_grads *grads, void *stream);
/* The same sequence at the network sizes of cn_policy_dims (R, M, A, O) inside the device box of cn_policy_create_sized; outside it every
 * *_sized call below fails with CN_ERR_INVALID naming the box (the two workspace functions, which run on the host, return 0) and launches
 * nothing.  dims == NULL or the default tuple: cn_rn_seq_fwd / cn_rn_seq_bwd themselves (they forward here) -- the same launches on the same
 * buffers, the same bits.  The edge width stays 256.  Layouts under dims:
 *   cn_rn_weights / cn_rn_grads:  rl_w [256,9]   te_w [256+M,256] (rows 0..255 u, rows 256.. encoder_linear; te_b [256+M])   edge_w [M,256]
 *                                 wih [3R,2M]    whh [3R,R] (bih / bhh [3R])   ac0_w [2O,R] (ac0_b [2O])   a2_w / c2_w [O,O] (_b [O])
 *                                 cl_w [1,O]     fm_w [2,O]    cl_b [1], fm_b [2], logstd [2] as before
 *   cn_rn_saved:                  rs [B,256]   z [B,256+2M] = u (256) | relu(enc) (M) | relu(edge) (M)   hr [B,256]   attn [B,H]   gi [B,3R]
 *                                 hs / hms [B,R]   gates [B,4R]   a1 / a2 [B,2O]
 *   h0 / d_h0 [N,R]; every buffer is dense: NO leading dimension is padded.
 * A appears only in the caller's fold u = Ws^T (Wt r + bt) and in the score temperature (float)((double)H / sqrt((double)A)), which both
 * robot-human attention kernels take from here (H / 8 at A = 64).
 * Products whose output width is not a multiple of 128 (3R at R = 64 / 192, O at O = 64 (2 a + 1), R at R = 64 / 192, 256 + M at M = 64) run on
 * weight planes zero-padded to the next multiple of 128 with a GUARDED STORE: the wavefronts that own the surplus 64 columns compute and store
 * nothing (cn_linear_fwd_act's kernel), so no output row is written past its real columns and no bias is read past its end.  Weight gradients
 * whose reduction-side width K is 64 (2 a + 1) (K = R for whh / ac0, K = O for a2 / c2) run on the two-barrier split-K kernel with a half-empty
 * last X tile; the split count depends on the shape alone (cn_linear_wgrad_splits), so the summation order is fixed.
 * The GRU runs on cn_gru_seq_fwd_sized / cn_gru_seq_bwd_sized (below). */
int64_t cn_rn_seq_workspace_floats_sized(int T, int N, const cn_policy_dims *dims);
int64_t cn_rn_seq_fwd_workspace_floats_sized(const cn_policy_dims *dims);
int cn_rn_seq_fwd_sized(int T, int N, int H, const float *robot_node, const float *temporal_edges, const float *out_sp, const int *row_off, const float *h0,
                        const float *masks, const float *actions, const cn_rn_weights *w, const cn_rn_saved *saved, float *workspace, float *value,
                        float *logp, const cn_policy_dims *dims, void *stream);
int cn_rn_seq_bwd_sized(int T, int N, int H, const float *robot_node, const float *temporal_edges, const float *out_sp, const int *row_off,
                        const float *masks, const float *actions, const cn_rn_weights *w, const cn_rn_saved *saved, const float *d_value,
                        const float *d_logp, float *workspace, float *d_out_sp, float *d_h0, const cn_rn_grads *grads, const cn_policy_dims *dims,
                        void *stream);
/* cn_gru_seq_fwd / cn_gru_seq_bwd at a hidden size R in {64, 128, 192, 256}: gi / dgi / dgh [T,N,3R], h0 / dh0 [N,R], hs / hms / d_hs [T,N,R],
 * gates [T,N,4R], w_hh [3R,R].  One kernel pair for every R (csrc/gru_seq.h).  R = 64 and 128 read w_hh itself, split it into bf16 hi / lo MFMA
 * fragments in registers and keep them there for the whole sequence: workspace is unused and may be NULL.  R = 192 and 256 need a workspace of
 * 3 R^2 floats: the call first writes W_hh there as fragments, which the sequence kernel re-reads from the L2 every step (the slice of a
 * wavefront would need 432 / 768 of its 512 registers).  16 rows per workgroup, fixed summation order. */
int cn_gru_seq_fwd_sized(int T, int N, int R, const float *gi, const float *h0, const float *masks, const float *w_hh, const float *b_hh, float *hs,
                         float *hms, float *gates, float *workspace, void *stream);
int cn_gru_seq_bwd_sized(int T, int N, int R, const float *gates, const float *hms, const float *masks, const float *w_hh, const float *d_hs,
                         float *dgi, float *dgh, float *dh0, float *workspace, void *stream);

/* ---- human-human attention core, stand-alone (training path) ----
 * The (env, head) units of torch.nn.MultiheadAttention's scaled-dot-product core (selfAttn_srnn_temp_node.py:89) on COMPACTED
 * rows: sample b owns rows row_off[b] .. row_off[b+1]-1 (its detected humans); qkv [R,1536] = [q | k | v] (8 heads x 64).
 * fwd: out [R,512] = softmax(scale * q k^T) v per unit.  bwd: d_qkv [R,1536] from d_out [R,512] (softmax recomputed). */
/* cls: device workspace of cn_hh_attention_workspace_ints(B) int32 holding the size-class lists of the samples (<= 8 / 16 / 32 / 64 live
 * humans): each class is one launch that walks only its own (sample, head) units with an LDS footprint sized for it.  The forward builds
 * the lists when cls != NULL (NULL: every launch inspects every unit); the backward needs the buffer and rebuilds the lists unless
 * cls_ready != 0 (= the buffer was filled by the forward call on the same row_off). */
int64_t cn_hh_attention_workspace_ints(int B);
int cn_hh_attention_fwd(int B, int H, const float *qkv, const int *row_off, float scale, float *out, int *cls, void *stream);
int cn_hh_attention_bwd(int B, int H, const float *qkv, const int *row_off, const float *d_out, float scale, float *d_qkv, int *cls, int cls_ready,
                        void *stream);

/* ---- robot-human attention, stand-alone (training path) ----
 * EdgeAttention_M.att_func (rl/networks/selfAttn_srnn_temp_node.py:145-177) on COMPACTED rows: sample b owns rows
 * row_off[b] .. row_off[b+1]-1 of out_sp [R,256] (the attended values).  The reference scores t . s_j with
 * t = temporal_edge_layer(robot) and s_j = spatial_edge_layer(out_sp_j) = Ws out_sp_j + bs equal (Ws^T t) . out_sp_j up
 * to a per-sample constant the softmax ignores, so the op takes u [B,256] = Ws^T t instead of t and s.
 * fwd: attn [B,H] = softmax((H / 8) u . out_sp_j) (zero on padded humans), hr_out [B,256] = sum_j attn_j out_sp_j.
 * bwd: d_u [B,256] and d_o [R,256] from d_hr [B,256]. */
int cn_hr_attention_fwd(int B, int H, const float *u, const float *out_sp, const int *row_off, float *hr_out, float *attn,
                        void *stream);
int cn_hr_attention_bwd(int B, int H, const float *u, const float *out_sp, const int *row_off, const float *attn,
                        const float *d_hr, float *d_u, float *d_o, void *stream);

/* ---- embedding_layer.0 of the human-human block (training path) ----
 * Linear(D -> 128) + ReLU on the compacted rows (rl/networks/selfAttn_srnn_temp_node.py:33-36), D = 2 (VarNum) or 12
 * (Pred envs).  fwd: y [R,128] = relu(x [R,D] W^T + b).  bwd: dWb [128, D+1] = per output column the D weight
 * gradients followed by the bias gradient, from dy [R,128] masked by y > 0; `blocks` row-strided partial sums land in
 * partials [blocks,128,D+1] and are reduced in block order (deterministic).  The inputs are observations: no dx. */
int cn_embed0_fwd(int R, int D, const float *x, const float *W, const float *b, float *y, void *stream);
int cn_embed0_bwd(int R, int D, const float *x, const float *y, const float *dy, int blocks, float *partials, float *dWb,
                  void *stream);

/* ---- GRU of the human node RNN over a whole sequence (training path) ----
 * torch.nn.GRU (gate order r,z,n) as EndRNN drives it one step at a time with h * done-mask
 * (rl/networks/srnn_model.py:35-105, selfAttn_srnn_temp_node.py:262-285), under autograd in PPO.update: one launch per direction,
 * W_hh resident in registers, one workgroup per 16 rows (cn_gru_seq_fwd_sized / _bwd_sized at R = 128, no workspace).
 * gi [T,N,384] = x W_ih^T + b_ih, h0 [N,128], masks [T,N] -> hs [T,N,128]; hms [T,N,128] (masked previous states) and
 * gates [T,N,512] = (r, z, n, gh_n) are kept for the backward.  bwd: d_hs [T,N,128] -> dgi [T,N,384], dgh [T,N,384] (the caller forms
 * d(W_hh) = dgh^T hms and d(b_hh) = column sums of dgh) and dh0 [N,128]. */
int cn_gru_seq_fwd(int T, int N, const float *gi, const float *h0, const float *masks, const float *w_hh, const float *b_hh,
                   float *hs, float *hms, float *gates, void *stream);
int cn_gru_seq_bwd(int T, int N, const float *gates, const float *hms, const float *masks, const float *w_hh,
                   const float *d_hs, float *dgi, float *dgh, float *dh0, void *stream);

/* ---- large Linear layers of the PPO update (training path), split-precision bf16x3 MFMA like the rollout forward ----
 * Replace torch.nn.Linear forward/backward of embedding_layer.2, the folded (q|k|v)_linear∘in_proj and the folded
 * out_proj∘spatial_linear (rl/networks/selfAttn_srnn_temp_node.py:63-91,408) as autograd runs them inside PPO.update
 * (rl/ppo.py:60-95).  All pointers are device pointers; hi/lo are bf16 planes (uint16 storage) of the weight.
 * cn_split_bf16:   w [rows,cols] fp32 -> hi, lo (bf16) of w (transpose = 0) or of w^T [cols,rows] (transpose = 1), stored in
 *                  the fragment order cn_linear_fwd loads (opaque: only cn_linear_fwd reads these planes).  The weight as
 *                  the product sees it must be [32 a, 16 b].
 * cn_linear_fwd:   Y[M,N] = act(X[M,K] W^T + bias), W given as hi/lo [N,K]; act 0 = none, 1 = ReLU; bias may be NULL.
 *                  With the transposed split of W [N,K] passed as a [K,N] weight it computes dX = dY W (no bias).
 *                  relu_gate (optional, same shape and leading dimension as X): X is replaced by X * [relu_gate > 0] while it
 *                  is loaded -- the backward of Linear+ReLU without a separate masking pass.  N % 128 == 0, K % 64 == 0.
 * cn_linear_fwd_act: the same product with the epilogues of the robot-node sequence (rl/networks/srnn_model.py actor / critic trunks: tanh): act 0 = none,
 *                  1 = ReLU, 2 = tanh, 3 = times relu'(.) = [aux > 0], 4 = times tanh'(.) = 1 - aux^2, aux [M, ldaux] being the forward VALUE of
 *                  the activation the product is a gradient of; columns >= relu_from get a ReLU on top (pass relu_from >= N for none).
 * cn_split_bf16_padded: cn_split_bf16 with the weight the product sees zero-padded to n_padded rows (a layer whose output count is not a
 *                  multiple of 128; 0 = no padding).
 * cn_linear_wgrad: dW[N,K] = dY[M,N]^T X[M,K] and (optional) db[N] = column sums of dY (dY gated by relu_gate > 0 when that
 *                  pointer, shaped like dY, is given).  The M reduction is cut into
 *                  `splits` ranges whose partial products land in partials [splits,N,K] (db_partials [splits,N]) and are
 *                  summed in split order (deterministic).  N % 64 == 0, K % 128 == 0.
 * cn_linear_wgrad_splits: the split count the library would pick for (M,N,K); 0 if the shape is unsupported. */
int cn_split_bf16(const float *w, int rows, int cols, int transpose, void *hi, void *lo, void *stream);
int cn_linear_fwd(int M, int N, int K, const float *X, int ldx, const float *relu_gate, const void *Whi, const void *Wlo,
                  const float *bias, int act, float *Y, int ldy, void *stream);
int cn_split_bf16_padded(const float *w, int rows, int cols, int transpose, int n_padded, void *hi, void *lo, void *stream);
int cn_linear_fwd_act(int M, int N, int K, const float *X, int ldx, const void *Whi, const void *Wlo, const float *bias, int act,
                      const float *aux, int ldaux, int relu_from, float *Y, int ldy, void *stream);
int cn_linear_wgrad_splits(int M, int N, int K);
/* C[M,N] (contiguous) = A . B in exact fp32, A and B addressed through element strides (A[m,k] = A[m * a_stride_m + k * a_stride_k], B[k,n] likewise):
 * the small weight-by-weight products of the update -- the affine folds of the mirror (policy.py: (q|k|v)_linear o in_proj, out_proj o
 * spatial_linear, Ws^T Wt, (actor.0 ; critic.0) o output_linear; selfAttn_srnn_temp_node.py:63-91, :160-163, :262-268 compute the unfolded
 * chains) and their backward, every transposed form being a choice of strides; N = 1 is a matrix-vector product.  Dimensions <= 4096. */
int cn_small_mm(int M, int N, int K, const float *A, int64_t a_stride_m, int64_t a_stride_k, const float *B, int64_t b_stride_k, int64_t b_stride_n,
                float *C, void *stream);
int cn_linear_wgrad(int M, int N, int K, const float *dY, int ldy, const float *relu_gate, const float *X, int ldx, int splits,
                    float *partials, float *db_partials, float *dW, float *db, void *stream);

/* ---- GST trajectory predictor + VecPretextNormalize (CrowdSimPredRealGST-v0, BASELINE configs[3]) ----
 * cn_gst_predict          <- gst_updated/scripts/wrapper/crowd_nav_interface_parallel.py:45-114 CrowdNavPredInterfaceMultiEnv.forward
 *                            (st_model.forward, gst_updated/src/gumbel_social_transformer/st_model.py:271-455, shipped hyper-parameters)
 * cn_gst_wrapper_reset    <- rl/vec_env/vec_pretext_normalize.py:85-101 VecPretextNormalize.reset (history buffers)
 * cn_gst_wrapper_step     <- rl/vec_env/vec_pretext_normalize.py:112-191 process_obs_rew
 * Device pointers to the fp32 parameters, named after the checkpoint's state_dict keys (epoch_100.pt). */
typedef struct {
    const float *node_embedding_w, *node_embedding_b;      /* gumbel_social_transformer.node_embedding [64,2] */
    const float *in_proj_w, *in_proj_b;                    /* ...node_encoder_layers.0.self_attn.in_proj_* [192,64] */
    const float *out_proj_w, *out_proj_b;                  /* ...self_attn.out_proj [64,64] */
    const float *norm_node_w, *norm_node_b;                /* ...norm_node [64] */
    const float *norm1_node_w, *norm1_node_b;              /* ...norm1_node [64] */
    const float *linear1_w, *linear1_b;                    /* ...linear1 [128,64] */
    const float *linear2_w, *linear2_b;                    /* ...linear2 [64,128] */
    const float *lstm_w_ih, *lstm_w_hh, *lstm_b_ih, *lstm_b_hh; /* lstm.*_l0 [256,64],[256,64],[256],[256] */
    const float *hidden2pos_w, *hidden2pos_b;              /* hidden2pos [5,64] */
} cn_gst_weights;
typedef struct cn_gst cn_gst;
int cn_gst_create(int human_num, int max_envs, cn_gst **out);
/* The prediction horizon P = pred_seq_len of the predictor = sim.predict_steps of the env, 1 <= pred_steps <= CN_MAX_PRED: the handle decodes P
 * steps per forward, out_traj is [E,H,P,5] and the wrapper's edges are 2 (P + 1) wide.  The observed length stays 5 and the parameters
 * (cn_gst_weights) do not depend on P: the decode is a recurrence.  cn_gst_create is cn_gst_create_horizon with P = 5 -- the same launches and
 * bits.  cn_gst_pred_steps: the handle's P.  (CN_ABI_VERSION is unchanged: these are additions, no existing signature or struct layout moved.) */
int cn_gst_create_horizon(int human_num, int max_envs, int pred_steps, cn_gst **out);
int cn_gst_pred_steps(const cn_gst *g);
int cn_gst_destroy(cn_gst *g);
int cn_gst_set_weights(cn_gst *g, const cn_gst_weights *w, void *stream);
/* in_traj [E,H,5,2] world positions, in_mask [E,H,5] (0/1 float) -> out_traj [E,H,P,5] = cumulative (mu_x, mu_y, sigma_x,
 * sigma_y, corr), positions -999 where the pedestrian is not predicted; out_mask [E,H] (0/1 float).  P: the handle's horizon. */
int cn_gst_predict(cn_gst *g, int E, const float *in_traj, const float *in_mask, float *out_traj, float *out_mask, void *stream);
int cn_gst_wrapper_reset(cn_gst *g, int E, void *stream);
/* Prediction stride (rl/vec_env/vec_pretext_normalize.py:56-57, :133-134): pred_interval = int(data.pred_timestep // env.time_step); the
 * wrapper keeps the last (5 - 1) * pred_interval + 1 observations and feeds every pred_interval-th of them (oldest first) to the predictor.
 * Default 1 (every shipped config).  Re-allocates the history: call before cn_gst_wrapper_reset.  cn_gst_wrapper_history_len = that length. */
int cn_gst_wrapper_set_interval(cn_gst *g, int pred_interval);
int cn_gst_wrapper_history_len(const cn_gst *g);
/* Checkpointing of the wrapper's observation history (traj_buffer / mask_buffer, vec_pretext_normalize.py:85-101), in time order, oldest first:
 * traj [len,E,H,2] float32, mask [len,E,H] uint8 (device buffers), len = cn_gst_wrapper_history_len.  With the simulator snapshot
 * (cn_env_save) this makes a resumed CrowdSimPredRealGST-v0 run continue bit for bit. */
int cn_gst_wrapper_save(cn_gst *g, float *traj, uint8_t *mask, void *stream);
int cn_gst_wrapper_load(cn_gst *g, int E, const float *traj, const uint8_t *mask, void *stream);
/* obs: the raw CrowdSimPredRealGST-v0 observation (robot_node, spatial_edges [E,H,2(P+1)] by human id, visible_masks; P = the handle's
 * horizon, 12 columns at the shipped 5).  Pushes the new positions into the 5-deep history, runs the predictor, adds the social penalty
 * min_{h, k < P}(collision * penalty / 2^(k+2)) to rewards [E] (in place, may be NULL) and writes spatial_edges_out [E,H,2(P+1)]:
 * predictions in the robot frame where valid, rows sorted by current distance. */
int cn_gst_wrapper_step(cn_gst *g, int E, const cn_obs *obs, float robot_plus_human_radius, float collision_penalty, float *rewards,
                        float *spatial_edges_out, void *stream);

/* ---- GST predictor TRAINING step: forward + negative log-likelihood + backward of one batch of sequences ----
 * gst_updated/scripts/experiments/train.py:107-146 (loop body) over st_model.py:271-455 (training-time forward: 'faster_lstm', recursive decoding on
 * the mean, sampling = False) and :62-112 (negative_log_likelihood_full_partial), shipped hyper-parameters.  One workgroup per sequence:
 *   v_obs [B,5,N,2], v_pred [B,5,N,2]: displacements of the N pedestrians (seq_to_graph's vertices; -999 where missing),
 *   loss_mask_rel [B,N,10]: 1 where the displacement exists (the per-step attention masks are its outer products, trajectories.py:131-133).
 * 4 <= N <= 64 (pad a smaller crowd with absent pedestrians: mask rows of zeros).  grads: same struct as the weights, every field WRITTEN with
 * d(loss)/d(parameter), loss = sum of the masked NLL over the batch / number of valid (step, pedestrian) pairs (train.py:131-133; B = 1 is
 * the shipped batch size).  p_drop: the reference's dropout (0.1 while training; four sites), masks from a counter-based hash of `seed` --
 * this library's own stream, not torch's; p_drop = 0 reproduces the reference's gradients.  loss_out [2] = loss, valid-pair count;
 * gauss_out (optional) [B,5,N,5] = mu_x, mu_y, sigma_x, sigma_y, corr of every predicted step.  The optimiser step is cn_adam_clip_step. */
int64_t cn_gst_train_workspace_bytes(int B, int N);
int cn_gst_train_step(int B, int N, const float *v_obs, const float *v_pred, const float *loss_mask_rel, const cn_gst_weights *w, const cn_gst_weights *grads,
                      float p_drop, uint64_t seed, void *workspace, int64_t workspace_bytes, float *loss_out, float *gauss_out, void *stream);
/* The same step at a prediction horizon of P = pred_seq_len steps, 1 <= P <= CN_MAX_PRED: v_pred [B,P,N,2], loss_mask_rel [B,N,5+P], gauss_out
 * [B,P,N,5]; 4 + P encoder-layer passes and LSTM steps per sequence.  The entry points above are these with P = 5 (same launches, same bits).
 * The dropout stream for general P: the mask of element `idx` of dropout site `site` (0 attention probabilities [8,N,N], 1 out_proj output
 * [N,64], 2 FFN hidden [N,128], 3 FFN output [N,64]; idx = the element's row-major offset) in encoder-layer pass `call` of sequence b is a
 * function of (seed + 0x632BE59BD9B4E019 (b + 1), call * 4 + site + 1, idx) alone, where call counts the 4 + P passes in forward order: 0 .. 4 the
 * observed slices, 4 + tt the pass in front of decode step tt = 1 .. P - 1.  P does not enter: a pass that exists at two horizons draws the
 * same mask at both. */
int64_t cn_gst_train_workspace_bytes_horizon(int B, int N, int P);
int cn_gst_train_step_horizon(int B, int N, int P, const float *v_obs, const float *v_pred, const float *loss_mask_rel, const cn_gst_weights *w,
                              const cn_gst_weights *grads, float p_drop, uint64_t seed, void *workspace, int64_t workspace_bytes, float *loss_out,
                              float *gauss_out, void *stream);

/* ---- GST predictor EVALUATION step: validation (decode on the mean) and the sampled test protocol, B sequences per call ----
 * Replaces, per sequence, the body of gst_updated/scripts/experiments/eval.py:63-117 (`inference`): st_model.forward (st_model.py:271-455, dropout
 * off) with sampling = False (mode 'val', eval.py:69-82) or S times with sampling = True (mode 'test', eval.py:84-107), negative_log_likelihood_
 * full_partial (st_model.py:62-112) and average_offset_error / final_offset_error (mgnn/utils.py:8-28) under loss_mask_per_pedestrian.
 * v_obs, v_pred, loss_mask_rel, w, the bounds on N and the padding rule: as cn_gst_train_step; every weight pointer 16-byte aligned.
 *   S = 0: one decode per sequence that feeds the mean back; noise must be NULL.
 *   1 <= S <= 64: S decodes per sequence; decode step t of sample s feeds back mu + (sx e_x, corr sy e_x + sqrt(1 - corr^2) sy e_y)
 *     (st_model.py:235-240) times loss_mask_rel_full_partial, (e_x, e_y) = noise[b, s, t, n] -- noise [B,S,5,N,2]: standard-normal draws supplied
 *     by the CALLER.  The library draws nothing: equal arguments give equal bits.  The five observed encoder passes / LSTM steps do not depend
 *     on the draws and run once per sequence; all B x S decodes of a call are in flight together.
 * Outputs, R = max(S, 1) rows per sequence:
 *   seq_out   [B,R,4]      sum of the masked NLL, number of valid (step, pedestrian) pairs, sum of the masked aoe, sum of the masked foe
 *   ped_out   [B,R,N,3]    (optional) aoe, foe, loss_mask_per_pedestrian; a pedestrian not present at all ten steps has aoe = foe = 0 exactly
 *   gauss_out [B,R,5,N,5]  (optional) mu_x, mu_y, sigma_x, sigma_y, corr of every predicted step
 * eval.py's per-sequence loss is seq_out[.,.,0] / seq_out[.,.,1]. */
int64_t cn_gst_eval_workspace_bytes(int B, int N, int S);
int cn_gst_eval_step(int B, int N, int S, const float *v_obs, const float *v_pred, const float *loss_mask_rel, const cn_gst_weights *w, const float *noise,
                     void *workspace, int64_t workspace_bytes, float *seq_out, float *ped_out, float *gauss_out, void *stream);
/* The same at a prediction horizon of P steps, 1 <= P <= CN_MAX_PRED: v_pred [B,P,N,2], loss_mask_rel [B,N,5+P], noise [B,S,P,N,2], gauss_out
 * [B,R,P,N,5]; the average offset error is over the P steps, and a pedestrian counts when present at all 5 + P.  A sequence lives in LDS:
 * 133 KB at N = 64, P = 8, the largest case, of the CU's 160 KiB.  The entry points above are these with P = 5. */
int64_t cn_gst_eval_workspace_bytes_horizon(int B, int N, int S, int P);
int cn_gst_eval_step_horizon(int B, int N, int S, int P, const float *v_obs, const float *v_pred, const float *loss_mask_rel, const cn_gst_weights *w,
                             const float *noise, void *workspace, int64_t workspace_bytes, float *seq_out, float *ped_out, float *gauss_out, void *stream);

/* ---- GST predictor training DATA on the device: sequences from the collect batch's observation log, and minibatches of them ----
 * Replaces gst_updated/src/mgnn/trajectories.py:9-160 (TrajectoriesDataset: obs 5, pred 5, skip 1, frame_diff 1, invalid -999) over the text
 * files of collect_data.py, without the files: the output is what that class holds for the files written from the same log, envs in order.
 *   log [F,E,H,4] float32, 16-byte aligned: the pred_info rows of F sampled observations of E CrowdSimVarNumCollect-v0 envs -- frame id,
 *   prediction id, px, py; a row is visible (a line of the file) iff py is not infinite.  F >= 10, 1 <= H <= 64, F * E < 2^24.
 * The rule.  Per env the samples with a visible row are its frames, in order, with the frame id of their visible rows.  Candidate window i is
 * frames i .. i+9 of that list; with W = frames - 9 candidates, i belongs to mode TRAIN iff i < (int)((W + 1) * 0.8) in float64, to VAL
 * otherwise, to ALL always.  A candidate becomes a sequence iff consecutive frame ids differ by exactly 1 and some prediction id has a row in
 * all ten frames.  Its pedestrians are the window's distinct prediction ids in ascending order; positions are the float32 values, -999 where
 * the pedestrian has no row; a displacement is (float)((double)x[t] - (double)x[t-1]) where both exist and 0 at t = 0 where x[0] exists, else
 * -999; loss_mask = 1 where a row exists, loss_mask_rel = 1 where the displacement does.  Sequences are ordered by (env, i).
 * Status word (int32 on the device, zeroed by the caller, OR-ed into): the log is refused if it is not zero after cn_gst_data_count --
 *   CN_GSTD_FRAME_ORDER     the frame ids of an env's list do not strictly increase (an episode boundary), or the visible rows of one sample
 *                           carry different frame ids
 *   CN_GSTD_DUPLICATE_ID    two visible rows of one sample carry the same prediction id
 *   CN_GSTD_TOO_MANY_PEDS   a sequence has more than 64 pedestrians (the bound of cn_gst_train_step / cn_gst_eval_step)
 * Three calls around two exclusive sums the caller runs on the device (so the ragged output needs no atomics and no launch-order dependence):
 *   cn_gst_data_frames  -> visible [F,E] int32 0/1, frame_id [F,E] float32
 *   (listed_before [F,E] int32 = exclusive sum of visible along F)
 *   cn_gst_data_count   -> frame_list [E,F] int32 scratch, ped_count [E*(F-9)] int32 pedestrians of candidate e*(F-9)+i (0: not a sequence of
 *                          this mode), first_frame [E*(F-9)] float32 its first frame id
 *   (ped_offset [E*(F-9)] int32 = exclusive sum of ped_count; total_peds = its total)
 *   cn_gst_data_fill    -> obs_traj, pred_traj, obs_traj_rel, pred_traj_rel [total_peds,2,5], loss_mask, loss_mask_rel [total_peds,10]; the same
 *                          mode and buffers as the count call. */
enum { CN_GSTD_ALL = 0, CN_GSTD_TRAIN = 1, CN_GSTD_VAL = 2 };
enum { CN_GSTD_FRAME_ORDER = 1, CN_GSTD_DUPLICATE_ID = 2, CN_GSTD_TOO_MANY_PEDS = 4 };
int cn_gst_data_frames(int F, int E, int H, const float *log, int32_t *visible, float *frame_id, int32_t *status, void *stream);
int cn_gst_data_count(int F, int E, int H, int mode, const float *log, const int32_t *visible, const int32_t *listed_before,
                      const float *frame_id, int32_t *frame_list, int32_t *ped_count, float *first_frame, int32_t *status, void *stream);
int cn_gst_data_fill(int F, int E, int H, int mode, const float *log, const int32_t *visible, const int32_t *listed_before,
                     const float *frame_id, const int32_t *frame_list, const int32_t *ped_count, const int32_t *ped_offset,
                     int64_t total_peds, float *obs_traj, float *pred_traj, float *obs_traj_rel, float *pred_traj_rel, float *loss_mask,
                     float *loss_mask_rel, void *stream);
/* One minibatch for cn_gst_train_step / cn_gst_eval_step: v_obs, v_pred [B,5,Np,2] and loss_mask_rel_out [B,Np,10] of the sequences
 * index [B] (int32, device) of a dataset of num_seq sequences (seq_start / seq_count [num_seq] int32: first pedestrian row and crowd).
 * v[b,t,n,c] = traj_rel[seq_start + n, c, t] (mgnn/utils.py:44-77 seq_to_graph), rotated by (c, s) = cos_sin[b] (float32 [B,2]) as
 * mgnn/utils.py:80-90 rotate_graph does: x*c - y*s, x*s + y*c, every product and sum rounded once, the -999 entries included; cos_sin NULL
 * copies instead (zeros keep their sign).  Rows n >= seq_count are zeros, values and mask; 4 <= Np <= 64, crowds above Np are cut. */
int cn_gst_gather_batch(int B, int Np, int num_seq, int64_t total_peds, const int32_t *index, const float *cos_sin, const int32_t *seq_start,
                        const int32_t *seq_count, const float *obs_traj_rel, const float *pred_traj_rel, const float *loss_mask_rel,
                        float *v_obs, float *v_pred, float *loss_mask_rel_out, void *stream);
/* The data calls at a prediction horizon of P = pred_seq_len steps, 1 <= P <= CN_MAX_PRED (TrajectoriesDataset(obs_seq_len=5, pred_seq_len=P)):
 * read 5 + P for every 10, 4 + P for every 9 and "all 5 + P frames" for "all ten" in the rule above -- F >= 5 + P, W = F - (4 + P) candidates
 * per env; pred_traj, pred_traj_rel [total_peds,2,P], loss_mask, loss_mask_rel [total_peds,5+P]; the gather writes v_pred [B,P,Np,2] and
 * loss_mask_rel_out [B,Np,5+P].  A log of fewer than 5 + P samples is refused and launches nothing.  The calls above are these with P = 5. */
int cn_gst_data_frames_horizon(int F, int E, int H, int P, const float *log, int32_t *visible, float *frame_id, int32_t *status, void *stream);
int cn_gst_data_count_horizon(int F, int E, int H, int mode, int P, const float *log, const int32_t *visible, const int32_t *listed_before,
                              const float *frame_id, int32_t *frame_list, int32_t *ped_count, float *first_frame, int32_t *status, void *stream);
int cn_gst_data_fill_horizon(int F, int E, int H, int mode, int P, const float *log, const int32_t *visible, const int32_t *listed_before,
                             const float *frame_id, const int32_t *frame_list, const int32_t *ped_count, const int32_t *ped_offset,
                             int64_t total_peds, float *obs_traj, float *pred_traj, float *obs_traj_rel, float *pred_traj_rel, float *loss_mask,
                             float *loss_mask_rel, void *stream);
int cn_gst_gather_batch_horizon(int B, int Np, int P, int num_seq, int64_t total_peds, const int32_t *index, const float *cos_sin,
                                const int32_t *seq_start, const int32_t *seq_count, const float *obs_traj_rel, const float *pred_traj_rel,
                                const float *loss_mask_rel, float *v_obs, float *v_pred, float *loss_mask_rel_out, void *stream);

/* ---- rollout math ---- */
/* rewards [T,N], values [T+1,N], masks [T+1,N] -> returns[t][n] for t < T (row T untouched).  fp32, torch op order. */
int cn_gae(int T, int N, const float *rewards, const float *values, const float *masks, double gamma, double lam,
           float *returns, void *stream);
/* stats[3] (float64, device) = {sum, sum of squares, count} of (returns - values) over n elements */
int cn_adv_stats(int64_t n, const float *returns, const float *values, double *stats, void *stream);
/* adv = ((returns - values) - mean) / (std_unbiased + 1e-5) with mean/std derived from stats (possibly all-reduced) */
int cn_adv_normalize(int64_t n, const float *returns, const float *values, const double *stats, float *adv, void *stream);

/* bench.Monitor's aggregate of one vec-env step (rl/networks/envs.py:70-73, train.py:180-182) from the outputs of cn_env_step: acc[8] (float64,
 * device) += {finished episodes, sum of their returns, sum of their lengths, timeouts, collisions, goals reached, -, -}.  One launch with a
 * fixed summation order instead of two dozen small reductions per rollout step. */
int cn_episode_stats_update(int E, const uint8_t *done, const uint8_t *info, const double *ep_return, const int32_t *ep_len, double *acc, void *stream);

/* The per-step bookkeeping of the evaluation protocol (rl/evaluation.py:49-110) for the FIRST episode of each of E envs, from the outputs of
 * cn_env_step as they are: done / info [E] u8, ep_return [E] f64, robot_node = the [E,1,7] float32 rows of the NEW observation (auto-reset start
 * of the next episode where done), danger_dist [E] f64 = cn_env_get_danger_min_dist of that step.  One launch, one workgroup, no atomics: a rerun
 * gives the same bits.  state: caller-owned, 8-byte words, cn_eval_state_words(E) = CN_EVAL_HEADER_WORDS + CN_EVAL_FIELDS * E of them:
 *   word CN_EVAL_N_ACTIVE (int64): envs whose first episode is still running after this call (OUTPUT; the other header words are reserved)
 *   then CN_EVAL_FIELDS arrays of E words each, array f at word CN_EVAL_HEADER_WORDS + f * E:
 *     ACTIVE int64 0/1 | STEPS int64 | DANGER_STEPS int64 | OUTCOME int64 (CN_INFO_* of the final step) |
 *     DANGER_SUM f64 (sum of danger_dist over the Danger steps, in step order) | PATH_LENGTH f64 (sum of the float32 norm of the float32 position
 *     difference, jump to the auto-reset start included) | RETURN f64 (ep_return at the final step) | LAST_POS 2 x float32 (x, y).
 * The caller starts an evaluation with ACTIVE = 1, LAST_POS = the robot position of the reset observation and everything else 0.  An env with
 * ACTIVE = 0 is left alone, so steps fed after every env has finished change nothing.  masks (optional, [E] float32) <- done == 0. */
enum { CN_EVAL_HEADER_WORDS = 8, CN_EVAL_N_ACTIVE = 0, CN_EVAL_FIELDS = 8 };
enum { CN_EVAL_ACTIVE = 0, CN_EVAL_STEPS = 1, CN_EVAL_DANGER_STEPS = 2, CN_EVAL_OUTCOME = 3, CN_EVAL_DANGER_SUM = 4, CN_EVAL_PATH_LENGTH = 5,
       CN_EVAL_RETURN = 6, CN_EVAL_LAST_POS = 7 };
int64_t cn_eval_state_words(int E);
int cn_eval_accumulate(int E, const uint8_t *done, const uint8_t *info, const double *ep_return, const float *robot_node, const double *danger_dist,
                       int64_t *state, float *masks, void *stream);

/* ---- PPO losses (rl/ppo/ppo.py:66-84) ----
 * values, logp (new policy), old_logp, adv (normalised advantages), value_preds, returns: [n] float32 (the [T*N,1] minibatch
 * tensors of recurrent_generator).  fwd: losses[0] = value_loss = 0.5 * mean(max((v - R)^2, (vp + clamp(v - vp, +-clip) - R)^2))
 * (or 0.5 * mean((R - v)^2) when use_clipped_value_loss == 0), losses[1] = action_loss = -mean(min(ratio * A,
 * clamp(ratio, 1 - clip, 1 + clip) * A)), ratio = exp(logp - old_logp).  workspace: cn_ppo_loss_workspace_doubles() float64.
 * bwd: d_values[n], d_logp[n] = gradients of g_losses[0] * value_loss + g_losses[1] * action_loss (g_losses: 2 floats on the
 * DEVICE, the upstream gradients autograd hands in -- value_loss_coef and 1 in ppo.py:86); torch's tie rules for min / max /
 * clamp.  The entropy term of ppo.py:86 depends on dist.logstd only and stays in the host mirror. */
int cn_ppo_loss_workspace_doubles(void);
int cn_ppo_loss_fwd(int64_t n, const float *values, const float *logp, const float *old_logp, const float *adv,
                    const float *value_preds, const float *returns, float clip_param, int use_clipped_value_loss,
                    double *workspace, float *losses, void *stream);
int cn_ppo_loss_bwd(int64_t n, const float *values, const float *logp, const float *old_logp, const float *adv,
                    const float *value_preds, const float *returns, float clip_param, int use_clipped_value_loss,
                    const float *g_losses, float *d_values, float *d_logp, void *stream);

/* ---- gradient-norm clip + Adam over one flat bucket (rl/ppo/ppo.py:88-90, optimiser of ppo.py:32) ----
 * param, grad, exp_avg, exp_avg_sq: [n] float32, the concatenation of all parameters / their gradients / Adam moments in
 * Module.parameters() order (the host mirror makes every p.data / p.grad / optimizer.state[p] a view into these).
 * grad <- grad * grad_scale (1 / world_size after a sum all-reduce, else 1); total_norm = ||grad||_2;
 * grad <- grad * min(1, max_grad_norm / (total_norm + 1e-6)) (skipped when max_grad_norm <= 0); then torch.optim.Adam's
 * update for step number `step` (1-based), no weight decay / amsgrad.  workspace: cn_adam_workspace_doubles() float64;
 * grad_norm_out (optional, 1 float, device) receives total_norm.  Two launches, no host synchronisation. */
int cn_adam_workspace_doubles(void);
int cn_adam_clip_step(int64_t n, float *param, float *grad, float *exp_avg, float *exp_avg_sq, double grad_scale,
                      double max_grad_norm, double lr, double beta1, double beta2, double eps, int64_t step, double *workspace,
                      float *grad_norm_out, void *stream);

/* ---- one PPO minibatch step as ONE boundary call (rl/ppo/ppo.py:55-95 for one `sample` of the recurrent generator) ----
 * Replaces, for the attention-graph network (use_self_attn, sort_humans; crowds of <= 48 humans, edge width <= 16) at the default sizes -- and,
 * through cn_ppo_minibatch_step_sized below, at every cn_policy_dims tuple of the device box --, the statement sequence
 *   sample = recurrent_generator(...)            rl/networks/storage.py:184-253  (gather of N whole env trajectories by index)
 *   evaluate_actions(...)                        rl/networks/model.py:82-90
 *   value_loss / action_loss / entropy           rl/ppo/ppo.py:66-86
 *   optimizer.zero_grad(); total.backward()      rl/ppo/ppo.py:87-88
 * by: gather -> affine folds -> cn_hh_block_fwd -> cn_rn_seq_fwd -> cn_ppo_loss_fwd/bwd -> cn_rn_seq_bwd -> the per-layer backward of
 * the human-human block -> chain rule of the folds, everything on `stream`, with NO framework kernel in between: every parameter gradient
 * is WRITTEN (not accumulated) to grads-><same field>; parameters the loss does not reach (attn.spatial_edge_layer.bias) get an exact
 * zero.  The caller then runs its gradient all-reduce (data parallel) and cn_adam_clip_step on the flat bucket the pointers live in.
 *
 * storage tensors (float32, contiguous, device; T = num_steps, E = envs in storage):
 *   robot_node [T+1,E,1,7], temporal_edges [T+1,E,1,2], spatial_edges [T+1,E,H,D], detected_human_num [T+1,E,1], h0 = recurrent_hidden_states
 *   ['human_node_rnn'][0] [E,1,128], masks [T+1,E,1], actions [T,E,2], value_preds / returns [T+1,E,1], old_logp = action_log_probs [T,E,1],
 *   adv = normalised advantages [T,E,1];  env_idx [N] int32 = perm[start : start + N] (storage.py:209-210).
 * rows = sum over the minibatch of clamp(detected_human_num, 1, H) -- the caller knows it from cn_ppo_row_totals (one readback per
 * update(), not per minibatch); the call fails with CN_ERR_INVALID if the workspace is smaller than cn_ppo_minibatch_workspace_bytes.
 * losses_out [3] (device) = value_loss, action_loss, dist_entropy (ppo.py:66-86, the three numbers update() averages). */
typedef struct {
    int T, N, E, H, D;
    const int32_t *env_idx;
    const float *robot_node, *temporal_edges, *spatial_edges, *detected_human_num, *h0, *masks, *actions, *value_preds, *returns, *old_logp, *adv;
} cn_ppo_batch;
typedef struct {
    float clip_param, value_loss_coef, entropy_coef;
    int use_clipped_value_loss;
} cn_ppo_hyper;
/* The most rows one call takes (host-only, no device needed): rows * 1536 < 2^31, the 32-bit element offsets into the [rows, 1536] q|k|v
 * gradient -- a bound on the LIVE rows, not on T * N * H.  Past it cn_ppo_minibatch_workspace_bytes returns 0 and cn_ppo_minibatch_step fails
 * with CN_ERR_INVALID before any launch; the caller takes another route for that minibatch. */
int64_t cn_ppo_minibatch_max_rows(void);
int64_t cn_ppo_minibatch_workspace_bytes(int T, int N, int H, int D, int64_t rows); /* 0 = shape outside the box above, or rows past the bound */
/* totals [E] int32 (device) = sum_t clamp(detected_human_num[t, e], 1, H) over t < T: the compacted rows env e contributes to a minibatch */
int cn_ppo_row_totals(int T, int E, int H, const float *detected_human_num, int32_t *totals, void *stream);
int cn_ppo_minibatch_step(const cn_ppo_batch *batch, int64_t rows, const cn_policy_weights *params, const cn_policy_weights *grads,
                          const cn_ppo_hyper *hyper, void *workspace, int64_t workspace_bytes, float *losses_out,
                          float *value_logp_out /* optional [2, T * N]: values, log-probs of the minibatch (tests) */, void *stream);
/* The same step at the network sizes of cn_policy_dims (R, M, A, O) inside the device box of cn_policy_create_sized.  dims == NULL or the default
 * tuple: cn_ppo_minibatch_step / cn_ppo_minibatch_workspace_bytes themselves (they forward here) -- the same launches on the same buffers, the
 * same bits, the same workspace size.  Outside the box the step fails with CN_ERR_INVALID naming the box and launches nothing; the workspace
 * query, which runs on the host, returns 0.  H <= 48, D <= 16 and cn_ppo_minibatch_max_rows() are unchanged (the human-human block in front of
 * out_sp [rows,256] does not depend on dims).  params / grads have the shapes listed under cn_policy_create_sized; batch->h0 is [E,1,R].
 * Inside, te = [Ws^T Wt ; encoder_linear] is [256+M,256] (the fold over A is a K = A segment, left unscaled: the sequence takes the score
 * temperature H / sqrt(A) from dims), ac0 = (actor.0 ; critic.0) o output_linear is [2O,R], the saved activations have the widths listed for
 * cn_rn_saved under cn_rn_seq_fwd_sized, and the sequence's two workspaces come from cn_rn_seq_*_workspace_floats_sized.
 * (CN_ABI_VERSION is unchanged: these are additions, no existing signature or struct layout moved.) */
int64_t cn_ppo_minibatch_workspace_bytes_sized(int T, int N, int H, int D, int64_t rows, const cn_policy_dims *dims);
int cn_ppo_minibatch_step_sized(const cn_ppo_batch *batch, int64_t rows, const cn_policy_weights *params, const cn_policy_weights *grads,
                                const cn_ppo_hyper *hyper, const cn_policy_dims *dims, void *workspace, int64_t workspace_bytes,
                                float *losses_out, float *value_logp_out, void *stream);
/* The same step for the two switches of the attention-graph network the reference accepts besides its sizes (arguments.py:189, :206):
 *   self_attn = 0    args.use_self_attn = False: no human-human attention.  In place of the human-human block the step runs the two-layer MLP
 *                    out_sp = relu(relu(x W0^T + b0) W2^T + b2) on the compacted rows (cn_embed0_fwd, then cn_linear_fwd at K = 128, N = 256: the
 *                    arithmetic of the rollout under cn_policy_set_self_attention(p, 0)) and its per-layer backward.  params / grads are read as
 *                    cn_policy_set_weights reads them in that mode: emb0_w / emb0_b = base.spatial_linear.0 [128,D], spatial_linear_w / _b =
 *                    base.spatial_linear.2 [256,128]; the fields emb2_w .. out_proj_b are not read and may be NULL.  The workspace holds none of the
 *                    block's buffers: cn_ppo_minibatch_workspace_bytes_variant reports the smaller size this variant uses.
 *   sort_humans = 0  args.sort_humans = False: the storage's spatial_edges are NOT sorted by detection; visible_masks = the storage's
 *                    [T+1,E,H] visibility bytes (non-zero = visible) is required, detected_human_num is not read.  The gather moves each sample's
 *                    visible humans to the front in index order, the others behind them in index order (the rule of cn_obs_compact_visible, an
 *                    all-invisible sample keeps human 0), and counts max(1, visible) rows for it; everything behind the gather is unchanged.
 *                    rows = sum over the minibatch of max(1, visible): cn_ppo_row_totals_visible gives the per-env totals over t < T.
 * v == NULL and {1, 1, NULL} are cn_ppo_minibatch_step_sized itself (it forwards here): the same launches, the same bits, the same workspace size.
 * visible_masks is ignored while sort_humans != 0.  sort_humans = 0 with visible_masks == NULL fails with CN_ERR_INVALID naming the field, like
 * every other refusal before the first launch.  The shape box (1 <= H <= 48, 1 <= D <= 16, dims inside the device box) and
 * cn_ppo_minibatch_max_rows() hold for every variant.  Gradients are written, not accumulated; summation orders are fixed.
 * (CN_ABI_VERSION is unchanged: additions only; cn_ppo_batch and cn_policy_weights keep their layouts.) */
typedef struct { int32_t self_attn; int32_t sort_humans; const uint8_t *visible_masks; } cn_ppo_variant;
int64_t cn_ppo_minibatch_workspace_bytes_variant(int T, int N, int H, int D, int64_t rows, const cn_policy_dims *dims, const cn_ppo_variant *v);
int cn_ppo_minibatch_step_variant(const cn_ppo_batch *batch, int64_t rows, const cn_policy_weights *params, const cn_policy_weights *grads,
                                  const cn_ppo_hyper *hyper, const cn_policy_dims *dims, const cn_ppo_variant *v, void *workspace,
                                  int64_t workspace_bytes, float *losses_out, float *value_logp_out, void *stream);
/* totals [E] int32 (device) = sum over t < T of max(1, visible humans of env e at step t), visible_masks [T+1,E,H] bytes */
int cn_ppo_row_totals_visible(int T, int E, int H, const uint8_t *visible_masks, int32_t *totals, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CROWDNAV_HIP_H */
