"""PPO training loop over the device-resident simulator -- the flow of the reference's train.py:140-242 with the
per-step host round trips removed.

`collect_rollout` is the fused rollout: for each of the T steps the policy forward writes value / action / log-prob /
next hidden state straight into the RolloutStorage rows and the simulator writes the next observation, reward and
done mask straight into row t+1 -- no clones, no host synchronisation, no Python work proportional to E.
(The reference-compatible `envs.step()` path, which returns CPU rewards / numpy dones / info dicts, still exists for
an unmodified train.py; it costs one D2H sync and O(E) Python per step.)
"""
import time

import torch

from .policy import Policy
from .ppo import PPO
from .storage import RolloutStorage
from .vec_env import make_vec_envs


class EpisodeStats:
    """Device-side bench.Monitor aggregate: sum of finished-episode returns / lengths / outcome counts."""

    def __init__(self, device):
        self.acc = torch.zeros(8, dtype=torch.float64, device=device)  # n_done, sum_ret, sum_len, timeout, collision, goal, -, -

    def update(self, done, info, ep_return, ep_len):
        if (done.is_cuda and done.dtype == torch.uint8 and info.dtype == torch.uint8 and ep_return.dtype == torch.float64 and ep_len.dtype == torch.int32
                and all(t.is_contiguous() for t in (done, info, ep_return, ep_len))):
            from . import _abi as A      # the step outputs of HipEnvBatch as they are: ONE launch, fixed summation order
            A.call("cn_episode_stats_update", done.numel(), A.ptr(done), A.ptr(info), A.ptr(ep_return), A.ptr(ep_len), A.ptr(self.acc), A.stream_ptr())
            return
        d = done.to(torch.float64)
        self.acc[0] += d.sum()
        self.acc[1] += (ep_return * d).sum()
        self.acc[2] += (ep_len.to(torch.float64) * d).sum()
        for code in (1, 2, 3):
            self.acc[2 + code] += ((info == code).to(torch.float64) * d).sum()

    def pop(self):
        """Aggregate since the last pop, over ALL ranks when torch.distributed is initialised (each rank steps its own shard of envs)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            acc = self.acc if dist.get_backend() == "nccl" else self.acc.cpu()
            dist.all_reduce(acc)
            if acc is not self.acc:
                self.acc.copy_(acc)
        a = self.acc.cpu().tolist()
        self.acc.zero_()
        n = max(a[0], 1.0)
        return dict(episodes=int(a[0]), eprewmean=a[1] / n, eplenmean=a[2] / n, timeout=a[3] / n, collision=a[4] / n, success=a[5] / n)


def collect_rollout(envs, actor_critic, rollouts, stats=None, generator=None):
    """Fill `rollouts` (row 0 must hold the current observation / hidden state / mask).  Zero host syncs."""
    env = envs._env
    E, dev = envs.num_envs, envs.device
    pol = actor_critic._hip_handle(E, dev)
    T = rollouts.num_steps
    if "human_human_edge_rnn" in pol.state_shapes(E):                     # a live edge state (DS-RNN) is written row by row like the node state
        rollouts.materialize_edge_rnn()
    hxs = {k: rollouts.recurrent_hidden_states[k] for k in pol.state_shapes(E)}
    eps = torch.empty(T, E, 2, device=dev).normal_(generator=generator)   # the action noise of the whole rollout in one launch
    # the simulator writes a row plan beside every observation (hip_env.HipEnvBatch.row_plan): row t of the storage IS the newest observation of
    # `env` at every t of this loop (row 0: the last one of the previous rollout, or the reset), so the plan in the buffer is the one made
    # for it.  Not through the GST wrapper, which post-processes the observation.
    base = actor_critic.base
    plan = env.row_plan if (envs._pretext is None and base.use_self_attn and base.sort_humans and pol.uses_row_plan) else None
    for t in range(T):
        obs_t = {k: rollouts.obs[k][t] for k in ("robot_node", "temporal_edges", "spatial_edges", "detected_human_num")}
        out = dict(value=rollouts.value_preds[t], action=rollouts.actions[t], logp=rollouts.action_log_probs[t])
        pol_obs = obs_t
        if not base.sort_humans:   # args.sort_humans = False: attention masked by visible_masks -> visible humans first + their count
            pol_obs = base.counted_inputs(dict(obs_t, visible_masks=rollouts.obs["visible_masks"][t]))
        pol.act_rnn(pol_obs, {k: v[t] for k, v in hxs.items()}, rollouts.masks[t], eps=eps[t], out=out,
                    rnn_hxs_out={k: v[t + 1] for k, v in hxs.items()}, row_plan=plan)
        obs_n = {k: rollouts.obs[k][t + 1] for k in obs_t}
        obs_n["visible_masks"] = None
        if "visible_masks" in rollouts.obs:
            obs_n["visible_masks"] = rollouts.obs["visible_masks"][t + 1].view(torch.uint8)
        if envs._pretext is None:
            _, reward, done, info, ep_ret, ep_len = env.step(rollouts.actions[t], obs=obs_n, not_done=rollouts.masks[t + 1],
                                                             reward=rollouts.rewards[t])   # rows written in place
        else:
            # GST wrapper in the loop, in place as well: the simulator writes every row but the spatial edges, which the wrapper needs raw
            # (by human id): those go to the batch's own buffer, and the wrapper writes predictions / distance sort into the storage row and
            # adds the social penalty to the reward row
            raw = dict(obs_n, spatial_edges=env.obs["spatial_edges"])
            if raw["visible_masks"] is None:
                raw["visible_masks"] = env.obs["visible_masks"]
            _, reward, done, info, ep_ret, ep_len = env.step(rollouts.actions[t], obs=raw, not_done=rollouts.masks[t + 1], reward=rollouts.rewards[t])
            envs._pretext.process(raw, rollouts.rewards[t].view(E), out=rollouts.obs["spatial_edges"][t + 1])
        if stats is not None:
            stats.update(done, info, ep_ret, ep_len)
    rollouts.step = 0


def evaluate_policy(actor_critic, env_name, config, seed, eval_cases=None, device=None, predictor=None, logging=None):
    """The batched test protocol on the current weights through a policy handle of its OWN: Policy._hip_handle hands out one handle per
    policy, and what the training rollout has set on it (weight snapshot, gemm mode, a post-hh hook) stays as it is.  No torch RNG draw."""
    from .config import Config
    from .evaluation import _evaluate_batched
    config = config if config is not None else Config()
    if eval_cases is None:
        eval_cases = int(config.env.test_size)
    E = len(set((2 * k) % int(config.env.test_size) for k in range(eval_cases)))     # distinct cases = envs of the batch (evaluation.py)
    base = actor_critic.base
    pol = base.make_hip_handle(E, device)
    try:
        pol.set_gemm_mode(getattr(actor_critic, base.gemm_mode_attr))
        pol.set_weights(actor_critic.state_dict())
        return _evaluate_batched(actor_critic, env_name, config, seed, eval_cases, device, logging, predictor=predictor, hip_policy=pol)
    finally:
        pol.close()


def bootstrap_value(actor_critic, rollouts):
    obs = {k: rollouts.obs[k][-1] for k in ("robot_node", "temporal_edges", "spatial_edges", "detected_human_num", "visible_masks") if k in rollouts.obs}
    hxs = {"human_node_rnn": rollouts.recurrent_hidden_states["human_node_rnn"][-1]}
    if getattr(rollouts, "edge_rnn_live", False):          # DS-RNN: the value of the last row needs its edge state
        hxs["human_human_edge_rnn"] = rollouts.recurrent_hidden_states["human_human_edge_rnn"][-1]
    return actor_critic.get_value(obs, hxs, rollouts.masks[-1])


def save_checkpoint(save_dir, update, actor_critic, agent, envs, rollouts, stats, device):
    """`<save_dir>/checkpoints/<update:05d>.pt` is the policy state_dict exactly as train.py:213-219 writes it (loadable by the
    reference's test.py and by --resume); `<update:05d>.resume.pt` beside it holds what a BIT-EXACT continuation needs on top:
    optimiser state, both torch RNG streams, the simulator snapshot (cn_env_save), row 0 of the rollout storage and the episode
    statistics accumulator.  One pair per rank under torch.distributed (`.rankN` suffix) since env shards and noise streams differ."""
    import os
    rank = 0
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        rank = torch.distributed.get_rank()
    d = os.path.join(save_dir, "checkpoints")
    os.makedirs(d, exist_ok=True)
    stem = os.path.join(d, "%.5i" % update)
    if rank == 0:
        torch.save(actor_critic.state_dict(), stem + ".pt")
    agent.sync_optimizer_state()
    ck = {"format": 1, "update": update, "optimizer": agent.optimizer.state_dict(), "rng_cpu": torch.get_rng_state(),
          "rng_cuda": torch.cuda.get_rng_state(device), "env": envs.state_dict(),
          "rollout0": {"obs": {k: v[0].clone() for k, v in rollouts.obs.items()},
                       "hxs": rollouts.recurrent_hidden_states["human_node_rnn"][0].clone(), "masks": rollouts.masks[0].clone(),
                       "bad_masks": rollouts.bad_masks[0].clone(),
                       # derived data of that observation (hip.HipEnvBatch.row_plan): with it the first forward after a resume walks the
                       # same tiles, i.e. sums in the same order, as the uninterrupted run
                       "row_plan": envs._env.row_plan.clone()},
          "stats": stats.acc.clone()}
    if getattr(rollouts, "edge_rnn_live", False):          # DS-RNN: the live edge state of row 0
        ck["rollout0"]["edge_hxs"] = rollouts.recurrent_hidden_states["human_human_edge_rnn"][0].clone()
    path = stem + (".resume.pt" if rank == 0 else ".resume.rank%d.pt" % rank)
    torch.save(ck, path)
    return stem + ".pt", path


def load_checkpoint(policy_path, resume_path, actor_critic, agent, envs, rollouts, stats, device):
    """Inverse of save_checkpoint; returns the index of the next update."""
    actor_critic.load_state_dict(torch.load(policy_path, map_location=device))          # train.py:105-108
    ck = torch.load(resume_path, map_location="cpu")
    agent.optimizer.load_state_dict(ck["optimizer"])       # PPO re-binds its flat buckets to the restored moments at the next update()
    envs.load_state_dict(ck["env"])
    r0 = ck["rollout0"]
    for k in rollouts.obs:
        rollouts.obs[k][0].copy_(r0["obs"][k])
    rollouts.recurrent_hidden_states["human_node_rnn"][0].copy_(r0["hxs"])
    if "edge_hxs" in r0:
        rollouts.materialize_edge_rnn()[0].copy_(r0["edge_hxs"])
    rollouts.masks[0].copy_(r0["masks"]); rollouts.bad_masks[0].copy_(r0["bad_masks"])
    if "row_plan" in r0 and r0["row_plan"].numel() == envs._env.row_plan.numel():   # (load_state_dict above cleared it)
        envs._env.row_plan.copy_(r0["row_plan"])
    stats.acc.copy_(ck["stats"])
    torch.set_rng_state(ck["rng_cpu"])
    torch.cuda.set_rng_state(ck["rng_cuda"], device)
    return int(ck["update"]) + 1


def update_flops(live_rows, samples, ppo_epoch):
    """Algorithmic FLOPs of one PPO.update(): ppo_epoch passes over all samples, forward + backward (dX and dW: 2 x forward) of
      * the three dense layers of the human-human block on the live rows (embedding_layer.2 128->512, folded q|k|v 512->1536, folded
        out_proj∘spatial_linear 512->256: 1.966 MFLOP per row, the figure bench.py prices the rollout kernel with), and
      * the per-sample robot-node layers (robot_linear 9->256, [u | enc] 256->320, edge embed 256->64, GRU 2 x 128->384, folded
        output_linear∘(actor.0 | critic.0) 128->512, actor.2 / critic.2 256->256, heads): 0.79 MFLOP per sample.
    The attention cores, the D->128 input layer and all pointwise work are left out (< 3 %)."""
    hh = 2.0 * (128 * 512 + 512 * 1536 + 512 * 256)
    rn = 2.0 * (9 * 256 + 256 * 320 + 256 * 64 + 2 * 128 * 384 + 128 * 512 + 2 * 256 * 256 + 256 + 512)
    return 3.0 * ppo_epoch * (live_rows * hh + samples * rn)


NETWORK_FLAGS = ("human_node_rnn_size", "human_node_embedding_size", "attention_size", "human_node_output_size")     # arguments.py:155-181


def network_kwargs(network):
    """train(network=...): a dict of the reference's four network-size flags (any subset; the others keep 128 / 64 / 64 / 256) -> the entries it
    adds to the policy's base_kwargs."""
    network = dict(network or {})
    stray = sorted(set(network) - set(NETWORK_FLAGS))
    if stray:
        raise KeyError("train(network=...): unknown flag(s) %s; the network-size flags are %s" % (", ".join(stray), ", ".join(NETWORK_FLAGS)))
    return {k: int(v) for k, v in network.items()}


def new_rollouts(actor_critic, num_steps, num_processes, obs_spaces, action_space):
    """The rollout storage of `actor_critic`: its node state is as wide as the policy's GRU (human_node_rnn_size), the edge state 256."""
    base = actor_critic.base
    return RolloutStorage(num_steps, num_processes, obs_spaces, action_space, base.human_node_rnn_size, base.human_human_edge_rnn_size)


def train(env_name="CrowdSimVarNum-v0", num_processes=4096, num_steps=30, num_updates=10, seed=425, config=None, ppo_epoch=5,
          num_mini_batch=2, lr=4e-5, eps=1e-5, clip_param=0.2, value_loss_coef=0.5, entropy_coef=0.0, max_grad_norm=0.5, gamma=0.99,
          gae_lambda=0.95, log=print, device=None, save_dir=None, save_interval=0, resume=None, use_self_attn=True, sort_humans=None,
          pretext_wrapper=None, predictor=None, eval_interval=0, eval_cases=None, base=None, network=None):
    """Returns a list of per-update dicts (losses, timings, episode stats).  Works single- or multi-GPU (one process per
    GPU, torch.distributed initialised by the caller).  save_dir / save_interval: write checkpoints like train.py:213-219 (every
    `save_interval` updates and after the last one); resume = path of a `NNNNN.pt` written by this function: continue that run
    (updates NNNNN+1 .. num_updates-1) with results bit-identical to the uninterrupted run.
    pretext_wrapper: train CrowdSimPredRealGST-v0 behind the VecPretextNormalize processing (GST predictions in the observation, social
    penalty in the reward); None follows config.env.use_wrapper, as the reference's train.py:86 does.  predictor: a gst.GSTPredictor instead
    of the checkpoint under config.pred.model_dir.
    eval_interval: every that many updates and after the last one, run the batched test protocol (evaluation.evaluate_batched: eval_cases
    episodes, default config.env.test_size, phase 'test', same config / seed / predictor) on the current weights and put its metrics under
    rec["eval"].  The training run itself -- losses, statistics, checkpoints, weights -- is bit-identical with and without it: the evaluation
    owns its simulator, wrapper and policy handle and draws from no torch RNG stream.  Under torch.distributed rank 0 evaluates.
    base: the network, 'selfAttn_merge_srnn' or 'srnn' (the DS-RNN baseline).  None follows config.robot.policy when it names one of the two, as
    the reference's train.py:94 does, and is 'selfAttn_merge_srnn' otherwise.
    network: a dict of the reference's network-size flags (NETWORK_FLAGS: human_node_rnn_size, human_node_embedding_size, attention_size,
    human_node_output_size) for the attention-graph network; sizes outside the device box (_abi.DIMS_BOX) are refused before the first rollout.
    The rollout runs on the HIP kernels at any sizes in the box, and so does the update: PPO.update takes one boundary call per minibatch at
    every tuple of the box (cn_ppo_minibatch_step at the default sizes, cn_ppo_minibatch_step_sized off them).  With
    PPO.use_minibatch_step = False evaluate_actions is the same two boundary calls each way (cn_hh_block_fwd + the per-layer backward,
    cn_rn_seq_fwd_sized / cn_rn_seq_bwd_sized) joined by autograd."""
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(seed)
    if pretext_wrapper is None:
        pretext_wrapper = bool(getattr(getattr(config, "env", None), "use_wrapper", False))
    # the attention policy's kernels take edge widths up to 16 (cn_policy_create), i.e. horizons up to 7: say so here, by name, before the
    # simulator, the predictor's handle and the storage are built (the DS-RNN baseline takes widths up to 64)
    steps = int(getattr(getattr(config, "sim", None), "predict_steps", 5))
    named_base = base if base is not None else getattr(getattr(config, "robot", None), "policy", None)
    if env_name not in ("CrowdSimVarNum-v0", "CrowdSimVarNumCollect-v0") and named_base != "srnn" and 2 * (steps + 1) > 16:
        raise NotImplementedError("sim.predict_steps = %d gives spatial edges of width %d, and the attention-graph policy's kernels take at most 16 "
                                  "(predict_steps <= 7); base='srnn' takes widths up to 64" % (steps, 2 * (steps + 1)))
    envs = make_vec_envs(env_name, seed, num_processes, gamma, None, device, False, config=config, phase="train", pretext_wrapper=bool(pretext_wrapper),
                         predictor=predictor)
    # arguments.py:189, :206: use_self_attn, and sort_humans -- by default whatever the config's args say (it also decides the simulator's row order)
    if sort_humans is None:
        sort_humans = bool(getattr(getattr(config, "args", None), "sort_humans", True))
    # the simulator's row order follows config.args.sort_humans (config.to_env_config): the policy must read the observation the same way, and the
    # unsorted mode masks by `visible_masks`, which CrowdSimPred-v0's observation does not have (crowd_sim_pred.py:36-48) -- refuse both here,
    # before anything is allocated, rather than with a KeyError in the middle of the first rollout
    cfg_sort = bool(getattr(getattr(config, "args", None), "sort_humans", True))
    if bool(sort_humans) != cfg_sort:
        raise ValueError("train(sort_humans=%s) disagrees with config.args.sort_humans=%s, which decides the simulator's row order" % (sort_humans, cfg_sort))
    if not sort_humans and "visible_masks" not in envs.observation_space.spaces:
        raise ValueError("sort_humans=False needs the `visible_masks` observation, which %s does not provide" % env_name)
    base_kwargs = dict(env_name=env_name, num_processes=num_processes, num_mini_batch=num_mini_batch, seq_length=num_steps, use_self_attn=use_self_attn,
                       sort_humans=sort_humans, **network_kwargs(network))
    if env_name in ("CrowdSimPred-v0", "CrowdSimPredRealGST-v0"):
        base_kwargs["predict_steps"] = steps              # the edge width the network expects of this env is 2 (predict_steps + 1)
    if base is None:
        base = getattr(getattr(config, "robot", None), "policy", None)
        if base not in ("selfAttn_merge_srnn", "srnn"):
            base = "selfAttn_merge_srnn"
    actor_critic = Policy(envs.observation_space.spaces, envs.action_space, base_kwargs=base_kwargs, base=base).to(device)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        # identical weights on every rank (seeded above), but each env shard explores with its own action noise
        torch.cuda.manual_seed(seed + 1000003 * torch.distributed.get_rank())
    if not actor_critic.is_srnn_baseline:
        from ._abi import policy_dims
        policy_dims(actor_critic.base.dims)       # sizes outside the device box: refused here, before anything else is allocated
    rollouts = new_rollouts(actor_critic, num_steps, num_processes, envs.observation_space.spaces, envs.action_space)
    rollouts.to(device)
    if actor_critic.is_srnn_baseline:
        rollouts.materialize_edge_rnn()
    agent = PPO(actor_critic, clip_param, ppo_epoch, num_mini_batch, value_loss_coef, entropy_coef, lr=lr, eps=eps, max_grad_norm=max_grad_norm)
    obs = envs.reset_device()
    for k in rollouts.obs:
        rollouts.obs[k][0].copy_(obs[k].view_as(rollouts.obs[k][0]) if k != "visible_masks" else obs[k].to(torch.bool))
    stats = EpisodeStats(device)
    history = []
    first = 0
    if resume is not None:
        rank = torch.distributed.get_rank() if (torch.distributed.is_available() and torch.distributed.is_initialized()) else 0
        side = resume[:-3] + (".resume.pt" if rank == 0 else ".resume.rank%d.pt" % rank)
        first = load_checkpoint(resume, side, actor_critic, agent, envs, rollouts, stats, device)
    for j in range(first, num_updates):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        collect_rollout(envs, actor_critic, rollouts, stats)
        next_value = bootstrap_value(actor_critic, rollouts)
        rollouts.compute_returns(next_value, True, gamma, gae_lambda, False)
        torch.cuda.synchronize(device)
        t1 = time.perf_counter()
        # live (env, human) rows of the T x E samples the update trains on: the human-human block runs on these (see update_flops)
        live_rows = rollouts.obs["detected_human_num"][:num_steps].clamp(1, envs.human_num).sum()
        value_loss, action_loss, dist_entropy = agent.update(rollouts)
        rollouts.after_update()
        torch.cuda.synchronize(device)
        t2 = time.perf_counter()
        rec = dict(update=j, value_loss=value_loss, action_loss=action_loss, entropy=dist_entropy, rollout_s=t1 - t0, update_s=t2 - t1,
                   allreduce_ms=getattr(agent, "last_allreduce_ms", None), live_rows=int(live_rows.item()),
                   samples_per_s=num_steps * num_processes / (t2 - t0), **stats.pop())
        if eval_interval and ((j + 1) % eval_interval == 0 or j == num_updates - 1):
            rank = torch.distributed.get_rank() if (torch.distributed.is_available() and torch.distributed.is_initialized()) else 0
            if rank == 0:     # the other ranks go on to the next rollout and meet this one at its first collective
                t3 = time.perf_counter()
                rec["eval"] = evaluate_policy(actor_critic, env_name, config, seed, eval_cases, device, predictor=envs._pretext.pred if envs._pretext is not None else predictor)
                rec["eval_s"] = time.perf_counter() - t3
        history.append(rec)
        if log:
            log(rec)
        if save_dir is not None and ((save_interval and j % save_interval == 0) or j == num_updates - 1):
            save_checkpoint(save_dir, j, actor_critic, agent, envs, rollouts, stats, device)
    envs.close()
    return history, actor_critic
