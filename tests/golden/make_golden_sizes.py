#!/usr/bin/env python3
"""Golden vectors for the four network-size flags of arguments.py:155-181 (human_node_rnn_size R, human_node_embedding_size M, attention_size A,
human_node_output_size O), produced by the reference's own Policy(base='selfAttn_merge_srnn') on the CPU (build container only; see
_ref_import.py).  Weights are policy_util.formula_state_dict over the reference's own shapes, so a file holds inputs and outputs, no weights.

  polsize_<tag>.npz   E = 5 envs x H = 20 humans: deterministic act and get_value on the first N rows (detected counts 1 .. H, one env with mask 0),
                      evaluate_actions on a [T = 3, N = 5] slice with interior done masks, and init_abs_sum per tensor under torch.manual_seed(0)
  rollsize_<tag>.npz  one whole PPO.update (same content as rollvar_*.npz; consumer: tests.test_policy_variants.check_update_against_the_reference)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import as R  # noqa: E402
import policy_util as PU  # noqa: E402
from make_golden_policy import ref_args, spaces, t, variant_obs  # noqa: E402

FLAGS = ("human_node_rnn_size", "human_node_embedding_size", "attention_size", "human_node_output_size")
# (tag, (R, M, A, O), env_name, D)
CASES = (("r64_m64_a32_o64", (64, 64, 32, 64), "CrowdSimVarNum-v0", 2),
         ("r256_m128_a128_o512", (256, 128, 128, 512), "CrowdSimVarNum-v0", 2),
         ("r192_m64_a48_o320", (192, 64, 48, 320), "CrowdSimVarNum-v0", 2),
         ("r128_m128_a64_o256_pred", (128, 128, 64, 256), "CrowdSimPred-v0", 12),
         ("r128_m64_a16_o256", (128, 64, 16, 256), "CrowdSimVarNum-v0", 2))


def sized_args(env_name, E, nmb, T, dims):
    a = ref_args(env_name, E, nmb, T)
    for f, v in zip(FLAGS, dims):
        setattr(a, f, v)
    return a


def size_case(tag, dims, env_name, D, N=5, H=20, T=3):
    import torch
    from rl.networks.model import Policy
    args = sized_args(env_name, N, 1, T, dims)
    ob_space, act_space = spaces(H, D)
    torch.manual_seed(0)
    pol = Policy(ob_space.spaces, act_space, base_kwargs=args, base="selfAttn_merge_srnn")
    init_sum = {k: float(v.double().abs().sum()) for k, v in pol.state_dict().items()}
    shapes = {k: tuple(v.shape) for k, v in pol.state_dict().items()}
    pol.load_state_dict({k: torch.from_numpy(v) for k, v in PU.formula_state_dict(shapes).items()})
    rs = np.random.RandomState(31)
    obs_seq = variant_obs(T * N, H, D, 5100 + dims[0] + dims[3], False)
    obs_seq["detected_human_num"][0], obs_seq["detected_human_num"][N - 1] = 1.0, float(H)      # act's N rows cover the counts 1 and H
    obs_seq["visible_masks"] = np.arange(H)[None, :] < obs_seq["detected_human_num"].reshape(-1, 1).astype(int)
    hxs = {"human_node_rnn": rs.uniform(-1, 1, (N, 1, dims[0])).astype(np.float32), "human_human_edge_rnn": np.zeros((N, H + 1, 256), np.float32)}
    masks_seq = np.ones((T * N, 1), np.float32)
    masks_seq[1] = 0.0                   # act: one env starts from a zeroed state
    masks_seq[N + 2] = 0.0               # evaluate_actions: done masks in the interior of the sequence
    masks_seq[2 * N + 4] = 0.0
    actions = rs.uniform(-1.5, 1.5, (T * N, 2)).astype(np.float32)
    with torch.no_grad():
        first = {k: t(v[:N]) for k, v in obs_seq.items()}
        h0 = lambda: {k: t(v.copy()) for k, v in hxs.items()}        # the reference writes the new state into the dict it was given: a fresh one per call
        value, action, logp, hx_out = pol.act(first, h0(), t(masks_seq[:N]), deterministic=True)
        gv = pol.get_value(first, h0(), t(masks_seq[:N]))
        _, actor_feat, _ = pol.base(first, h0(), t(masks_seq[:N]), infer=True)
        ev_value, ev_logp, ev_ent, ev_hx = pol.evaluate_actions({k: t(v) for k, v in obs_seq.items()}, h0(), t(masks_seq), t(actions))
    out = {"obs_" + k: v for k, v in obs_seq.items()}
    out.update(hxs_node=hxs["human_node_rnn"], masks=masks_seq, actions=actions, value=value.numpy(), action=action.numpy(), logp=logp.numpy(),
               get_value=gv.numpy(), hx_out=hx_out["human_node_rnn"].numpy(), actor_feat=actor_feat.numpy(),
               ev_value=ev_value.numpy(), ev_logp=ev_logp.numpy(), ev_entropy=np.float32(ev_ent.item()), ev_hx=ev_hx["human_node_rnn"].numpy(),
               meta=np.array(json.dumps(dict(env_name=env_name, N=N, H=H, D=D, T=T, dims=list(dims), use_self_attn=True, sort_humans=True,
                                             shapes={k: list(v) for k, v in shapes.items()}, init_abs_sum=init_sum))))
    path = os.path.join(HERE, "polsize_%s.npz" % tag)
    np.savez_compressed(path, **out)
    print("size %-26s value[0]=%.5f -> %s (%.0f KB)" % (tag, out["value"][0, 0], os.path.basename(path), os.path.getsize(path) / 1024))


def rollout_size_case(tag, dims, env_name, E, H, D, T, nmb):
    """make_golden_policy.rollout_variant_case with the four size flags set: the storage's node state is [.., R]."""
    import torch
    from rl.networks.model import Policy
    from rl.networks.storage import RolloutStorage
    from rl import ppo as ref_ppo
    args = sized_args(env_name, E, nmb, T, dims)
    ob_space, act_space = spaces(H, D)
    torch.manual_seed(0)
    pol = Policy(ob_space.spaces, act_space, base_kwargs=args, base="selfAttn_merge_srnn")
    shapes = {k: tuple(v.shape) for k, v in pol.state_dict().items()}
    pol.load_state_dict({k: torch.from_numpy(v) for k, v in PU.formula_state_dict(shapes).items()})
    rollouts = RolloutStorage(T, E, ob_space.spaces, act_space, dims[0], 256)
    rs = np.random.RandomState(23)
    obs_seq = [variant_obs(E, H, D, 900 + s, False) for s in range(T + 1)]
    dones = rs.uniform(size=(T, E)) < 0.15
    rewards = rs.uniform(-1, 1, (T, E, 1)).astype(np.float32)
    for k in rollouts.obs:
        rollouts.obs[k][0].copy_(t(obs_seq[0][k]))
    torch.manual_seed(123)
    for s in range(T):
        with torch.no_grad():
            ob = {k: rollouts.obs[k][s] for k in rollouts.obs}
            hx = {k: rollouts.recurrent_hidden_states[k][s] for k in rollouts.recurrent_hidden_states}
            value, action, logp, hx_new = pol.act(ob, hx, rollouts.masks[s])
        masks = t(np.where(dones[s], 0.0, 1.0).astype(np.float32).reshape(E, 1))
        rollouts.insert({k: t(v) for k, v in obs_seq[s + 1].items()}, hx_new, action, logp, value, t(rewards[s]), masks, torch.ones(E, 1))
    with torch.no_grad():
        ob = {k: rollouts.obs[k][-1] for k in rollouts.obs}
        hx = {k: rollouts.recurrent_hidden_states[k][-1] for k in rollouts.recurrent_hidden_states}
        next_value = pol.get_value(ob, hx, rollouts.masks[-1]).detach()
    rollouts.compute_returns(next_value, True, 0.99, 0.95, False)
    out = dict(rewards=rewards, actions=rollouts.actions.numpy().copy(), logp=rollouts.action_log_probs.numpy().copy(), values=rollouts.value_preds.numpy().copy(),
               next_value=next_value.numpy(), returns=rollouts.returns.numpy().copy(), masks=rollouts.masks.numpy().copy(),
               hxs_node=rollouts.recurrent_hidden_states["human_node_rnn"].numpy().copy())
    agent = ref_ppo.PPO(pol, 0.2, 2, nmb, 0.5, 0.0, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
    torch.manual_seed(321)
    v_loss, a_loss, ent = agent.update(rollouts)
    out["losses"] = np.array([v_loss, a_loss, ent], dtype=np.float64)
    for k, v in pol.state_dict().items():
        flat = v.detach().numpy().reshape(-1)
        out["smp_" + k] = flat[np.linspace(0, flat.size - 1, min(flat.size, 256)).astype(np.int64)].copy()
        out["chk_" + k] = np.array([float(flat.astype(np.float64).sum()), float(np.abs(flat.astype(np.float64)).sum())])
    for s in range(T + 1):
        for k, v in obs_seq[s].items():
            out["obs%d_%s" % (s, k)] = v
    out["meta"] = np.array(json.dumps(dict(env_name=env_name, E=E, N=E, H=H, D=D, T=T, nmb=nmb, dims=list(dims), use_self_attn=True, sort_humans=True,
                                           update_seed=321, ppo_epoch=2, shapes={k: list(v) for k, v in shapes.items()})))
    path = os.path.join(HERE, "rollsize_%s.npz" % tag)
    np.savez_compressed(path, **out)
    print("rollout size %-22s losses=%s -> %s (%.0f KB)" % (tag, out["losses"], os.path.basename(path), os.path.getsize(path) / 1024))


def main():
    R.install()
    for tag, dims, env_name, D in CASES:
        size_case(tag, dims, env_name, D)
    rollout_size_case("r192_m64_a48_o320_e4_h8_t5", (192, 64, 48, 320), "CrowdSimVarNum-v0", 4, 8, 2, 5, 2)


if __name__ == "__main__":
    main()
