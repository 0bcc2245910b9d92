#!/usr/bin/env python3
"""Golden vectors for the DS-RNN baseline (`Policy(base='srnn')`, rl/networks/srnn_model.py): act with taps, evaluate_actions on [T, N]
sequences, one PPO.update on a synthetic rollout and the seeded-init checksums, all by the reference's own torch code on the CPU
(build container only; see _ref_import.py).  Same weights (policy_util.formula_state_dict), observations (synth_obs) and file layout as
make_golden_policy.py, whose helpers this imports.

One attribute the reference does not define is set here: srnn_model.py:378 reads `args.env_type`, which arguments.py lacks, so the
constructor raises AttributeError as shipped.  `args.env_type = 'crowd_sim'` selects the 7-wide robot node of the crowd-sim envs."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import as R  # noqa: E402
import policy_util as PU  # noqa: E402
import make_golden_policy as G  # noqa: E402

t = G.t


def build_srnn(env_name, E, H, D, nmb=1, T=1, formula=True):
    import torch
    from rl.networks.model import Policy
    args = G.ref_args(env_name, E, nmb, T)
    args.env_type = "crowd_sim"
    ob_space, act_space = G.spaces(H, D)
    torch.manual_seed(0)
    pol = Policy(ob_space.spaces, act_space, base_kwargs=args, base="srnn")
    shapes = {k: tuple(v.shape) for k, v in pol.state_dict().items()}
    if formula:
        pol.load_state_dict({k: torch.from_numpy(v) for k, v in PU.formula_state_dict(shapes).items()})
    return pol, args, shapes, ob_space, act_space


def _hooks(base, taps):
    return [base.attn.register_forward_hook(lambda m, i, o: taps.update(weighted=o[0].detach().numpy().copy(), attn=o[1].detach().numpy().copy())),
            base.humanNodeRNN.register_forward_hook(lambda m, i, o: taps.__setitem__("node_out", o[0].detach().numpy().copy()))]


def act_case(tag, env_name, E, H, D):
    import torch
    pol, args, shapes, _, _ = build_srnn(env_name, E, H, D)
    ob = PU.synth_obs(E, H, D, seed=3000 + E * 7 + H + D)
    rs = np.random.RandomState(41)
    hxs = {"human_node_rnn": rs.uniform(-1, 1, (E, 1, 128)).astype(np.float32),
           "human_human_edge_rnn": rs.uniform(-1, 1, (E, H + 1, 256)).astype(np.float32)}
    masks = np.ones((E, 1), np.float32)
    if E > 1:
        masks[1] = 0.0
    if E > 4:
        masks[E - 2] = 0.0
    taps = {}
    hooks = _hooks(pol.base, taps)
    with torch.no_grad():
        tob = {k: t(v) for k, v in ob.items()}
        value, action, logp, hx_out = pol.act(tob, {k: t(v) for k, v in hxs.items()}, t(masks), deterministic=True)
        _, actor_feat, _ = pol.base(tob, {k: t(v) for k, v in hxs.items()}, t(masks), infer=True)
        fixed_action = rs.uniform(-1.5, 1.5, (E, 2)).astype(np.float32)
        dist = pol.dist(actor_feat)
        logp_fixed = dist.log_probs(t(fixed_action))
        entropy = dist.entropy().mean()
    for h in hooks:
        h.remove()
    out = dict(ob)
    out.update(hxs_node=hxs["human_node_rnn"], hxs_edge=hxs["human_human_edge_rnn"], masks=masks, value=value.numpy(), action=action.numpy(),
               logp=logp.numpy(), hx_out=hx_out["human_node_rnn"].numpy().reshape(E, 1, 128),
               edge_out=hx_out["human_human_edge_rnn"].numpy().reshape(E, H + 1, 256), actor_feat=actor_feat.numpy().reshape(E, 256),
               fixed_action=fixed_action, logp_fixed=logp_fixed.numpy(), entropy=np.float32(entropy.item()),
               attn=taps["attn"].reshape(E, H), weighted=taps["weighted"].reshape(E, 256), node_out=taps["node_out"].reshape(E, 256),
               meta=np.array(json.dumps(dict(env_name=env_name, E=E, H=H, D=D, shapes={k: list(v) for k, v in shapes.items()}))))
    path = os.path.join(HERE, "srnn_act_%s.npz" % tag)
    np.savez_compressed(path, **out)
    print("srnn act %-10s value[0]=%.5f action[0]=%s -> %s (%.0f KB)" % (tag, out["value"][0, 0], out["action"][0], os.path.basename(path),
                                                                        os.path.getsize(path) / 1024))


def seq_case(tag, env_name, N, H, D, T):
    """evaluate_actions on a [T, N] slice with about 20 % zero masks (interior ones included: the reference splits the sequence there)."""
    import torch
    pol, args, shapes, _, _ = build_srnn(env_name, N, H, D, nmb=1, T=T)
    rs = np.random.RandomState(43)
    obs_seq = PU.synth_obs(T * N, H, D, seed=5000 + H + 10 * D)
    hxs = {"human_node_rnn": rs.uniform(-1, 1, (N, 1, 128)).astype(np.float32),
           "human_human_edge_rnn": rs.uniform(-1, 1, (N, H + 1, 256)).astype(np.float32)}
    masks_seq = np.ones((T * N, 1), np.float32)
    masks_seq[rs.choice(T * N, int(round(0.2 * T * N)), replace=False)] = 0.0     # 20 % zeros ...
    masks_seq[N + 1] = 0.0                                                        # ... one of them certainly at an interior step
    actions = rs.uniform(-1.5, 1.5, (T * N, 2)).astype(np.float32)
    with torch.no_grad():
        ev_value, ev_logp, ev_ent, ev_hx = pol.evaluate_actions({k: t(v) for k, v in obs_seq.items()}, {k: t(v) for k, v in hxs.items()}, t(masks_seq),
                                                                t(actions))
    out = {"obs_" + k: v for k, v in obs_seq.items()}
    out.update(hxs_node=hxs["human_node_rnn"], hxs_edge=hxs["human_human_edge_rnn"], masks=masks_seq, actions=actions, ev_value=ev_value.numpy(),
               ev_logp=ev_logp.numpy(), ev_entropy=np.float32(ev_ent.item()), ev_hx=ev_hx["human_node_rnn"].numpy().reshape(N, 1, 128),
               ev_edge=ev_hx["human_human_edge_rnn"].numpy().reshape(N, H + 1, 256),
               meta=np.array(json.dumps(dict(env_name=env_name, N=N, H=H, D=D, T=T, shapes={k: list(v) for k, v in shapes.items()}))))
    path = os.path.join(HERE, "srnn_seq_%s.npz" % tag)
    np.savez_compressed(path, **out)
    print("srnn seq %-10s value[0]=%.5f zero masks %d/%d -> %s (%.0f KB)" % (tag, out["ev_value"][0, 0], int((masks_seq == 0).sum()), T * N,
                                                                            os.path.basename(path), os.path.getsize(path) / 1024))


def rollout_case(tag, env_name, E, H, D, T, nmb):
    """A synthetic rollout through the reference's RolloutStorage / compute_returns / PPO.update (layout of make_golden_policy.rollout_case)."""
    import torch
    from rl.networks.storage import RolloutStorage
    from rl import ppo as ref_ppo
    pol, args, shapes, ob_space, act_space = build_srnn(env_name, E, H, D, nmb=nmb, T=T)
    rollouts = RolloutStorage(T, E, ob_space.spaces, act_space, 128, 256)
    rs = np.random.RandomState(47)
    obs_seq = [PU.synth_obs(E, H, D, seed=900 + s) for s in range(T + 1)]
    dones = rs.uniform(size=(T, E)) < 0.2
    rewards = rs.uniform(-1, 1, (T, E, 1)).astype(np.float32)
    node0 = rs.uniform(-1, 1, (E, 1, 128)).astype(np.float32)
    edge0 = rs.uniform(-1, 1, (E, H + 1, 256)).astype(np.float32)
    rollouts.recurrent_hidden_states["human_node_rnn"][0].copy_(t(node0))
    rollouts.recurrent_hidden_states["human_human_edge_rnn"][0].copy_(t(edge0))
    for k in rollouts.obs:
        if k in obs_seq[0]:
            rollouts.obs[k][0].copy_(t(obs_seq[0][k]))
    torch.manual_seed(123)
    actions_rec, logp_rec, value_rec = [], [], []
    for s in range(T):
        with torch.no_grad():
            ob = {k: rollouts.obs[k][s] for k in rollouts.obs}
            hx = {k: rollouts.recurrent_hidden_states[k][s] for k in rollouts.recurrent_hidden_states}
            value, action, logp, hx_new = pol.act(ob, hx, rollouts.masks[s])
        masks = t(np.where(dones[s], 0.0, 1.0).astype(np.float32).reshape(E, 1))
        nxt = {k: t(obs_seq[s + 1][k]) for k in obs_seq[s + 1]}
        nxt["visible_masks"] = torch.zeros(E, H, dtype=torch.bool)
        rollouts.insert(nxt, hx_new, action, logp, value, t(rewards[s]), masks, torch.ones(E, 1))
        actions_rec.append(action.numpy().copy()); logp_rec.append(logp.numpy().copy()); value_rec.append(value.numpy().copy())
    with torch.no_grad():
        ob = {k: rollouts.obs[k][-1] for k in rollouts.obs}
        hx = {k: rollouts.recurrent_hidden_states[k][-1] for k in rollouts.recurrent_hidden_states}
        next_value = pol.get_value(ob, hx, rollouts.masks[-1]).detach()
    rollouts.compute_returns(next_value, True, 0.99, 0.95, False)
    returns = rollouts.returns.numpy().copy()
    edge_last = rollouts.recurrent_hidden_states["human_human_edge_rnn"][-1].numpy().copy()
    agent = ref_ppo.PPO(pol, 0.2, 2, nmb, 0.5, 0.0, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
    torch.manual_seed(321)
    v_loss, a_loss, ent = agent.update(rollouts)
    sd_after = {k: v.detach().numpy().copy() for k, v in pol.state_dict().items()}
    out = dict(rewards=rewards, dones=dones, actions=np.array(actions_rec), logp=np.array(logp_rec), values=np.array(value_rec),
               next_value=next_value.numpy(), returns=returns, masks=rollouts.masks.numpy().copy(),
               hxs_node=rollouts.recurrent_hidden_states["human_node_rnn"].numpy().copy(), hxs_edge0=edge0, hxs_edge_last=edge_last,
               losses=np.array([v_loss, a_loss, ent], dtype=np.float64),
               meta=np.array(json.dumps(dict(env_name=env_name, E=E, H=H, D=D, T=T, nmb=nmb, act_seed=123, update_seed=321, ppo_epoch=2,
                                             shapes={k: list(v) for k, v in shapes.items()}))))
    for s in range(T + 1):
        for k, v in obs_seq[s].items():
            out["obs%d_%s" % (s, k)] = v
    for k, v in sd_after.items():
        flat = v.reshape(-1)
        out["chk_" + k] = np.array([float(np.sum(flat.astype(np.float64))), float(np.sum(np.abs(flat.astype(np.float64))))])
        out["smp_" + k] = flat[np.linspace(0, flat.size - 1, min(flat.size, 256)).astype(np.int64)].copy()
    path = os.path.join(HERE, "srnn_rollout_%s.npz" % tag)
    np.savez_compressed(path, **out)
    print("srnn rollout %-14s losses=%s -> %s (%.0f KB)" % (tag, out["losses"], os.path.basename(path), os.path.getsize(path) / 1024))


def init_case():
    """Parameter checksums of the reference Policy(base='srnn') right after construction under torch.manual_seed(0)."""
    out = {}
    for tag, env_name, H, D in (("varnum_h20", "CrowdSimVarNum-v0", 20, 2), ("pred_h20", "CrowdSimPred-v0", 20, 12)):
        pol, _, _, _, _ = build_srnn(env_name, 16, H, D, nmb=2, T=30, formula=False)
        for k, v in pol.state_dict().items():
            a = v.detach().numpy().astype(np.float64)
            out["%s/%s" % (tag, k)] = np.array([a.sum(), np.abs(a).sum(), float(a.ravel()[0]), float(a.ravel()[-1])])
    path = os.path.join(HERE, "srnn_init.npz")
    np.savez_compressed(path, **out)
    print("srnn init checksums -> %s (%.0f KB)" % (os.path.basename(path), os.path.getsize(path) / 1024))


def main():
    R.install()
    init_case()
    act_case("e4_h20_d2", "CrowdSimVarNum-v0", 4, 20, 2)
    act_case("e1_h5_d2", "CrowdSimVarNum-v0", 1, 5, 2)
    act_case("e4_h20_d12", "CrowdSimPred-v0", 4, 20, 12)
    act_case("e3_h64_d2", "CrowdSimVarNum-v0", 3, 64, 2)
    act_case("e7_h20_d2", "CrowdSimVarNum-v0", 7, 20, 2)
    seq_case("t3_n4_h20_d2", "CrowdSimVarNum-v0", 4, 20, 2, 3)
    seq_case("t4_n3_h10_d12", "CrowdSimPred-v0", 3, 10, 12, 4)
    rollout_case("e4_h5_t5", "CrowdSimVarNum-v0", 4, 5, 2, 5, 2)
    rollout_case("e4_h20_d12_t4", "CrowdSimPred-v0", 4, 20, 12, 4, 2)


if __name__ == "__main__":
    main()
