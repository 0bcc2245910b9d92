"""GPU tests of the DS-RNN baseline (Policy(base='srnn')): the cn_srnn rollout forward against the reference's goldens in both arithmetic
modes, a T-step device rollout, the training path against an fp64 CPU graph, PPO.update against the reference, and train() end to end."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import srnn_util as SU  # noqa: E402

TAPS = ("edge_out", "attn", "weighted", "node_out", "actor_feat")


def _dev(z, keys, prefix=""):
    return {k: torch.from_numpy(z[prefix + k]).cuda() for k in keys}


def _handle(pol, E, mode):
    pol.srnn_gemm_mode = mode
    return pol._hip_srnn(E, torch.device("cuda", torch.cuda.current_device()))


@pytest.mark.parametrize("mode", ["bf16x3", "fp32"])
@pytest.mark.parametrize("path", SU.ACT_CASES, ids=SU.case_id)
def test_act_fixtures_through_cn_srnn_act(path, mode):
    """Value, action, log-prob, both hidden states and all taps within 1e-4 of the reference.  (1, 5, 2): less than one tile; (7, 20, 2): 147 edge
    rows, a ragged last tile and a temporal tile beside spatial ones; (3, 64, 2): 65 slots per env; D = 12."""
    z, meta = SU.load(path)
    E, H = meta["E"], meta["H"]
    pol, _, _ = SU.policy(meta, E)
    pol = pol.cuda()
    h = _handle(pol, E, mode)
    obs = _dev(z, SU.OBS_KEYS)
    node, edge, masks = (torch.from_numpy(z[k]).cuda() for k in ("hxs_node", "hxs_edge", "masks"))
    out = h.act(obs, node, edge, masks, eps=None)
    taps = h.taps(E)
    torch.cuda.synchronize()
    for k, ref in (("value", "value"), ("action", "action"), ("logp", "logp"), ("hxs", "hx_out"), ("edge_hxs", "edge_out")):
        np.testing.assert_allclose(out[k].cpu().numpy(), z[ref], atol=1e-4, err_msg=k)
    for k in TAPS:
        np.testing.assert_allclose(taps[k].cpu().numpy(), z[k], atol=1e-4, err_msg=k)
    # get_value returns the bits of act's value; the same call twice gives the same bits
    assert torch.equal(h.get_value(obs, node, edge, masks), out["value"])
    again = h.act(obs, node, edge, masks, eps=None)
    for k in out:
        assert torch.equal(out[k], again[k]), k
    # sampled mode: action = mean + std * eps, and its log-prob by the torch formula
    eps = torch.randn(E, 2, generator=torch.Generator().manual_seed(7)).cuda()
    smp = h.act(obs, node, edge, masks, eps=eps)
    std = pol.dist.logstd._bias.detach().view(1, 2).exp()
    np.testing.assert_allclose(smp["action"].cpu().numpy(), (out["action"] + std * eps).cpu().numpy(), atol=1e-6)
    lp = pol._log_prob(out["action"], std.expand(E, 2), smp["action"])
    np.testing.assert_allclose(smp["logp"].cpu().numpy(), lp.cpu().numpy(), atol=1e-5)
    assert torch.equal(smp["value"], out["value"]) and torch.equal(smp["edge_hxs"], out["edge_hxs"])
    # the Policy methods take the same handle
    with torch.no_grad():
        v, a, l, hx = pol.act(obs, {"human_node_rnn": node, "human_human_edge_rnn": edge}, masks, deterministic=True)
    assert torch.equal(v, out["value"]) and torch.equal(a, out["action"]) and torch.equal(hx["human_human_edge_rnn"], out["edge_hxs"])
    # in place: the new edge state over the old one
    e2 = edge.clone()
    inpl = h.act(obs, node, e2, masks, eps=None, out=dict(out, edge_hxs=e2, value=torch.empty_like(out["value"])))
    assert torch.equal(e2, again["edge_hxs"]) and torch.equal(inpl["value"], again["value"])


@pytest.mark.parametrize("path", SU.ROLLOUT_CASES, ids=SU.case_id)
def test_device_rollout_follows_the_reference(path):
    """T steps on the device from the fixture's first row, fed with the fixture's observations, masks and the reference's sampled actions only
    through the log-prob: values and log-probs of every step against the reference's records.  The recurrence compounds rounding, so the bar
    is max(1e-4, 4 d) with d = |fp32 - fp64| of the mirror's own CPU graph on this sequence (the rule of tests/test_gpu_gst_eval.py)."""
    z, meta = SU.load(path)
    T, E, H = meta["T"], meta["E"], meta["H"]
    pol, _, _ = SU.policy(meta, E)

    def cpu_graph(p, dt):
        node, edge = torch.from_numpy(z["hxs_node"][0]).to(dt), torch.from_numpy(z["hxs_edge0"]).to(dt)
        vals, lps = [], []
        with torch.no_grad():
            for s in range(T):
                obs = {k: torch.from_numpy(z["obs%d_%s" % (s, k)]).to(dt) for k in SU.OBS_KEYS}
                v, feat, node, edge = p.base.forward_sequence(obs, node, edge, torch.from_numpy(z["masks"][s]).to(dt), 1, E)
                mean = p.dist.fc_mean(feat)
                std = p.dist.logstd(torch.zeros_like(mean)).exp()
                vals.append(v); lps.append(p._log_prob(mean, std, torch.from_numpy(z["actions"][s]).to(dt)))
        return torch.stack(vals).double(), torch.stack(lps).double()

    v32, l32 = cpu_graph(pol, torch.float32)
    import copy
    v64, l64 = cpu_graph(copy.deepcopy(pol).double(), torch.float64)
    d = max(float((v32 - v64).abs().max()), float((l32 - l64).abs().max()))
    bar = max(1e-4, 4 * d)
    pol = pol.cuda()
    h = _handle(pol, E, "bf16x3")
    node, edge = torch.from_numpy(z["hxs_node"][0]).cuda(), torch.from_numpy(z["hxs_edge0"]).cuda()
    std = pol.dist.logstd._bias.detach().view(1, 2).exp().expand(E, 2)
    worst = 0.0
    for s in range(T):
        obs = _dev(z, SU.OBS_KEYS, "obs%d_" % s)
        out = h.act(obs, node, edge, torch.from_numpy(z["masks"][s]).cuda(), eps=None)
        lp = pol._log_prob(out["action"], std, torch.from_numpy(z["actions"][s]).cuda())
        worst = max(worst, float((out["value"].cpu() - torch.from_numpy(z["values"][s])).abs().max()),
                    float((lp.cpu() - torch.from_numpy(z["logp"][s])).abs().max()))
        np.testing.assert_allclose(out["hxs"].cpu().numpy(), z["hxs_node"][s + 1], atol=bar)
        node, edge = out["hxs"], out["edge_hxs"]
    print("srnn device rollout %s: d = %.3g, bar = %.3g, measured deviation = %.3g" % (SU.case_id(path), d, bar, worst))
    assert worst <= bar
    np.testing.assert_allclose(edge.cpu().numpy(), z["hxs_edge_last"], atol=bar)


@pytest.mark.parametrize("path", SU.SEQ_CASES, ids=SU.case_id)
def test_evaluate_actions_and_gradients_match_fp64_cpu_graph(path):
    import copy
    z, meta = SU.load(path)
    N, T = meta["N"], meta["T"]
    pol, _, _ = SU.policy(meta, N, 1, T)
    ref = copy.deepcopy(pol).double()
    pol = pol.cuda()

    def run(p, dev, dt):
        obs = {k: torch.from_numpy(z["obs_" + k]).to(device=dev, dtype=dt) for k in SU.OBS_KEYS}
        hxs = {"human_node_rnn": torch.from_numpy(z["hxs_node"]).to(device=dev, dtype=dt),
               "human_human_edge_rnn": torch.from_numpy(z["hxs_edge"]).to(device=dev, dtype=dt)}
        v, lp, ent, _ = p.evaluate_actions(obs, hxs, torch.from_numpy(z["masks"]).to(device=dev, dtype=dt), torch.from_numpy(z["actions"]).to(device=dev, dtype=dt))
        w = torch.linspace(-1, 1, v.numel(), dtype=dt, device=dev).view_as(v)
        ((v * w).sum() + (lp * w.flip(0)).sum() + ent).backward()
        return v.detach().cpu().double(), lp.detach().cpu().double()

    v, lp = run(pol, "cuda", torch.float32)
    v64, lp64 = run(ref, "cpu", torch.float64)
    np.testing.assert_allclose(v.numpy(), v64.numpy(), atol=1e-4)
    np.testing.assert_allclose(lp.numpy(), lp64.numpy(), atol=1e-4)
    np.testing.assert_allclose(v.numpy(), z["ev_value"], atol=1e-4)
    np.testing.assert_allclose(lp.numpy(), z["ev_logp"], atol=1e-4)
    gref = dict(ref.named_parameters())
    for name, p in pol.named_parameters():
        g64 = gref[name].grad
        if name.startswith(SU.DEAD):
            assert p.grad is None and g64 is None, name
            continue
        # the bar of tests/test_gpu_minibatch_step.py: 5e-4 of the tensor's largest entry + 1e-7 (spatial_edge_layer's bias has a gradient that
        # is zero up to rounding: the softmax does not see it)
        err = float((p.grad.cpu().double() - g64).abs().max())
        assert err <= 5e-4 * float(g64.abs().max()) + 1e-7, (name, err, float(g64.abs().max()))


@pytest.mark.parametrize("path", SU.ROLLOUT_CASES, ids=SU.case_id)
def test_ppo_update_on_the_gpu_matches_reference(path):
    from crowdnav_prediction_attngraph_amd import hip
    from crowdnav_prediction_attngraph_amd.ppo import PPO
    z, meta = SU.load(path)
    T, E, nmb = meta["T"], meta["E"], meta["nmb"]
    pol, ob_space, act_space = SU.policy(meta, E, nmb, T)
    pol = pol.cuda()
    before = {k: v.clone() for k, v in pol.state_dict().items()}
    ro = SU.fill_rollouts(z, meta, ob_space, act_space)
    ro.to(torch.device("cuda"))
    assert ro.edge_rnn_live and not hip.MinibatchStepper.supported(pol, ro)
    ro.compute_returns(torch.from_numpy(z["next_value"]).cuda(), True, 0.99, 0.95, False)
    np.testing.assert_allclose(ro.returns.cpu().numpy()[:-1], z["returns"][:-1], atol=1e-6)
    agent = PPO(pol, 0.2, meta["ppo_epoch"], nmb, 0.5, 0.0, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
    torch.manual_seed(meta["update_seed"])
    losses = agent.update(ro)
    np.testing.assert_allclose(losses, z["losses"], atol=1e-5)
    for k, t in pol.state_dict().items():
        flat = t.cpu().numpy().reshape(-1)
        smp = flat[np.linspace(0, flat.size - 1, min(flat.size, 256)).astype(np.int64)]
        np.testing.assert_allclose(smp, z["smp_" + k], atol=1e-5, err_msg=k)
        if k.startswith(SU.DEAD):
            assert torch.equal(t, before[k]), k
    # the rollout path sees the new weights
    obs = {k: ro.obs[k][0] for k in SU.OBS_KEYS}
    hxs = {k: v[0] for k, v in ro.recurrent_hidden_states.items()}
    with torch.no_grad():
        v_hip = pol.get_value(obs, hxs, ro.masks[0])
        v_ops, _, _, _ = pol.base.forward_sequence(obs, hxs["human_node_rnn"], hxs["human_human_edge_rnn"], ro.masks[0], 1, E)
    np.testing.assert_allclose(v_hip.cpu().numpy(), v_ops.cpu().numpy(), atol=1e-4)


def _sig(hist, pol):
    return ([(r["value_loss"], r["action_loss"], r["entropy"], r["eprewmean"], r["episodes"]) for r in hist],
            [float(p.detach().double().sum()) for p in pol.parameters()])


def test_train_end_to_end_is_reproducible_and_resumes(tmp_path):
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd.evaluation import evaluate_batched
    from crowdnav_prediction_attngraph_amd.policy import SRNNBase
    from crowdnav_prediction_attngraph_amd.trainer import train
    cfg = C.Config(**{"sim.human_num": 5})
    kw = dict(num_processes=8, num_steps=5, config=cfg, log=None, ppo_epoch=2, base="srnn")
    h1, p1 = train("CrowdSimVarNum-v0", num_updates=4, **kw)
    assert isinstance(p1.base, SRNNBase) and len(h1) == 4 and all(math.isfinite(r["value_loss"]) for r in h1)
    h2, p2 = train("CrowdSimVarNum-v0", num_updates=4, **kw)
    assert _sig(h1, p1) == _sig(h2, p2)
    for a, b in zip(p1.parameters(), p2.parameters()):
        assert torch.equal(a, b)
    d = str(tmp_path)
    ha, _ = train("CrowdSimVarNum-v0", num_updates=2, save_dir=d, **kw)
    hb, pb = train("CrowdSimVarNum-v0", num_updates=4, resume=d + "/checkpoints/00001.pt", **kw)
    assert _sig(ha + hb, pb) == _sig(h1, p1)
    for a, b in zip(p1.parameters(), pb.parameters()):
        assert torch.equal(a, b)
    m1 = evaluate_batched(p1, "CrowdSimVarNum-v0", cfg, 425, 8)
    m2 = evaluate_batched(p1, "CrowdSimVarNum-v0", cfg, 425, 8)
    assert m1 == m2


def test_train_follows_the_config_robot_policy():
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd.policy import AttnGraphBase, SRNNBase
    from crowdnav_prediction_attngraph_amd.trainer import train
    _, pol = train("CrowdSimVarNum-v0", num_processes=8, num_steps=5, num_updates=1, ppo_epoch=1, log=None,
                   config=C.Config(**{"sim.human_num": 5, "robot.policy": "srnn"}), eval_interval=1, eval_cases=4)
    assert isinstance(pol.base, SRNNBase)
    _, pol = train("CrowdSimVarNum-v0", num_processes=8, num_steps=5, num_updates=1, ppo_epoch=1, log=None, config=C.Config(**{"sim.human_num": 5}))
    assert isinstance(pol.base, AttnGraphBase)
