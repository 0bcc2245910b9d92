"""CPU tests of the DS-RNN baseline mirror (Policy(base='srnn') / RolloutStorage / PPO) against golden outputs of the reference's own
`Policy(base='srnn')` (tests/golden/make_golden_srnn.py)."""
import os

import numpy as np
import pytest
import torch

from crowdnav_prediction_attngraph_amd.policy import Policy, SRNNBase, make_spaces
from crowdnav_prediction_attngraph_amd.ppo import PPO
from crowdnav_prediction_attngraph_amd.storage import RolloutStorage
from tests import srnn_util as SU
from tests.golden_util import GOLDEN


def test_state_dict_keys_shapes_and_order_match_reference():
    z, meta = SU.load(SU.ACT_CASES[0])
    pol, _, _ = SU.policy(meta, meta["E"], formula=False)
    assert isinstance(pol.base, SRNNBase)
    assert [(k, list(v.shape)) for k, v in pol.state_dict().items()] == [(k, list(v)) for k, v in meta["shapes"].items()]
    assert 970000 < sum(p.numel() for p in pol.parameters()) < 980000      # 974k


@pytest.mark.parametrize("tag,env_name,H,D", [("varnum_h20", "CrowdSimVarNum-v0", 20, 2), ("pred_h20", "CrowdSimPred-v0", 20, 12)])
def test_seeded_init_matches_reference(tag, env_name, H, D):
    """Same construction order -> same RNG consumption -> the reference's initial weights (orthogonal_ goes through LAPACK QR, whose last
    bits depend on the BLAS thread count: the tolerance of tests/test_host_policy.py)."""
    ref = np.load(os.path.join(GOLDEN, "srnn_init.npz"))
    torch.manual_seed(0)
    pol, _, _ = SU.policy(dict(H=H, D=D, env_name=env_name), 16, 2, 30, formula=False)
    for k, v in pol.state_dict().items():
        a = v.detach().numpy().astype(np.float64)
        got = np.array([a.sum(), np.abs(a).sum(), float(a.ravel()[0]), float(a.ravel()[-1])])
        np.testing.assert_allclose(got, ref["%s/%s" % (tag, k)], rtol=1e-6, atol=2e-5, err_msg=k)


@pytest.mark.parametrize("path", SU.ACT_CASES, ids=SU.case_id)
def test_cpu_act_and_taps_match_reference_golden(path):
    z, meta = SU.load(path)
    E, H = meta["E"], meta["H"]
    pol, _, _ = SU.policy(meta, E)
    obs = {k: torch.from_numpy(z[k]) for k in SU.OBS_KEYS}
    hxs = {"human_node_rnn": torch.from_numpy(z["hxs_node"]), "human_human_edge_rnn": torch.from_numpy(z["hxs_edge"])}
    masks = torch.from_numpy(z["masks"])
    value, action, logp, hx = pol.act(obs, hxs, masks, deterministic=True)
    np.testing.assert_allclose(value.numpy(), z["value"], atol=2e-5)
    np.testing.assert_allclose(action.numpy(), z["action"], atol=2e-5)
    np.testing.assert_allclose(logp.numpy(), z["logp"], atol=2e-5)
    np.testing.assert_allclose(hx["human_node_rnn"].numpy(), z["hx_out"], atol=2e-5)
    assert hx["human_human_edge_rnn"].shape == (E, H + 1, 256)
    np.testing.assert_allclose(hx["human_human_edge_rnn"].numpy(), z["edge_out"], atol=2e-5)
    np.testing.assert_allclose(pol.get_value(obs, hxs, masks).numpy(), z["value"], atol=2e-5)
    taps = {}
    with torch.no_grad():
        _, feat, _, _ = pol.base.forward_sequence(obs, hxs["human_node_rnn"], hxs["human_human_edge_rnn"], masks, 1, E, taps=taps)
        mean = pol.dist.fc_mean(feat)
        std = pol.dist.logstd(torch.zeros_like(mean)).exp()
        logp_fixed = pol._log_prob(mean, std, torch.from_numpy(z["fixed_action"]))
    np.testing.assert_allclose(logp_fixed.numpy(), z["logp_fixed"], atol=2e-5)
    for k in ("edge_out", "attn", "weighted", "node_out", "actor_feat"):
        np.testing.assert_allclose(taps[k].numpy(), z[k], atol=2e-5, err_msg=k)
    np.testing.assert_allclose(taps["attn"].sum(-1).numpy(), 1.0, atol=1e-5)         # softmax over ALL H slots, padded humans included


@pytest.mark.parametrize("path", SU.SEQ_CASES, ids=SU.case_id)
def test_cpu_evaluate_actions_matches_reference_golden(path):
    """The fixtures hold zero masks at interior steps: masking the state at every step equals the reference's split of the sequence."""
    z, meta = SU.load(path)
    N, T = meta["N"], meta["T"]
    assert (z["masks"].reshape(T, N)[1:] == 0).any()
    pol, _, _ = SU.policy(meta, N, 1, T)
    obs = {k: torch.from_numpy(z["obs_" + k]) for k in SU.OBS_KEYS}
    hxs = {"human_node_rnn": torch.from_numpy(z["hxs_node"]), "human_human_edge_rnn": torch.from_numpy(z["hxs_edge"])}
    with torch.no_grad():
        v, lp, ent, hx = pol.evaluate_actions(obs, hxs, torch.from_numpy(z["masks"]), torch.from_numpy(z["actions"]))
    np.testing.assert_allclose(v.numpy(), z["ev_value"], atol=2e-5)
    np.testing.assert_allclose(lp.numpy(), z["ev_logp"], atol=2e-5)
    assert float(ent) == pytest.approx(float(z["ev_entropy"]), abs=1e-6)
    np.testing.assert_allclose(hx["human_node_rnn"].numpy(), z["ev_hx"], atol=2e-5)
    np.testing.assert_allclose(hx["human_human_edge_rnn"].numpy(), z["ev_edge"], atol=2e-5)


@pytest.mark.parametrize("path", SU.ROLLOUT_CASES, ids=SU.case_id)
def test_ppo_update_matches_reference(path):
    """compute_returns and one whole PPO.update (2 epochs, the reference's torch.randperm draws) against the reference's losses and <= 256
    sampled entries of every post-update tensor at 1e-5; the three modules no gradient reaches come out bit-unchanged."""
    z, meta = SU.load(path)
    T, E, nmb = meta["T"], meta["E"], meta["nmb"]
    pol, ob_space, act_space = SU.policy(meta, E, nmb, T)
    before = {k: v.clone() for k, v in pol.state_dict().items()}
    ro = SU.fill_rollouts(z, meta, ob_space, act_space)
    np.testing.assert_array_equal(ro.masks.numpy(), z["masks"])
    ro.compute_returns(torch.from_numpy(z["next_value"]), True, 0.99, 0.95, False)
    np.testing.assert_allclose(ro.returns.numpy()[:-1], z["returns"][:-1], atol=1e-6)
    agent = PPO(pol, 0.2, meta["ppo_epoch"], nmb, 0.5, 0.0, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
    torch.manual_seed(meta["update_seed"])
    losses = agent.update(ro)
    np.testing.assert_allclose(losses, z["losses"], atol=1e-5)
    moved = 0
    for k, t in pol.state_dict().items():
        flat = t.numpy().reshape(-1)
        smp = flat[np.linspace(0, flat.size - 1, min(flat.size, 256)).astype(np.int64)]
        np.testing.assert_allclose(smp, z["smp_" + k], atol=1e-5, err_msg=k)
        a = flat.astype(np.float64)
        np.testing.assert_allclose([a.sum(), np.abs(a).sum()], z["chk_" + k], rtol=2e-6, atol=2e-4, err_msg=k)
        if k.startswith(SU.DEAD):
            assert torch.equal(t, before[k]), k
        else:
            moved += int(not torch.equal(t, before[k]))
    assert moved > 20


def test_storage_keeps_live_edge_rows():
    z, meta = SU.load(SU.ROLLOUT_CASES[0])
    T, E, H = meta["T"], meta["E"], meta["H"]
    ob_space, act_space = make_spaces(H, meta["D"])
    ro = SU.fill_rollouts(z, meta, ob_space, act_space)
    edge = ro.recurrent_hidden_states["human_human_edge_rnn"]
    assert ro.edge_rnn_live and edge.shape == (T + 1, E, H + 1, 256) and edge.is_contiguous()
    np.testing.assert_array_equal(edge[0].numpy(), z["hxs_edge0"])
    for s in range(1, T):
        assert float(edge[s].min()) == float(edge[s].max()) == float(s)
    np.testing.assert_array_equal(edge[T].numpy(), z["hxs_edge_last"])
    torch.manual_seed(3)
    perm = torch.randperm(E)
    torch.manual_seed(3)
    for b, sample in enumerate(ro.recurrent_generator(torch.zeros(T, E, 1), meta["nmb"])):
        idx = perm[b * (E // meta["nmb"]):(b + 1) * (E // meta["nmb"])]
        assert torch.equal(sample[1]["human_human_edge_rnn"], edge[0, idx])
        assert torch.equal(sample[1]["human_node_rnn"], ro.recurrent_hidden_states["human_node_rnn"][0, idx])
    ro.to("cpu")
    assert ro.edge_rnn_live and torch.equal(ro.recurrent_hidden_states["human_human_edge_rnn"][T], torch.from_numpy(z["hxs_edge_last"]))
    ro.after_update()
    np.testing.assert_array_equal(ro.recurrent_hidden_states["human_human_edge_rnn"][0].numpy(), z["hxs_edge_last"])


def test_attention_graph_storage_still_holds_the_zero_view():
    T, E, H = 3, 4, 5
    ob_space, act_space = make_spaces(H, 2)
    ro = RolloutStorage(T, E, ob_space.spaces, act_space, 128, 256)
    pol = Policy(ob_space.spaces, act_space, base="selfAttn_merge_srnn", base_kwargs=dict(num_processes=E))
    obs = {k: torch.zeros(E, *ob_space.spaces[k].shape) for k in SU.OBS_KEYS}
    obs["detected_human_num"] += 2.0
    _, action, logp, hx = pol.act(obs, {"human_node_rnn": torch.zeros(E, 1, 128)}, torch.ones(E, 1))
    for _ in range(2):
        ro.insert(obs, hx, action, logp, torch.zeros(E, 1), torch.zeros(E, 1), torch.ones(E, 1), torch.ones(E, 1))
    ro.after_update()
    ro.to("cpu")
    edge = ro.recurrent_hidden_states["human_human_edge_rnn"]
    assert not ro.edge_rnn_live and edge.shape == (T + 1, E, H + 1, 256) and set(edge.stride()) == {0} and float(edge.sum()) == 0.0
    for sample in ro.recurrent_generator(torch.zeros(T, E, 1), 2):
        assert set(sample[1]["human_human_edge_rnn"].stride()) == {0}


def test_other_bases_behave_as_before():
    ob_space, act_space = make_spaces(5, 2)
    assert type(Policy(ob_space.spaces, act_space).base).__name__ == "AttnGraphBase"
    assert type(Policy(ob_space.spaces, act_space, base="selfAttn_merge_srnn").base).__name__ == "AttnGraphBase"
    with pytest.raises(NotImplementedError):
        Policy(ob_space.spaces, act_space, base="mlp")
    with pytest.raises(NotImplementedError):
        Policy(ob_space.spaces, act_space, base="srnn", base_kwargs=dict(human_human_edge_rnn_size=128))
