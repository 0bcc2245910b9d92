"""The four network-size flags of arguments.py:155-181 -- human_node_rnn_size R, human_node_embedding_size M, attention_size A,
human_node_output_size O -- on the host mirror, against outputs of the reference's own Policy at five (R, M, A, O) tuples (tests/golden/polsize_*.npz,
rollsize_*.npz: tests/golden/make_golden_sizes.py, build container).  CPU: the torch-op mirror, the seeded init, one PPO.update, the refusals and
the plumbing that needs no device.  -m gpu (tests/test_gpu_policy_sizes.py): the HIP path on the same vectors."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from crowdnav_prediction_attngraph_amd import _abi as A
from crowdnav_prediction_attngraph_amd.policy import Policy, make_spaces
from tests import policy_util as PU
from tests.golden_util import GOLDEN
from tests.test_policy_variants import check_update_against_the_reference

PATHS = sorted(glob.glob(os.path.join(GOLDEN, "polsize_*.npz")))
ROLL = sorted(glob.glob(os.path.join(GOLDEN, "rollsize_*.npz")))
FLAGS = ("human_node_rnn_size", "human_node_embedding_size", "attention_size", "human_node_output_size")
TUPLES = [(64, 64, 32, 64), (256, 128, 128, 512), (192, 64, 48, 320), (128, 128, 64, 256), (128, 64, 16, 256)]


def size_kwargs(dims):
    return dict(zip(FLAGS, dims))


def build(meta, N=None, nmb=1):
    ob_space, act_space = make_spaces(meta["H"], meta["D"])
    kw = dict(env_name=meta["env_name"], num_processes=N or meta["N"], num_mini_batch=nmb, seq_length=meta["T"], **size_kwargs(meta["dims"]))
    torch.manual_seed(0)
    return Policy(ob_space.spaces, act_space, base="selfAttn_merge_srnn", base_kwargs=kw)


def load_formula_weights(pol, meta):
    pol.load_state_dict({k: torch.from_numpy(v) for k, v in PU.formula_state_dict({k: tuple(v) for k, v in meta["shapes"].items()}).items()})
    return pol


def inputs(z, meta, device="cpu", n=None):
    keys = ("robot_node", "temporal_edges", "spatial_edges", "detected_human_num", "visible_masks")
    obs = {k: torch.from_numpy(z["obs_" + k][:n] if n else z["obs_" + k]).to(device) for k in keys}
    hxs = {"human_node_rnn": torch.from_numpy(z["hxs_node"]).to(device), "human_human_edge_rnn": torch.zeros(meta["N"], meta["H"] + 1, 256, device=device)}
    return obs, hxs


def test_the_five_tuples_and_one_update_fixture_exist():
    assert sorted(tuple(json.loads(str(np.load(p)["meta"]))["dims"]) for p in PATHS) == sorted(TUPLES)
    assert len(ROLL) == 1 and json.loads(str(np.load(ROLL[0])["meta"]))["dims"] == [192, 64, 48, 320]
    assert sum(json.loads(str(np.load(p)["meta"]))["D"] == 12 for p in PATHS) == 1
    for p in PATHS + ROLL:
        assert os.path.getsize(p) < 842890, p


@pytest.mark.parametrize("path", PATHS, ids=lambda p: os.path.basename(p)[8:-4])
def test_sized_state_dict_and_seeded_init_match_the_reference(path):
    z = np.load(path)
    meta = json.loads(str(z["meta"]))
    pol = build(meta)
    assert [(k, list(v.shape)) for k, v in pol.state_dict().items()] == [(k, list(v)) for k, v in meta["shapes"].items()]
    for k, v in pol.state_dict().items():       # same construction order -> same draws of torch.manual_seed(0)
        np.testing.assert_allclose(float(v.double().abs().sum()), meta["init_abs_sum"][k], rtol=1e-5, atol=1e-6, err_msg=k)
    assert pol.base.dims == tuple(meta["dims"])


@pytest.mark.parametrize("path", PATHS, ids=lambda p: os.path.basename(p)[8:-4])
def test_sized_cpu_mirror_matches_the_reference(path):
    z = np.load(path)
    meta = json.loads(str(z["meta"]))
    N, R = meta["N"], meta["dims"][0]
    det = z["obs_detected_human_num"][:N].reshape(-1)
    assert det.min() == 1 and det.max() == meta["H"] and (z["masks"][:N] == 0).sum() == 1 and (z["masks"][N:] == 0).sum() == 2
    pol = load_formula_weights(build(meta), meta)
    obs, hxs = inputs(z, meta, n=N)
    masks = torch.from_numpy(z["masks"][:N])
    value, action, logp, hx = pol.act(obs, hxs, masks, deterministic=True)
    assert hx["human_node_rnn"].shape == (N, 1, R)
    np.testing.assert_allclose(value.numpy(), z["value"], atol=2e-5)
    np.testing.assert_allclose(action.numpy(), z["action"], atol=2e-5)
    np.testing.assert_allclose(logp.numpy(), z["logp"], atol=2e-5)
    np.testing.assert_allclose(hx["human_node_rnn"].numpy(), z["hx_out"], atol=2e-5)
    np.testing.assert_allclose(pol.get_value(obs, hxs, masks).numpy(), z["get_value"], atol=2e-5)
    obs, hxs = inputs(z, meta)
    ev_value, ev_logp, ev_ent, ev_hx = pol.evaluate_actions(obs, hxs, torch.from_numpy(z["masks"]), torch.from_numpy(z["actions"]))
    np.testing.assert_allclose(ev_value.detach().numpy(), z["ev_value"], atol=2e-5)
    np.testing.assert_allclose(ev_logp.detach().numpy(), z["ev_logp"], atol=2e-5)
    np.testing.assert_allclose(float(ev_ent), float(z["ev_entropy"]), atol=1e-6)
    np.testing.assert_allclose(ev_hx["human_node_rnn"].detach().numpy().reshape(N, -1), z["ev_hx"].reshape(N, -1), atol=2e-5)
    (ev_value.sum() + ev_logp.sum()).backward()
    no_grad = [k for k, p in pol.named_parameters() if p.grad is None]
    assert no_grad == ["base.human_node_final_linear.weight", "base.human_node_final_linear.bias"], no_grad   # unused in the reference too


def filled_rollouts(z, meta, pol, device="cpu"):
    """tests.test_policy_variants.filled_rollouts with the node state as wide as the policy's GRU (trainer.new_rollouts)."""
    from crowdnav_prediction_attngraph_amd.trainer import new_rollouts
    T, E = meta["T"], meta["E"]
    ob_space, act_space = make_spaces(meta["H"], meta["D"])
    ro = new_rollouts(pol, T, E, ob_space.spaces, act_space)
    for s in range(T + 1):
        for k in ro.obs:
            ro.obs[k][s].copy_(torch.from_numpy(z["obs%d_%s" % (s, k)]).view_as(ro.obs[k][s]))
    ro.recurrent_hidden_states["human_node_rnn"].copy_(torch.from_numpy(z["hxs_node"]))
    ro.actions.copy_(torch.from_numpy(z["actions"])); ro.action_log_probs.copy_(torch.from_numpy(z["logp"]))
    ro.value_preds.copy_(torch.from_numpy(z["values"])); ro.rewards.copy_(torch.from_numpy(z["rewards"])); ro.masks.copy_(torch.from_numpy(z["masks"]))
    if device != "cpu":
        ro.to(torch.device(device))
    return ro


def update_policy(meta):
    ob_space, act_space = make_spaces(meta["H"], meta["D"])
    pol = Policy(ob_space.spaces, act_space, base="selfAttn_merge_srnn",
                 base_kwargs=dict(env_name=meta["env_name"], num_processes=meta["E"], num_mini_batch=meta["nmb"], seq_length=meta["T"], **size_kwargs(meta["dims"])))
    return load_formula_weights(pol, meta)


def test_sized_ppo_update_matches_the_reference():
    """rl/ppo/ppo.py:36-101 at (192, 64, 48, 320): returns, the three losses and every tensor after two epochs x two minibatches, at the bars of
    tests/test_policy_variants.py."""
    z = np.load(ROLL[0])
    meta = json.loads(str(z["meta"]))
    pol = update_policy(meta)
    ro = filled_rollouts(z, meta, pol)
    assert ro.recurrent_hidden_states["human_node_rnn"].shape == (meta["T"] + 1, meta["E"], 1, 192)
    check_update_against_the_reference(z, meta, pol, ro)


def test_an_edge_size_other_than_256_is_refused_naming_the_reference():
    ob_space, act_space = make_spaces(5, 2)
    with pytest.raises(NotImplementedError, match="reference itself cannot run"):
        Policy(ob_space.spaces, act_space, base="selfAttn_merge_srnn", base_kwargs=dict(human_human_edge_rnn_size=128))


def test_sizes_outside_the_device_box_run_on_the_cpu_and_are_refused_for_a_device_handle():
    ob_space, act_space = make_spaces(5, 2)
    torch.manual_seed(3)
    pol = Policy(ob_space.spaces, act_space, base="selfAttn_merge_srnn", base_kwargs=size_kwargs((96, 40, 7, 100)))
    ob = {k: torch.from_numpy(v) for k, v in PU.synth_obs(3, 5, 2, seed=5).items()}
    hxs = {"human_node_rnn": torch.zeros(3, 1, 96), "human_human_edge_rnn": torch.zeros(3, 6, 256)}
    value, action, logp, hx = pol.act(ob, hxs, torch.ones(3, 1), deterministic=True)
    assert value.shape == (3, 1) and hx["human_node_rnn"].shape == (3, 1, 96) and torch.isfinite(action).all()
    # the refusal is the Python guard's: it names the box and comes before the handle asks for a device
    with pytest.raises(NotImplementedError, match=r"outside the device box.*\{64, 128, 192, 256\}.*\{64, 128\}.*\[64, 512\].*\[1, 256\]"):
        pol.base.make_hip_handle(3, "cuda:0")
    for bad in ((96, 64, 64, 256), (128, 32, 64, 256), (128, 64, 0, 256), (128, 64, 257, 256), (128, 64, 64, 576), (128, 64, 64, 96)):
        with pytest.raises(NotImplementedError, match="outside the device box"):
            A.policy_dims(bad)
    for ok in TUPLES + [(128, 64, 1, 64), (256, 128, 256, 512)]:
        assert A.policy_dims(ok).astuple() == ok


def test_default_dims_are_one_policy_dims():
    d = A.policy_dims(None)
    assert d == A.policy_dims(A.DEFAULT_DIMS) == A.policy_dims({}) == A.policy_dims(A.PolicyDims(128, 64, 64, 256)) and d.astuple() == (128, 64, 64, 256)
    assert A.policy_dims(dict(attention_size=48)).astuple() == (128, 64, 48, 256)
    assert d != A.policy_dims((128, 64, 48, 256))
    with pytest.raises(KeyError):
        A.policy_dims(dict(rnn=64))
    ob_space, act_space = make_spaces(5, 2)
    assert Policy(ob_space.spaces, act_space, base="selfAttn_merge_srnn", base_kwargs=None).base.dims == A.DEFAULT_DIMS


def test_train_network_flags_reach_the_policy_and_the_storage():
    from crowdnav_prediction_attngraph_amd.trainer import NETWORK_FLAGS, network_kwargs, new_rollouts
    assert NETWORK_FLAGS == FLAGS and network_kwargs(None) == {}
    with pytest.raises(KeyError, match="human_human_edge_rnn_size"):
        network_kwargs(dict(human_human_edge_rnn_size=128))
    kw = network_kwargs(dict(human_node_rnn_size=192, human_node_output_size=320, attention_size=48))
    ob_space, act_space = make_spaces(5, 2)
    pol = Policy(ob_space.spaces, act_space, base="selfAttn_merge_srnn", base_kwargs=dict(env_name="CrowdSimVarNum-v0", num_processes=8, **kw))
    assert pol.base.dims == (192, 64, 48, 320)
    ro = new_rollouts(pol, 4, 8, ob_space.spaces, act_space)
    assert ro.recurrent_hidden_states["human_node_rnn"].shape == (5, 8, 1, 192)
    assert tuple(pol.dist.fc_mean.weight.shape) == (2, 320)
