"""The binding layer of the device handles on a machine without a GPU: the one call helper, the shared prologue and teardown of the four
handle wrappers, the rollout contract of Policy on CPU tensors for both bases, and the import surface of `hip`."""
import ctypes as C

import pytest

from crowdnav_prediction_attngraph_amd import _abi as A

torch = pytest.importorskip("torch")

# dir() of the hip module before it was split by concern, underscore names dropped
HIP_NAMES = ['A', 'C', 'Embed0', 'GRUSequence', 'HHAttention', 'HHBlockFused', 'HRAttention', 'HipEnvBatch', 'HipGST', 'HipLinear', 'HipPolicy',
             'HipSrnn', 'MinibatchStepper', 'PPOLoss', 'RightMatmul', 'RnSequence', 'SmallMM', 'SrnnEdgeSequence', 'StepStamps', 'WgradLinear',
             'adam_clip_step', 'adv_normalize', 'adv_stats', 'compact_visible', 'gae', 'linear_act', 'linear_supported', 'math', 'orca_solve',
             'prediction_dots', 'render_scenes', 'split_bf16', 'tile_images', 'torch', 'weight_mm', 'wgrad', 'wgrad_supported']


def test_call_names_the_symbol_and_carries_the_library_message():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    with pytest.raises(A.CnError) as e:
        A.call("cn_policy_create", 20, 2, 4, C.byref(h))
    assert "cn_policy_create" in str(e.value) and "no HIP device" in str(e.value)
    with pytest.raises(AttributeError):
        A.call("cn_no_such_symbol")


def test_every_handle_wrapper_refuses_without_a_gpu_and_closes_silently(monkeypatch):
    from crowdnav_prediction_attngraph_amd import hip
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for cls, args in ((hip.HipEnvBatch, (A.default_env_config(), 4, 425)), (hip.HipPolicy, (20, 2, 4)), (hip.HipSrnn, (20, 2, 4)), (hip.HipGST, (20, 4))):
        assert issubclass(cls, hip.HipHandle)
        obj = cls.__new__(cls)
        with pytest.raises(A.CnError, match="no CPU fallback"):
            obj.__init__(*args)
        obj.close()
        obj.close()
        obj.__del__()
        del obj
    with pytest.raises(A.CnError, match="no CPU fallback"):
        hip.orca_solve(torch.zeros(1, 8), torch.zeros(1, 2, 5))


def test_hip_still_exports_every_name_it_had():
    from crowdnav_prediction_attngraph_amd import hip
    assert [n for n in HIP_NAMES if not hasattr(hip, n)] == []


@pytest.mark.parametrize("base", ["selfAttn_merge_srnn", "srnn"])
def test_policy_rollout_contract_on_cpu_tensors(base):
    """act / get_value / evaluate_actions of both bases are one body each over base.forward_rnn: the three agree with each other and return
    the reference's two-key rnn_hxs.  (Their values against the golden fixtures: test_host_policy.py, test_srnn_host.py.)"""
    from crowdnav_prediction_attngraph_amd.policy import Policy, make_spaces
    from tests import policy_util as PU
    E, H, D = 3, 5, 2
    torch.manual_seed(7)
    ob_space, act_space = make_spaces(H, D)
    pol = Policy(ob_space.spaces, act_space, base=base, base_kwargs=dict(env_name="CrowdSimVarNum-v0", num_processes=E, num_mini_batch=1, seq_length=1))
    assert pol.is_srnn_baseline == (base == "srnn")
    if base == "srnn":
        assert pol.base.hip_provider == pol._hip_handle
    obs = {k: torch.from_numpy(v) for k, v in PU.synth_obs(E, H, D, 3).items()}
    hxs = {"human_node_rnn": torch.randn(E, 1, 128), "human_human_edge_rnn": torch.randn(E, H + 1, 256) if base == "srnn" else torch.zeros(E, H + 1, 256)}
    masks = torch.tensor([[1.0], [0.0], [1.0]])
    value, action, logp, h = pol.act(obs, hxs, masks, deterministic=True)
    assert value.shape == (E, 1) and action.shape == (E, 2) and logp.shape == (E, 1)
    assert list(h) == ["human_node_rnn", "human_human_edge_rnn"]
    assert h["human_node_rnn"].shape == (E, 1, 128) and h["human_human_edge_rnn"].shape == (E, H + 1, 256)
    assert bool(h["human_human_edge_rnn"].abs().sum() > 0) == (base == "srnn")       # live for DS-RNN only
    assert torch.equal(pol.get_value(obs, hxs, masks), value)
    v2, lp2, ent, h2 = pol.evaluate_actions(obs, hxs, masks, action)
    assert torch.allclose(v2, value, atol=1e-6) and torch.allclose(lp2, logp, atol=1e-6) and abs(float(ent.detach()) - 1.4189385) < 1e-6
    for k in h:
        assert torch.allclose(h2[k], h[k], atol=1e-6), k
