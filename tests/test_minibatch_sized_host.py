"""Host side of cn_ppo_minibatch_step_sized (no device): the workspace query runs on the host -- the default tuple and NULL are the unsized query,
the size grows with the network, a tuple outside the device box or a row count past cn_ppo_minibatch_max_rows() gives 0 -- and
hip.SizedMinibatchStepper.supported is false wherever the step cannot run.  The GPU side: tests/test_gpu_minibatch_sized.py."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

from crowdnav_prediction_attngraph_amd import _abi as A  # noqa: E402

SHAPES = [(30, 2048, 20, 2, 405000), (1, 1, 1, 2, 1), (5, 17, 48, 16, 5 * 17 * 48)]     # (T, N, H, D, rows)


@pytest.mark.parametrize("shape", SHAPES)
def test_default_tuple_and_null_are_the_unsized_query(shape):
    L = A.lib()
    want = L.cn_ppo_minibatch_workspace_bytes(*shape)
    assert want > 0
    d = A.PolicyDims(*A.DEFAULT_DIMS)
    assert L.cn_ppo_minibatch_workspace_bytes_sized(*shape, C.byref(d)) == want
    assert L.cn_ppo_minibatch_workspace_bytes_sized(*shape, None) == want


@pytest.mark.parametrize("shape", SHAPES)
def test_the_workspace_grows_with_the_network(shape):
    L = A.lib()
    small, large = A.PolicyDims(64, 64, 32, 64), A.PolicyDims(256, 128, 128, 512)
    s, l_ = L.cn_ppo_minibatch_workspace_bytes_sized(*shape, C.byref(small)), L.cn_ppo_minibatch_workspace_bytes_sized(*shape, C.byref(large))
    assert 0 < s < L.cn_ppo_minibatch_workspace_bytes(*shape) < l_
    assert s % 256 == 0 and l_ % 256 == 0                                # every piece is 256-byte aligned


@pytest.mark.parametrize("bad", [(96, 64, 64, 256), (128, 32, 64, 256), (128, 64, 64, 96), (128, 64, 0, 256), (128, 64, 257, 256)],
                         ids=["R96", "M32", "O96", "A0", "A257"])
def test_a_tuple_outside_the_box_gives_zero(bad):
    L = A.lib()
    d = A.PolicyDims(*bad)
    for shape in SHAPES:
        assert L.cn_ppo_minibatch_workspace_bytes_sized(*shape, C.byref(d)) == 0


def test_rows_past_the_bound_give_zero_at_every_size():
    L = A.lib()
    top = int(L.cn_ppo_minibatch_max_rows())
    T, N, H, D = 30, 2048, 48, 2
    for dims in ((64, 64, 1, 64), (192, 64, 48, 320), (256, 128, 256, 512)):
        d = A.PolicyDims(*dims)
        assert L.cn_ppo_minibatch_workspace_bytes_sized(T, N, H, D, top, C.byref(d)) > 0
        assert L.cn_ppo_minibatch_workspace_bytes_sized(T, N, H, D, top + 1, C.byref(d)) == 0
    d = A.PolicyDims(192, 64, 48, 320)                                   # the unchanged shape limits: H <= 48, D <= 16
    assert L.cn_ppo_minibatch_workspace_bytes_sized(2, 3, 49, 2, 6, C.byref(d)) == 0
    assert L.cn_ppo_minibatch_workspace_bytes_sized(2, 3, 5, 17, 6, C.byref(d)) == 0


def _policy_and_storage(base="selfAttn_merge_srnn", **kw):
    from crowdnav_prediction_attngraph_amd.policy import Policy, make_spaces
    from crowdnav_prediction_attngraph_amd.trainer import new_rollouts
    T, E, H, D = 2, 3, 5, 2
    ob_space, act_space = make_spaces(H, D)
    pol = Policy(ob_space.spaces, act_space, base=base, base_kwargs=dict(env_name="CrowdSimVarNum-v0", num_processes=E, num_mini_batch=1, seq_length=T, **kw))
    return pol, new_rollouts(pol, T, E, ob_space.spaces, act_space)


def test_supported_is_false_where_the_step_cannot_run():
    from crowdnav_prediction_attngraph_amd import hip
    sized = dict(human_node_rnn_size=192, human_node_embedding_size=64, attention_size=48, human_node_output_size=320)
    assert issubclass(hip.SizedMinibatchStepper, hip.MinibatchStepper)
    pol, ro = _policy_and_storage(**sized)                               # CPU tensors
    assert pol.base.sized_rn_ok() and not ro.rewards.is_cuda
    assert not hip.SizedMinibatchStepper.supported(pol, ro) and not hip.MinibatchStepper.supported(pol, ro)
    pol, ro = _policy_and_storage(base="srnn")                           # the DS-RNN baseline
    assert not hip.SizedMinibatchStepper.supported(pol, ro)
    pol, ro = _policy_and_storage(use_self_attn=False, **sized)
    assert not hip.SizedMinibatchStepper.supported(pol, ro)
