"""GPU tests of the DS-RNN baseline's edge-sequence training kernels (hip.SrnnEdgeSequence = cn_srnn_seq_fwd / cn_srnn_seq_bwd): the op against
the torch-op loop in fp64, every gradient through evaluate_actions against the fp64 CPU graph, the kernel path against the op path on the GPU,
bit determinism and row isolation, one PPO.update with the path on and off, and the refusals."""
import copy
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from crowdnav_prediction_attngraph_amd import _abi as A  # noqa: E402
from tests import srnn_seq_util as Q  # noqa: E402
from tests import srnn_util as SU  # noqa: E402

MODES = ("bf16x3", "fp32")
# Parameters whose gradient terms cancel and which, in mode 'bf16x3' only, are held at 1e-2 of the largest entry and 1 - cos <= 2e-6 (the rule of
# tests/test_gpu_minibatch_step.py) instead of 5e-4: none was needed at these shapes.
CANCELLING = ()


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(policy on the CPU, its fp64 copy, the sequence): built once per shape and never written."""
    T, N, H, D = shape
    pol = Q.policy(H, D, N, T)
    return pol, copy.deepcopy(pol).double(), Q.sequence(T, N, H, D)


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """The fp64 CPU graph of a shape, computed once: h_all of the op loop in fp64 and fp32, and evaluate_actions with all gradients."""
    T, N, H, D = shape
    pol, ref, seq = _case(shape)
    with torch.no_grad():
        h64, h32 = Q.op_loop(ref, seq, T, N, torch.float64), Q.op_loop(pol, seq, T, N, torch.float32)
    ref = copy.deepcopy(ref)
    v, lp, g, d_h0 = _evaluate(ref, seq, "cpu", torch.float64)
    return dict(h64=h64, d=float((h32.double() - h64).abs().max()), v=v, lp=lp, grads=g, d_h0=d_h0)


_evaluate = Q.evaluate


def _gpu_policy(shape, mode, kernels=True):
    pol = copy.deepcopy(_case(shape)[0]).cuda()
    pol.srnn_gemm_mode = mode
    pol.base.train_edge_kernels = kernels
    return pol


def _seq_op(pol, seq, N):
    """h_all of hip.SrnnEdgeSequence on the policy's own handle and parameters."""
    from crowdnav_prediction_attngraph_amd.hip import SrnnEdgeSequence
    dev = _dev()
    hip = pol._hip_srnn(N, dev)
    return SrnnEdgeSequence.apply(hip, seq["obs"]["temporal_edges"].to(dev), seq["obs"]["spatial_edges"].to(dev), seq["edge_h0"].to(dev),
                                  seq["masks"].to(dev), *pol.base._edge_parameters())


def _check_grads(got, want, mode, label):
    Q.check_grads(got, want, mode, label, cancelling=CANCELLING, dead=SU.DEAD)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", Q.SHAPES, ids=Q.shape_id)
def test_h_all_follows_the_op_loop_in_fp64(shape, mode):
    """max(1e-4, 4 d) with d = |fp32 - fp64| of the op loop's own CPU graph on this input (the rule of test_device_rollout_follows_the_reference)."""
    T, N, H, D = shape
    ref, seq = _reference(shape), _case(shape)[2]
    pol = _gpu_policy(shape, mode)
    with torch.no_grad():
        h = _seq_op(pol, seq, N)
    bar = max(1e-4, 4 * ref["d"])
    err = float((h.cpu().double() - ref["h64"]).abs().max())
    print("srnn edge sequence %s %s: d = %.3g, bar = %.3g, deviation = %.3g" % (Q.shape_id(shape), mode, ref["d"], bar, err))
    assert tuple(h.shape) == (T, N, H + 1, 256) and err <= bar


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [s for s in Q.SHAPES if s[0] == 1] + [(1, 5, 20, 12)], ids=Q.shape_id)
def test_one_step_is_cn_srnn_act_bit_for_bit(shape, mode):
    T, N, H, D = shape
    seq = Q.sequence(T, N, H, D)
    pol = copy.deepcopy(Q.policy(H, D, N, T)).cuda()
    pol.srnn_gemm_mode = mode
    dev = _dev()
    with torch.no_grad():
        h = _seq_op(pol, seq, N)
        out = pol._hip_srnn(N, dev).act({k: seq["obs"][k].to(dev) for k in Q.OBS_KEYS[:3]}, seq["node_h0"].to(dev), seq["edge_h0"].to(dev),
                                        seq["masks"].to(dev), eps=None)
    assert torch.equal(h[0], out["edge_hxs"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", Q.SHAPES, ids=Q.shape_id)
def test_gradients_match_the_fp64_cpu_graph(shape, mode):
    """Every live parameter and edge_h0 at 5e-4 of the tensor's largest entry + 1e-7; the three dead modules keep grad None."""
    ref, seq = _reference(shape), _case(shape)[2]
    pol = _gpu_policy(shape, mode)
    v, lp, grads, d_h0 = _evaluate(pol, seq, "cuda", torch.float32)
    np.testing.assert_allclose(v.numpy(), ref["v"].numpy(), atol=1e-4)
    np.testing.assert_allclose(lp.numpy(), ref["lp"].numpy(), atol=1e-4)
    _check_grads(dict(grads, edge_h0=d_h0), dict(ref["grads"], edge_h0=ref["d_h0"]), mode, Q.shape_id(shape))


def test_kernel_path_against_op_path_on_the_gpu():
    """(4, 4, 20, 12) in fp32 arithmetic: values, log-probs and every gradient of the two paths agree within the bars above."""
    shape = (4, 4, 20, 12)
    seq = _case(shape)[2]
    on, off = _gpu_policy(shape, "fp32", True), _gpu_policy(shape, "fp32", False)
    v1, lp1, g1, d1 = _evaluate(on, seq, "cuda", torch.float32)
    # the kernel path ran: the handle exists; the op path never asks for one
    assert on._hip is not None
    v0, lp0, g0, d0 = _evaluate(off, seq, "cuda", torch.float32)
    assert off._hip is None
    np.testing.assert_allclose(v1.numpy(), v0.numpy(), atol=1e-4)
    np.testing.assert_allclose(lp1.numpy(), lp0.numpy(), atol=1e-4)
    _check_grads(dict(g1, edge_h0=d1), dict(g0, edge_h0=d0), "fp32", "kernel vs ops")


@pytest.mark.parametrize("mode", MODES)
def test_equal_arguments_give_equal_bits_and_rows_do_not_see_their_tile(mode):
    shape = (4, 4, 20, 12)
    T, N, H, D = shape
    seq = _case(shape)[2]
    runs = []
    for _ in range(2):
        pol = _gpu_policy(shape, mode)
        with torch.no_grad():
            h = _seq_op(pol, seq, N).clone()
        v, lp, g, d = _evaluate(pol, seq, "cuda", torch.float32)
        runs.append([h.cpu(), v, lp, d] + [t for t in g.values() if t is not None])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # env 0 alone (N = 1) gives the bits it has as one of four
    one = dict(obs={k: t.view(T, N, *t.shape[1:])[:, :1].reshape(T, *t.shape[1:]) for k, t in seq["obs"].items()}, edge_h0=seq["edge_h0"][:1],
               masks=seq["masks"].view(T, N, 1)[:, :1].reshape(T, 1))
    pol = _gpu_policy(shape, mode)
    with torch.no_grad():
        h1 = _seq_op(pol, one, 1)
    assert torch.equal(h1[:, 0].cpu(), runs[0][0][:, 0])


def test_one_ppo_update_with_the_path_on_and_off():
    """srnn_rollout_e4_h5_t5: losses and the 256-sample weight probes of the two paths within 1e-5, the bar of the reference's goldens."""
    from crowdnav_prediction_attngraph_amd.ppo import PPO
    path = [p for p in SU.ROLLOUT_CASES if SU.case_id(p) == "rollout_e4_h5_t5"][0]
    z, meta = SU.load(path)
    T, E, nmb = meta["T"], meta["E"], meta["nmb"]
    res = []
    for flag in (True, False):
        pol, ob_space, act_space = SU.policy(meta, E, nmb, T)
        pol = pol.cuda()
        pol.base.train_edge_kernels = flag
        ro = SU.fill_rollouts(z, meta, ob_space, act_space)
        ro.to(torch.device("cuda"))
        ro.compute_returns(torch.from_numpy(z["next_value"]).cuda(), True, 0.99, 0.95, False)
        agent = PPO(pol, 0.2, meta["ppo_epoch"], nmb, 0.5, 0.0, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
        torch.manual_seed(meta["update_seed"])
        losses = agent.update(ro)
        probes = {}
        for k, t in pol.state_dict().items():
            flat = t.cpu().numpy().reshape(-1)
            probes[k] = flat[np.linspace(0, flat.size - 1, min(flat.size, 256)).astype(np.int64)]
        res.append((losses, probes, pol._hip is not None))
    assert res[0][2] and not res[1][2]          # only the kernel path asks for the handle inside update()
    np.testing.assert_allclose(res[0][0], res[1][0], atol=1e-5)
    for k in res[0][1]:
        np.testing.assert_allclose(res[0][1][k], res[1][1][k], atol=1e-5, err_msg=k)


def test_refusals_name_the_call_and_launch_nothing():
    shape = (3, 3, 20, 2)
    T, N, H, D = shape
    seq = _case(shape)[2]
    pol = _gpu_policy(shape, "bf16x3")
    dev = _dev()
    hip = pol._hip_srnn(N, dev)
    te, se, e0, m = (seq["obs"]["temporal_edges"].to(dev), seq["obs"]["spatial_edges"].to(dev), seq["edge_h0"].to(dev), seq["masks"].to(dev))
    torch.cuda.synchronize()
    with pytest.raises(A.CnError, match="cn_srnn_seq_fwd.*float32"):
        hip.seq_fwd(te.double(), se, e0, m, T, N)
    with pytest.raises(A.CnError, match="cn_srnn_seq_fwd.*must live on"):
        hip.seq_fwd(te, se.cpu(), e0, m, T, N)
    small = torch.zeros(hip.seq_workspace_bytes(T - 1, N) // 4, device=dev)
    with pytest.raises(A.CnError, match=r"cn_srnn_seq_fwd: T \* N = 3 \* 3 needs a workspace"):
        hip.seq_fwd(te, se, e0, m, T, N, workspace=small)
    assert not small.any()                      # no launch: the short workspace is untouched
    h_all, ws = hip.seq_fwd(te, se, e0, m, T, N)
    kept = ws.clone()
    grads = [torch.zeros_like(p) for p in pol.base._edge_parameters()]
    d_h = torch.ones_like(h_all)
    with pytest.raises(A.CnError, match="cn_srnn_seq_bwd: gradient pointer #3 is null"):
        hip.seq_bwd(te, se, e0, m, h_all, d_h, ws, T, N, grads[:3] + [None] + grads[4:])
    with pytest.raises(A.CnError, match=r"cn_srnn_seq_bwd: T \* N = 3 \* 3 needs a workspace"):
        hip.seq_bwd(te, se, e0, m, h_all, d_h, small, T, N, grads)
    with pytest.raises(A.CnError, match="cn_srnn_seq_bwd.*d_h_all must be float32"):
        hip.seq_bwd(te, se, e0, m, h_all, d_h.double(), ws, T, N, grads)
    assert torch.equal(ws, kept) and not any(g.any() for g in grads)       # the backward consumes the workspace: untouched = no launch
    # a handle without weights
    from crowdnav_prediction_attngraph_amd.hip import HipSrnn
    bare = HipSrnn(H, D, N, device=dev)
    with pytest.raises(A.CnError, match="cn_srnn_seq_fwd: cn_srnn_set_weights has not been called"):
        bare.seq_fwd(te, se, e0, m, T, N)
    bare.close()
