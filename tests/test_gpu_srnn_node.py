"""GPU tests of the DS-RNN baseline's node-half training path: cn_srnn_attn_fwd / cn_srnn_attn_bwd (hip.SrnnAttention) against the fp64 graph of
SRNNBase.attention with guarded, NaN-filled outputs; bit determinism and sample isolation; forward_sequence + evaluate_actions with
SRNNBase.train_node_kernels against the fp64 CPU graph, with the edge kernels on and off; no torch-op loop or attention left with both flags on;
one PPO.update with the flag on and off; the refusals."""
import copy
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from crowdnav_prediction_attngraph_amd import _abi as A  # noqa: E402
from crowdnav_prediction_attngraph_amd import policy as policy_module  # noqa: E402
from crowdnav_prediction_attngraph_amd.policy import Policy, make_spaces  # noqa: E402
from tests import srnn_seq_util as Q  # noqa: E402
from tests import srnn_util as SU  # noqa: E402

MODES = ("bf16x3", "fp32")
# (B, H): a softmax of one; small; the training crowd; past 32 slots, 9 workgroups of 16 samples with 6 in the last; the box edge
ATTN_CASES = [(1, 1), (3, 5), (15, 20), (134, 33), (70, 64)]
GUARD = 64
PATH_SHAPES = Q.SHAPES + [(3, 17, 5, 2)]          # N = 17: past one 16-row tile of the GRU sequence kernels


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _layouts(B):
    """Both ways h_all [T,N,H+1,256] holds B = T * N samples, and a proper factorisation where B has one."""
    out = list(dict.fromkeys([(1, B), (B, 1)]))
    f = next((k for k in range(2, B) if B % k == 0), None)
    return out + ([(f, B // f)] if f else [])


@functools.lru_cache(maxsize=None)
def _attn_module():
    """The seeded module init of the two attention layers (a base of any H has them); nn.Linear gives spatial_edge_layer a non-zero bias, which
    the softmax must not see."""
    torch.manual_seed(0)
    ob_space, act_space = make_spaces(5, 2)
    base = Policy(ob_space.spaces, act_space, base="srnn", base_kwargs=dict(num_processes=1, num_mini_batch=1, seq_length=1)).base
    return base, copy.deepcopy(base).double()


@functools.lru_cache(maxsize=None)
def _attn_reference(case):
    """Inputs (states uniform in (-1, 1), as GRU states are) and the fp64 graph of SRNNBase.attention with its autograd, computed once per case."""
    B, H = case
    base, base64 = _attn_module()
    rs = np.random.RandomState(100 * B + H)
    h_all = torch.from_numpy(rs.uniform(-1, 1, (B, H + 1, 256)).astype(np.float32))
    d_w = torch.from_numpy(rs.uniform(-1, 1, (B, 256)).astype(np.float32))
    d_t = torch.from_numpy(rs.uniform(-1, 1, (B, 256)).astype(np.float32))
    with torch.no_grad():
        w32, a32 = base.attention(h_all[:, 0], h_all[:, 1:])
    h64 = h_all.double().requires_grad_(True)
    w64, a64 = base64.attention(h64[:, 0], h64[:, 1:])
    tl, sl = base64.attn.temporal_edge_layer[0], base64.attn.spatial_edge_layer[0]
    params = [tl.weight, tl.bias, sl.weight, sl.bias]
    ref = dict(h_all=h_all, d_w=d_w, d_t=d_t, w64=w64.detach(), a64=a64.detach(),
               d=max(float((w32.double() - w64.detach()).abs().max()), float((a32.double() - a64.detach()).abs().max())))
    for direct in (False, True):
        loss = (w64 * d_w.double()).sum() + ((h64[:, 0] * d_t.double()).sum() if direct else 0.0)
        g = torch.autograd.grad(loss, [h64] + params, retain_graph=True)
        ref[direct] = dict(zip(("d_h_all", "Wt", "bt", "Ws", "bs"), (t.detach() for t in g)))
    return ref


def _attn_params(dev):
    base = _attn_module()[0]
    tl, sl = base.attn.temporal_edge_layer[0], base.attn.spatial_edge_layer[0]
    return [p.detach().to(dev).clone().requires_grad_(True) for p in (tl.weight, tl.bias, sl.weight, sl.bias)]


def _guarded(n, dev):
    return torch.full((n + GUARD,), float("nan"), device=dev)


def _raw_calls(h_all, params, d_w, d_t, H):
    """cn_srnn_attn_fwd and cn_srnn_attn_bwd on NaN-filled outputs with GUARD floats behind each; returns {name: written part} after checking
    that every element was written and no guard was touched."""
    dev = h_all.device
    B = h_all.numel() // ((H + 1) * 256)
    wt, bt, ws, _ = (p.detach() for p in params)
    sizes = dict(weighted=B * 256, attn=B * H, te=B * 64, u=B * 256, d_h_all=B * (H + 1) * 256, d_u=B * 256, d_te=B * 64)
    o = {k: _guarded(n, dev) for k, n in sizes.items()}
    A.call("cn_srnn_attn_fwd", B, H, A.ptr(h_all), A.ptr(wt), A.ptr(bt), A.ptr(ws), A.ptr(o["weighted"]), A.ptr(o["attn"]), A.ptr(o["te"]), A.ptr(o["u"]),
           A.stream_ptr())
    attn, u = o["attn"][:B * H].clone(), o["u"][:B * 256].clone()      # (named: a temporary would be freed, and its block reused, before the call)
    A.call("cn_srnn_attn_bwd", B, H, A.ptr(h_all), A.ptr(wt), A.ptr(ws), A.ptr(attn), A.ptr(u), A.ptr(d_w), A.ptr(d_t), A.ptr(o["d_h_all"]), A.ptr(o["d_u"]),
           A.ptr(o["d_te"]), A.stream_ptr())
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert not bool(torch.isnan(o[k][:n]).any()), "%s: elements left unwritten" % k
        assert bool(torch.isnan(o[k][n:]).all()), "%s: the guard behind it was written" % k
    return {k: o[k][:n].clone() for k, n in sizes.items()}


@pytest.mark.parametrize("direct", (False, True), ids=("null", "direct"))
@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: "b%d_h%d" % c)
def test_attention_follows_the_fp64_graph(case, direct):
    """Forward: weighted and attn at max(1e-4, 4 d), d = |fp32 - fp64| of the torch-op graph on this input.  Backward: d_h_all and the five
    parameter gradients by srnn_seq_util.check_grads' rule; the bias of spatial_edge_layer exactly zero.  d_t_direct NULL and given."""
    from crowdnav_prediction_attngraph_amd.hip import SrnnAttention
    B, H = case
    ref, dev = _attn_reference(case), _dev()
    bar = max(1e-4, 4 * ref["d"])
    d_w, d_t = ref["d_w"].to(dev), (ref["d_t"].to(dev) if direct else None)
    want = dict(ref[direct])
    for T, N in _layouts(B):
        h_all = ref["h_all"].to(dev).view(T, N, H + 1, 256).clone().requires_grad_(True)
        params = _attn_params(dev)
        raw = _raw_calls(h_all.detach(), params, d_w, d_t, H)
        out = SrnnAttention.apply(h_all, *params, True) if direct else SrnnAttention.apply(h_all, *params)
        weighted, attn = out[0], out[1]
        assert tuple(weighted.shape) == (T, N, 256) and tuple(attn.shape) == (T, N, H) and not attn.requires_grad
        assert torch.equal(weighted.detach().reshape(-1), raw["weighted"]) and torch.equal(attn.reshape(-1), raw["attn"])
        e_w = float((weighted.detach().cpu().double().view(B, 256) - ref["w64"]).abs().max())
        e_a = float((attn.cpu().double().view(B, H) - ref["a64"]).abs().max())
        print("srnn attention b%d_h%d [%d,%d] %s: d = %.3g, bar = %.3g, weighted %.3g, attn %.3g" % (B, H, T, N, "direct" if direct else "null", ref["d"], bar, e_w, e_a))
        assert e_w <= bar and e_a <= bar
        loss = (weighted.view(B, 256) * d_w).sum()
        if direct:
            assert torch.equal(out[2].reshape(B, 256), h_all.detach().view(B, H + 1, 256)[:, 0])
            loss = loss + (out[2].view(B, 256) * d_t).sum()
        loss.backward()
        assert torch.equal(h_all.grad.reshape(-1), raw["d_h_all"])
        got = dict(d_h_all=h_all.grad.cpu().double().view(B, H + 1, 256), **{k: p.grad.cpu().double() for k, p in zip(("Wt", "bt", "Ws", "bs"), params)})
        assert got["bs"].shape == (64,) and not bool(got["bs"].any()), "the bias of spatial_edge_layer must get an exact zero"
        want_live = {k: v for k, v in want.items() if k != "bs"}
        Q.check_grads(got, want_live, "fp32", "srnn attention b%d_h%d [%d,%d]" % (B, H, T, N))
        assert float(want["bs"].abs().max()) <= 1e-9            # ... as the fp64 graph has it, to rounding


def test_equal_arguments_give_equal_bits_and_a_sample_does_not_see_its_batch():
    case = (134, 33)
    B, H = case
    ref, dev = _attn_reference(case), _dev()
    h_all, d_w, d_t = ref["h_all"].to(dev), ref["d_w"].to(dev), ref["d_t"].to(dev)
    params = _attn_params(dev)
    a, b = _raw_calls(h_all, params, d_w, d_t, H), _raw_calls(h_all, params, d_w, d_t, H)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    r = 77                                                           # workgroup 4, wavefront 13 of the batch; workgroup 0, wavefront 0 alone
    one = _raw_calls(h_all[r:r + 1].contiguous(), params, d_w[r:r + 1].contiguous(), d_t[r:r + 1].contiguous(), H)
    for k, t in one.items():
        assert torch.equal(t, a[k].view(B, -1)[r]), k


# ---- the whole path: forward_sequence + evaluate_actions ----
@functools.lru_cache(maxsize=None)
def _case(shape):
    T, N, H, D = shape
    pol = Q.policy(H, D, N, T)
    return pol, Q.sequence(T, N, H, D)


def _evaluate(p, seq, dev, dt):
    """srnn_seq_util.evaluate with value weights that do not sum to zero.  Its weights, linspace(-1, 1), make the gradient of critic_linear.bias
    -- their sum -- an exact zero, so check_grads holds that tensor to its absolute floor of 1e-7, which the fp32 rounding of a sum of B terms of
    order one passes or misses by the order of summation alone (N = 17, T = 3: partial sums reach 13, one ulp there is 9.5e-7).  Shifted by
    0.25 the gradient is B / 4 and the relative bar applies to it like to every other tensor.  Everything else is that helper's."""
    to = lambda t: t.to(device=dev, dtype=dt)  # noqa: E731
    e0 = to(seq["edge_h0"]).clone().requires_grad_(True)
    p.zero_grad(set_to_none=True)
    v, lp, ent, _ = p.evaluate_actions({k: to(t) for k, t in seq["obs"].items()}, {"human_node_rnn": to(seq["node_h0"]), "human_human_edge_rnn": e0},
                                       to(seq["masks"]), to(seq["actions"]))
    w = torch.linspace(-1, 1, v.numel(), dtype=dt, device=dev).view_as(v)
    ((v * (w + 0.25)).sum() + (lp * w.flip(0)).sum() + ent).backward()
    grads = {n: (None if q.grad is None else q.grad.detach().cpu().double().clone()) for n, q in p.named_parameters()}
    return v.detach().cpu().double(), lp.detach().cpu().double(), grads, e0.grad.detach().cpu().double()


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """The fp64 CPU graph through evaluate_actions, once per shape."""
    pol, seq = _case(shape)
    v, lp, g, d_h0 = _evaluate(copy.deepcopy(pol).double(), seq, "cpu", torch.float64)
    return dict(v=v, lp=lp, grads=g, d_h0=d_h0)


def _gpu_policy(shape, mode, edge=True, node=True):
    pol = copy.deepcopy(_case(shape)[0]).cuda()
    pol.srnn_gemm_mode = mode
    pol.base.train_edge_kernels, pol.base.train_node_kernels = edge, node
    return pol


@pytest.mark.parametrize("edge", (True, False), ids=("edge_kernels", "edge_ops"))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", PATH_SHAPES, ids=Q.shape_id)
def test_whole_path_follows_the_fp64_cpu_graph(shape, mode, edge):
    """Value and log-prob at 1e-4; every live parameter's gradient and edge_h0's by check_grads; the three dead modules keep None."""
    ref, seq = _reference(shape), _case(shape)[1]
    pol = _gpu_policy(shape, mode, edge=edge)
    v, lp, grads, d_h0 = _evaluate(pol, seq, "cuda", torch.float32)
    print("srnn node path %s %s %s: value %.3g, log-prob %.3g" % (Q.shape_id(shape), mode, "edge kernels" if edge else "edge ops",
                                                                  float((v - ref["v"]).abs().max()), float((lp - ref["lp"]).abs().max())))
    np.testing.assert_allclose(v.numpy(), ref["v"].numpy(), atol=1e-4)
    np.testing.assert_allclose(lp.numpy(), ref["lp"].numpy(), atol=1e-4)
    Q.check_grads(dict(grads, edge_h0=d_h0), dict(ref["grads"], edge_h0=ref["d_h0"]), mode, Q.shape_id(shape), dead=SU.DEAD)


def test_taps_keep_working_on_the_kernel_route():
    shape = (4, 4, 20, 12)
    T, N, H, D = shape
    seq = _case(shape)[1]
    dev = _dev()
    taps = {}
    for node in (True, False):
        pol = _gpu_policy(shape, "bf16x3", node=node)
        t = {}
        with torch.no_grad():
            pol.base.forward_sequence({k: x.to(dev) for k, x in seq["obs"].items()}, seq["node_h0"].to(dev), seq["edge_h0"].to(dev), seq["masks"].to(dev),
                                      T, N, taps=t)
        taps[node] = t
    assert sorted(taps[True]) == sorted(taps[False]) == ["actor_feat", "attn", "edge_out", "node_out", "weighted"]
    for k in taps[True]:
        assert taps[True][k].shape == taps[False][k].shape
        np.testing.assert_allclose(taps[True][k].cpu().numpy(), taps[False][k].cpu().numpy(), atol=1e-4, err_msg=k)


def test_no_loop_left_with_both_flags_on(monkeypatch):
    """With both flags on neither the per-step torch cell nor the torch-op attention runs: both raise here, and forward plus backward still run."""
    def gone(*a, **k):
        raise AssertionError("the torch-op route ran")
    monkeypatch.setattr(policy_module, "_gru_cell", gone)
    monkeypatch.setattr(policy_module.SRNNBase, "attention", gone)
    shape = (4, 4, 20, 12)
    pol = _gpu_policy(shape, "bf16x3")
    v, lp, grads, d_h0 = _evaluate(pol, _case(shape)[1], "cuda", torch.float32)
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(lp).all()) and bool(torch.isfinite(d_h0).all())
    live = [n for n, g in grads.items() if g is not None]
    assert len(live) == len(grads) - 6 and all(bool(torch.isfinite(grads[n]).all()) for n in live)


def _one_update(flag):
    from crowdnav_prediction_attngraph_amd.ppo import PPO
    path = [p for p in SU.ROLLOUT_CASES if SU.case_id(p) == "rollout_e4_h5_t5"][0]
    z, meta = SU.load(path)
    T, E, nmb = meta["T"], meta["E"], meta["nmb"]
    pol, ob_space, act_space = SU.policy(meta, E, nmb, T)
    pol = pol.cuda()
    pol.base.train_node_kernels = flag
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
    return losses, probes


def test_one_ppo_update_with_the_flag_on_and_off():
    """srnn_rollout_e4_h5_t5: losses and the 256-sample weight probes of the two routes within 1e-5; two runs with the flag on are bit-identical."""
    on, on2, off = _one_update(True), _one_update(True), _one_update(False)
    np.testing.assert_allclose(on[0], off[0], atol=1e-5)
    for k in on[1]:
        np.testing.assert_allclose(on[1][k], off[1][k], atol=1e-5, err_msg=k)
    assert np.array_equal(np.asarray(on[0]), np.asarray(on2[0]))
    for k in on[1]:
        assert np.array_equal(on[1][k], on2[1][k]), k


def test_refusals_name_the_call_and_launch_nothing():
    dev = _dev()
    B, H = 4, 5
    h_all = torch.zeros(B, H + 1, 256, device=dev)
    wt, bt, ws, _ = (p.detach() for p in _attn_params(dev))
    o = {k: _guarded(n, dev) for k, n in dict(weighted=B * 256, attn=B * H, te=B * 64, u=B * 256, d_h_all=B * (H + 1) * 256, d_u=B * 256, d_te=B * 64).items()}
    ones = torch.ones(B, 256, device=dev)
    attn = torch.full((B, H), 1.0 / H, device=dev)
    for b, h, first in ((B, 0, h_all), (B, 65, h_all), (0, H, h_all), (B, H, None)):
        with pytest.raises(A.CnError, match="cn_srnn_attn_fwd"):
            A.call("cn_srnn_attn_fwd", b, h, A.ptr(first), A.ptr(wt), A.ptr(bt), A.ptr(ws), A.ptr(o["weighted"]), A.ptr(o["attn"]), A.ptr(o["te"]),
                   A.ptr(o["u"]), A.stream_ptr())
        with pytest.raises(A.CnError, match="cn_srnn_attn_bwd"):
            A.call("cn_srnn_attn_bwd", b, h, A.ptr(first), A.ptr(wt), A.ptr(ws), A.ptr(attn), A.ptr(ones), A.ptr(ones), None, A.ptr(o["d_h_all"]),
                   A.ptr(o["d_u"]), A.ptr(o["d_te"]), A.stream_ptr())
    torch.cuda.synchronize()
    for k, t in o.items():
        assert bool(torch.isnan(t).all()), "%s was written: something was launched" % k
