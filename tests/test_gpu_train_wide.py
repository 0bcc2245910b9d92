"""-m gpu: the training route of crowds of 49 to 64 humans against the torch-op graph on the CPU in fp64, with the GPU's ReLU gates imposed.

cn_ppo_minibatch_step declares 1 <= H <= 48.  The simulator, the rollout policy, Policy.evaluate_actions and PPO.update take up to 64 humans,
and for those crowds training runs the per-layer human-human block of policy.py::_hh_block (Embed0 -> HipLinear -> HipLinear -> HHAttention ->
HipLinear, the affine folds as plain products), hip_train.RnSequence behind it and the autograd-joined update.  Each case makes ONE call of that
route at the default flags (train_gemm_mode 'bf16x3', train_fused_hh, train_fused_rn): evaluate_actions on the minibatch
RolloutStorage.recurrent_generator hands over for the env subset `idx` (the same index_select / T-major flattening; the generator itself can
only draw E // num_mini_batch envs), PPO._losses, backward() into the flat bucket.  Storage, policy and the fp64 side are the ones of
tests/test_gpu_minibatch_edges.py and tests/test_gpu_minibatch_step.py.

  * values and log-probs of ALL samples within 1e-4 of the fp64 graph, the two losses at rtol 2e-4 / atol 1e-6, the entropy in closed form
    at 1e-6 (the bars of the edges test);
  * the gates of the block's three ReLUs, recorded from the Functions' outputs (tests/relu_gate_util.py), differ from the fp64 graph's own
    only at units whose fp64 pre-activation is within 1e-4 (the forward bar) of zero;
  * every parameter gradient against the fp64 graph WITH THOSE GATES IMPOSED: 5e-4 of the reference tensor's largest entry + 1e-7; what the
    loss does not reach is an exact zero, spatial_edge_layer's bias too;
  * a second forward + backward gives identical bits.
tests/test_train_wide_cases.py holds, on the CPU, what the case table needs for that to be a fair comparison (the ReLUs that cannot be
gate-imposed and the PPO kinks are nowhere near their thresholds); the seed of a case is 1000 + sum(map(ord, name)) + k with the first k that
meets those conditions.

Measured on an MI355X (bars: values and log-probs 1e-4; gradients 5e-4 of the tensor's largest entry + 1e-7):
  case                  k  values  log-probs  worst relative gradient error                   gate units that differ from fp64
  h49_first             0  3.9e-6  4.4e-6     4.8e-5 (attn.temporal_edge_layer.0.weight)      0
  h64_all               4  3.2e-6  4.1e-6     2.8e-4 (attn.temporal_edge_layer.0.bias)        0
  h64_boundaries_d12   10  3.6e-6  3.1e-6     9.2e-5 (attn.temporal_edge_layer.0.weight)      0
  h50_one_human        14  4.0e-6  7.1e-6     1.4e-5 (spatial_attn.embedding_layer.0.bias)    0
  h50_mixed           124  4.6e-6  5.8e-6     1.4e-5 (attn.spatial_edge_layer.0.weight)       2 (|fp64 pre-activation| <= 2.2e-6)
  h64_sharp             2  3.4e-6  1.9e-6     3.7e-3 (attn.temporal_edge_layer.0.weight)      0
The rollout goldens at 49, 50 and 64 humans (tests/golden/rollout_*.npz through tests/test_gpu_ppo.py) hold the 1e-5 loss bar in both gemm
modes: no fixture needed another bar.

h64_sharp is the one case that does not run the freshly initialised weights.  At those the robot-human softmax is uniform (see SHARPEN below and
tests/test_train_wide_cases.py), so the five cases above cannot see the sequence's temperature: a library whose cn_rn_seq_fwd / _bwd form
it with min(H, 48) passes all five (values within 4.3e-6) and is caught only by the direct cases of tests/rn_seq_util.py.  With the two
projections x32 the same library misses this case's gradient bar by 30x (spatial_attn.q_linear.weight), and one that stops the robot-human
scores at row 32 by 90x.  In this case the tensors behind the scores pass on the bar's absolute term: temporal_edge_layer.0.weight 3.7e-9
against a largest entry of 8.5e-7, q_linear.weight 2.2e-8 against 1.2e-5 (1.8e-3).  The softmax backward g_j = T p_j (dp_j - sum p dp)
cancels there: the float32 torch-op graph on the CPU is 1.0e-3 (temporal_edge_layer.0.weight) and 1.5e-4 (q_linear.weight) away from fp64 on
the same minibatch, so these are the conditioning of the tensors at this shape, with the split-precision products on top, not a lost term.
"""
import copy
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.test_gpu_minibatch_edges import _counts_const, _counts_ragged  # noqa: E402

# T, N, E, H, D, detected counts, counts the minibatch must contain, edge, seed offset k (see the module docstring)
CASES = {
    "h49_first": (2, 3, 4, 49, 2, _counts_ragged(48, 49), (48, 49), "first H outside the step's box; one sample with 49 live rows", 0),
    "h64_all": (2, 3, 5, 64, 2, _counts_const(64), (64,), "only the 64-wide class, every tile full: the box edge", 4),
    "h64_boundaries_d12": (3, 4, 5, 64, 12, _counts_ragged(1, 8, 9, 16, 17, 32, 33, 48, 49, 64), (1, 8, 9, 16, 17, 32, 33, 48, 49, 64),
                           "every class boundary, widest observation", 10),
    "h50_one_human": (4, 5, 6, 50, 2, _counts_const(1), (1,), "rows == B at a wide H: a softmax over one element under temperature 50 / 8", 14),
    "h50_mixed": (5, 8, 9, 50, 2, _counts_ragged(1, 50), (1, 50), "the crowd size of BASELINE configs[4]; N < E, one all-ones and one all-zeros mask env", 124),
    "h64_sharp": (2, 3, 5, 64, 2, _counts_ragged(33, 64), (33, 64), "a robot-human softmax that is not uniform (SHARPEN): the temperature 64 / 8 and the rows past 32 carry weight", 2),
}
# At the freshly initialised weights the robot-human scores are ~1e-4 and the softmax is uniform to three digits (0.016 = 1 / 64 everywhere at
# H = 64): the temperature H / sqrt(A) cancels out of the forward, and the gradients that pass through the scores (temporal_edge_layer,
# spatial_edge_layer: largest entry ~1e-7) sit at the absolute term of the gradient bar.  A case listed here has the weights of those two
# projections multiplied by the factor (a power of two: the same bits on both sides) in the CPU and the GPU policy before the call, so the
# scores grow by its square: x32 gives attention maxima of 0.09 to 0.76 per sample.  The rollout in the storage stays the unscaled policy's.
SHARPEN = {"h64_sharp": 32.0}
CLIP, VCOEF = 0.2, 0.5
FORWARD_BAR = 1e-4


def seed_of(case, k=None):
    return 1000 + sum(map(ord, case)) + (CASES[case][8] if k is None else k)


def sharpen(case, *policies):
    """SHARPEN[case] applied to the robot-human projections of every given policy (nothing for the other cases)."""
    f = SHARPEN.get(case)
    if f is not None:
        with torch.no_grad():
            for pol in policies:
                pol.base.attn.temporal_edge_layer[0].weight.mul_(f)
                pol.base.attn.spatial_edge_layer[0].weight.mul_(f)


def _minibatch(ro, adv, idx, T):
    """What RolloutStorage.recurrent_generator yields for the env group `idx` (storage.py: take())."""
    idx = idx.to(ro.rewards.device)
    N = idx.numel()

    def take(x):
        g = x[:T].index_select(1, idx)
        return g.reshape(T * N, *g.shape[2:])
    obs = {k: take(v) for k, v in ro.obs.items()}
    hxs = {"human_node_rnn": ro.recurrent_hidden_states["human_node_rnn"][0].index_select(0, idx)}
    return obs, hxs, take(ro.actions), take(ro.value_preds), take(ro.returns), take(ro.masks), take(ro.action_log_probs), take(adv)


def _bucket_grads(pol, g):
    off, out = 0, {}
    for name, p in pol.named_parameters():
        k = p.numel()
        out[name] = g[off:off + k].view_as(p).cpu().double()
        off += (k + 3) // 4 * 4
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_wide_crowd_training_route_matches_the_gated_fp64_graph(case, monkeypatch):
    """See the module docstring; the case table is CASES."""
    from crowdnav_prediction_attngraph_amd import hip
    from crowdnav_prediction_attngraph_amd.ppo import PPO
    from tests import relu_gate_util as G
    from tests.test_gpu_minibatch_edges import _pair
    from tests.test_gpu_minibatch_step import _cpu_grads_in_chunks
    T, N, E, H, D, counts, must, edge, _ = CASES[case]
    B = T * N
    assert B <= 40
    pol_c, ro_c, pol, ro, idx, det = _pair(T, N, E, H, D, counts, seed_of(case))
    sharpen(case, pol_c, pol)
    base = pol.base
    assert base.train_gemm_mode == "bf16x3" and base.train_fused_hh and base.train_fused_rn and base.sized_rn_ok()
    agent = PPO(pol, CLIP, 2, 1, VCOEF, 0.0, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
    flat = agent._bind_flat()
    assert not hip.MinibatchStepper.supported(pol, ro) and not agent._fast_path(ro)
    adv = agent._advantages(ro)
    live = det[:T][:, idx.numpy()]
    rows = int(live.sum())
    assert set(must) <= set(live.reshape(-1).tolist()), live
    gates = G.record_gpu_gates(monkeypatch)

    def run():
        obs_b, hxs_b, act_b, vp_b, ret_b, m_b, olp_b, adv_b = _minibatch(ro, adv, idx, T)
        values, logp, ent, _ = pol.evaluate_actions(obs_b, hxs_b, m_b, act_b)
        vl, al = agent._losses(values, logp, olp_b, adv_b, vp_b, ret_b)
        flat.g.zero_()
        (vl * agent.value_loss_coef + al - ent * agent.entropy_coef).backward()
        flat.claim_grads(copy_in=True)
        torch.cuda.synchronize()
        return values.detach().clone(), logp.detach().clone(), torch.stack([vl.detach(), al.detach(), ent.detach()]), flat.g.clone()

    v1, lp1, l1, g1 = run()
    v2, lp2, l2, g2 = run()                                               # deterministic: a second forward + backward gives identical bits
    assert len(gates) == 6 and [tuple(g.shape) for g in gates[:3]] == [(rows, 128), (rows, 512), (rows, 256)], [tuple(g.shape) for g in gates]
    assert torch.equal(v1, v2) and torch.equal(lp1, lp2) and torch.equal(l1, l2)
    assert all(torch.equal(a, b) for a, b in zip(gates[:3], gates[3:]))
    assert bool(torch.isfinite(g1).all())
    got, again = _bucket_grads(pol, g1), _bucket_grads(pol, g2)
    for k in got:
        assert torch.equal(got[k], again[k]), k

    # fp64: the graph as it is (forward, losses, its own gates), then with the GPU's gates at the block's three ReLUs (gradients)
    pol64 = pol_c.double()
    with G.relu_taps() as pre:
        v_c, lp_c, sums_c, _ = _cpu_grads_in_chunks(pol64, ro_c, adv.cpu(), idx, T, H, CLIP, VCOEF, chunk=N)
    assert len(pre) == 6 and [tuple(p.shape) for p in pre] == [(B, 256), (rows, 128), (rows, 512), (rows, 256), (B, 64), (B, 64)]
    diffs = G.gate_differences(gates, pre)
    with G.relu_taps(gates[:3]) as pre_g:
        _, _, _, g_c = _cpu_grads_in_chunks(pol64, ro_c, adv.cpu(), idx, T, H, CLIP, VCOEF, chunk=N)
    assert len(pre_g) == 6
    v_g, lp_g = v1.view(B).cpu().double(), lp1.view(B).cpu().double()
    ev, elp = float((v_c - v_g).abs().max()), float((lp_c - lp_g).abs().max())
    table = []
    for k, want in g_c.items():
        scale = float(want.abs().max())
        err = float((want - got[k]).abs().max())
        table.append((err / max(scale, 1e-6), k, err, scale))
    table.sort(reverse=True)
    for row in table[:6]:
        print("%.2e  %-60s err %.3e  max %.3e" % row)
    print("%s (T=%d N=%d E=%d H=%d D=%d, %d rows, seed %d): values %.2e  log-probs %.2e  worst relative gradient error %.2e (%s)"
          % (case, T, N, E, H, D, rows, seed_of(case), ev, elp, table[0][0], table[0][1]))
    for name, (n, worst) in zip(G.RELU_CALLS[1:4], diffs):
        print("%s gates of %-7s %d units differ from fp64, largest |fp64 pre-activation| among them %.2e" % (case, name, n, worst))
    print("%s gate units that differ from fp64: %d" % (case, sum(n for n, _ in diffs)))
    assert ev <= FORWARD_BAR, ev
    assert elp <= FORWARD_BAR, elp
    np.testing.assert_allclose(l1[:2].cpu().double().numpy(), sums_c.numpy(), rtol=2e-4, atol=1e-6)
    ent = 0.5 + 0.5 * math.log(2 * math.pi) + float(pol_c.dist.logstd._bias.detach().mean())
    assert abs(float(l1[2]) - ent) <= 1e-6
    for name, (n, worst) in zip(G.RELU_CALLS[1:4], diffs):               # a missing or garbage activation breaks this at once
        assert worst <= FORWARD_BAR, (name, n, worst)
    for rel, k, err, scale in table:
        assert err <= 5e-4 * scale + 1e-7, (k, err, scale)
    for k in got:
        if k not in g_c:                                                  # parameters the loss does not reach: exact zeros, as None on the CPU
            assert k.startswith("base.human_node_final_linear"), k
            assert float(got[k].abs().max()) == 0.0, k
    # the softmax cannot see spatial_edge_layer's bias: an exact zero on the GPU (the fp64 graph leaves its rounding there, ~1e-18)
    assert float(got["base.attn.spatial_edge_layer.0.bias"].abs().max()) == 0.0


def test_crowds_past_48_humans_are_routed_around_the_minibatch_step(monkeypatch):
    """hip.MinibatchStepper.supported and the C workspace query refuse H = 49 and take H = 48 from the same builder, and PPO.update on the
    h49_first storage runs to finite losses without a single call of the step."""
    from crowdnav_prediction_attngraph_amd import _abi as A
    from crowdnav_prediction_attngraph_amd import hip
    from crowdnav_prediction_attngraph_amd.ppo import PPO
    from tests.test_gpu_minibatch_edges import _pair
    T, N, E, H, D, counts, _, _, _ = CASES["h49_first"]
    _, _, pol, ro, _, _ = _pair(T, N, E, H, D, counts, seed_of("h49_first"))
    _, _, pol48, ro48, _, _ = _pair(T, N, E, 48, D, _counts_ragged(47, 48), seed_of("h49_first"))
    assert not hip.MinibatchStepper.supported(pol, ro) and not hip.SizedMinibatchStepper.supported(pol, ro)
    assert hip.MinibatchStepper.supported(pol48, ro48)
    rows = T * N * 20                                                    # inside [B, B * H] for both crowd sizes
    L = A.lib()
    assert L.cn_ppo_minibatch_workspace_bytes(T, N, 49, D, rows) == 0 and L.cn_ppo_minibatch_workspace_bytes(T, N, 48, D, rows) > 0

    def no_step(self, *a, **k):
        raise AssertionError("cn_ppo_minibatch_step was launched for a crowd of 49 humans")
    monkeypatch.setattr(hip.MinibatchStepper, "step", no_step)
    agent = PPO(copy.deepcopy(pol), CLIP, 2, 2, VCOEF, 0.01, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
    assert not agent._fast_path(ro)
    torch.manual_seed(123)
    out = agent.update(ro)
    assert len(out) == 3 and all(math.isfinite(x) for x in out), out
