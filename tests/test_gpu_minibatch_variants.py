"""-m gpu: cn_ppo_minibatch_step_variant -- the one-call PPO minibatch step with use_self_attn and / or sort_humans off (cn_ppo_variant) --
through hip.MinibatchStepper / hip.SizedMinibatchStepper and ppo.PPO.update.

  1. the step against the torch-op graph on the CPU in fp64 (evaluate_actions of the CPU mirror in double with the same switches: its
     counted_inputs CPU branch is the definition of the unsorted form), one call per case on a shuffled strict subset of the storage's envs
     (the N == E case apart), one env with done masks all 1 and one with masks all 0, a random visible_masks (p = 0.5), in every unsorted case
     the masks all-invisible / all-visible / only-the-last-human planted in the minibatch's first three samples, at the bars of
     tests/test_gpu_minibatch_edges.py and tests/test_gpu_minibatch_sized.py: values and log-probs of ALL samples 1e-4 absolute, value and action
     loss rtol 2e-4 / atol 1e-6, the entropy 1e-6 against its closed form, every gradient 5e-4 of the fp64 tensor's largest entry + 1e-7;
     NaN-filled bucket, every covered gradient finite, human_node_final_linear keeps the fill, unreached parameters exact zeros, a second call
     identical bits, rows == row_totals[idx].sum() == the host count of max(1, visible);
  2. the compacting gather, bit for bit: the step on the unsorted storage == the step of a sort_humans = True policy with the same weights on a
     copy of the storage compacted by hip.compact_visible;
  3. the workspace: exactly cn_ppo_minibatch_workspace_bytes_variant bytes with a NaN guard tail behind it, one byte less refused, the
     no-attention query smaller than the default one;
  4. v = NULL and {1, 1, NULL}: the bits of cn_ppo_minibatch_step_sized, at the default tuple and at (192, 64, 48, 320);
  5. sort_humans = 0 without visible_masks: CN_ERR_INVALID naming the field, nothing launched;
  6. routing: PPO.update takes the step once per optimiser step for each variant, never with use_minibatch_step = False;
  7. one PPO.update through the step against the autograd-joined producer (bars of tests/test_gpu_minibatch_step.py for that comparison);
  8. the reference's two PPO.update goldens with the switches set (tests/golden/rollvar_*.npz) through the step.

Each case of 1 is the smallest shape that reaches its edge (CASES).  First seed of a case: 1000 + sum(map(ord, name)).  A gradient miss with
values and log-probs inside 1e-4 is diagnosed as tests/test_gpu_minibatch_edges.py describes before any re-seed: impose the GPU's ReLU gates in the
fp64 graph and look at what is left.

Measured on an MI355X, worst relative gradient error per case (error / largest fp64 entry of the tensor; the bar is 5e-4):
  noattn_smallest   12 rows                 3.2e-5  (attn.spatial_edge_layer.0.weight)   values 2.6e-6  log-probs 5.3e-6
  noattn_ragged     147 rows                1.4e-5  (spatial_linear.2.weight)            values 4.8e-6  log-probs 7.4e-6
  noattn_rows_b     2 rows                  1.5e-5  (critic.2.weight)                    values 6.3e-6  log-probs 1.7e-6
  unsorted_planted  10 rows                 2.5e-5  (spatial_attn.q_linear.weight)       values 2.5e-6  log-probs 1.2e-6
  unsorted_h48      122 rows                6.9e-5  (attn.spatial_edge_layer.0.weight)   values 1.6e-6  log-probs 5.4e-7
  unsorted_h33      99 rows                 2.0e-5  (spatial_attn.q_linear.weight)       values 5.6e-6  log-probs 2.0e-6
  both_h10          38 rows                 2.2e-5  (critic.0.bias)                      values 1.6e-6  log-probs 2.8e-6
  both_sized        128 rows                2.0e-5  (attn.temporal_edge_layer.0.weight)  values 5.6e-6  log-probs 4.3e-6
(unsorted_h48: the three attn.* tensors of that storage have largest entries of 5e-8, so their absolute error of 7e-11 sits far under the bar's
1e-7 floor; the next tensor of the case is at 1.3e-5.)  No case missed a bar with its first seed: nothing was re-seeded and there is no diagnosis
to record.
"""
import copy
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from crowdnav_prediction_attngraph_amd import _abi as A  # noqa: E402

SIZED = (192, 64, 48, 320)
# name: (use_self_attn, sort_humans, (R, M, A, O), T, N, E, H, D, edge)
CASES = {
    "noattn_smallest": (False, True, A.DEFAULT_DIMS, 2, 3, 5, 3, 2, "smallest"),
    "noattn_ragged": (False, True, A.DEFAULT_DIMS, 3, 17, 19, 5, 12, "rows past one 64-row tile with a ragged last tile; N past one GRU workgroup"),
    "noattn_rows_b": (False, True, A.DEFAULT_DIMS, 1, 2, 3, 1, 16, "rows == B; widest D"),
    "unsorted_planted": (True, False, A.DEFAULT_DIMS, 2, 3, 5, 3, 2, "planted masks"),
    "unsorted_h48": (True, False, A.DEFAULT_DIMS, 2, 3, 4, 48, 2, "widest crowd"),
    "unsorted_h33": (True, False, A.DEFAULT_DIMS, 2, 3, 4, 33, 12, "mask past bit 31 of the ballot"),
    "both_h10": (False, False, A.DEFAULT_DIMS, 2, 4, 4, 10, 12, "shape of polvar_pred_h10_noattn_unsorted; N == E"),
    "both_sized": (False, False, SIZED, 3, 17, 19, 5, 12, "sized"),
}
UNSORTED = [k for k, c in CASES.items() if c[0] and not c[1]]
VARIANTS = [(False, True), (True, False), (False, False)]
HYPER = (0.2, 0.5, 0.0, True)
OBS_KEYS = ("robot_node", "temporal_edges", "spatial_edges", "detected_human_num", "visible_masks")


def _seed(name):
    return 1000 + sum(map(ord, name))


def _policy(attn, srt, dims, T, E, H, D):
    from crowdnav_prediction_attngraph_amd.policy import Policy, make_spaces
    from tests.test_policy_sizes import size_kwargs
    ob_space, act_space = make_spaces(H, D)
    kw = dict(env_name="CrowdSimVarNum-v0" if D == 2 else "CrowdSimPred-v0", num_processes=E, num_mini_batch=1, seq_length=T, use_self_attn=attn,
              sort_humans=srt, **size_kwargs(dims))
    if D not in (2, 12):
        kw["predict_steps"] = D // 2 - 1
    pol = Policy(ob_space.spaces, act_space, base="selfAttn_merge_srnn", base_kwargs=kw)
    pol.base.nenv = E
    assert pol.base.use_self_attn == attn and pol.base.sort_humans == srt
    return pol, ob_space, act_space


def _storage(pol, ob_space, act_space, T, E, H, D, det, vis, env_ones, env_zeros, seed):
    """tests.test_gpu_minibatch_sized._storage with the visibility bytes: sort_humans on, the humans are ordered by distance and the ones past the
    detected count are 15.0; off, they stay in index order (NOT ordered by detection), the invisible ones are 15.0 (what the simulator writes) and
    detected_human_num is max(1, visible)."""
    from crowdnav_prediction_attngraph_amd.trainer import new_rollouts
    rs = np.random.RandomState(seed)
    n = (T + 1) * E
    R = pol.base.dims[0]
    ro = new_rollouts(pol, T, E, ob_space.spaces, act_space)
    robot = np.concatenate([rs.uniform(-6, 6, (n, 2)), np.full((n, 1), 0.3), rs.uniform(-6, 6, (n, 2)), np.ones((n, 1)), np.full((n, 1), np.pi / 2)], 1)
    p = rs.uniform(-4, 4, (n, H, 2))
    if pol.base.sort_humans:
        p = np.take_along_axis(p, np.argsort(np.linalg.norm(p, axis=2), axis=1)[:, :, None], 1)
    v = rs.uniform(-1, 1, (n, H, 2))
    se = np.concatenate([p + 0.25 * k * v for k in range(D // 2)], 2)
    if pol.base.sort_humans:
        se[np.arange(H)[None, :] >= det.reshape(n, 1)] = 15.0
    else:
        se[~vis.reshape(n, H)] = 15.0
    ro.obs["robot_node"].copy_(torch.from_numpy(robot.astype(np.float32)).view(T + 1, E, 1, 7))
    ro.obs["temporal_edges"].copy_(torch.from_numpy(rs.uniform(-1, 1, (n, 2)).astype(np.float32)).view(T + 1, E, 1, 2))
    ro.obs["spatial_edges"].copy_(torch.from_numpy(se.astype(np.float32)).view(T + 1, E, H, D))
    ro.obs["detected_human_num"].copy_(torch.from_numpy(det.astype(np.float32)).view(T + 1, E, 1))
    ro.obs["visible_masks"].copy_(torch.from_numpy(vis).view(T + 1, E, H))
    g = torch.Generator().manual_seed(seed + 9)
    ro.recurrent_hidden_states["human_node_rnn"].copy_(0.5 * torch.randn(T + 1, E, 1, R, generator=g))
    ro.masks.copy_((torch.rand(T + 1, E, 1, generator=g) > 0.15).float())
    ro.masks[:, env_ones] = 1.0
    if env_zeros is not None:
        ro.masks[:, env_zeros] = 0.0
    ro.actions.copy_(torch.randn(T, E, 2, generator=g))
    ro.rewards.copy_(0.2 * torch.randn(T, E, 1, generator=g))
    with torch.no_grad():
        flat = {k: ro.obs[k][:T].reshape(T * E, *ro.obs[k].shape[2:]) for k in OBS_KEYS}
        val, lp, _, _ = pol.evaluate_actions(flat, {"human_node_rnn": ro.recurrent_hidden_states["human_node_rnn"][0]}, ro.masks[:T].reshape(T * E, 1),
                                             ro.actions.reshape(T * E, 2))
    ro.value_preds[:T].copy_((val + 0.15 * torch.randn(T * E, 1, generator=g)).view(T, E, 1))
    ro.action_log_probs.copy_((lp + 0.2 * torch.randn(T * E, 1, generator=g)).view(T, E, 1))
    return ro, torch.randn(E, 1, generator=g)


def _counts(srt, T, N, E, H, idx, seed):
    """(detected counts [T + 1, E], visibility [T + 1, E, H]).  sort_humans on: counts uniform in 1..H with 1 and H planted at the minibatch's first
    two samples (sample s = t * N + j reads env idx[j] at step t), a random visibility nobody reads.  Off: visibility with p = 0.5, the masks
    all-invisible, all-visible and only-the-last-human planted at the first three samples, counts = max(1, visible)."""
    rs = np.random.RandomState(seed)
    vis = rs.rand(T + 1, E, H) < 0.5
    if srt:
        det = rs.randint(1, H + 1, size=(T + 1, E))
        for s, c in enumerate((1, H)[:T * N]):
            det[s // N, int(idx[s % N])] = c
        return det, vis
    last = np.zeros(H, dtype=bool)
    last[H - 1] = True
    for s, m in enumerate((np.zeros(H, dtype=bool), np.ones(H, dtype=bool), last)[:T * N]):
        vis[s // N, int(idx[s % N])] = m
    return np.maximum(vis.sum(-1), 1), vis


def _pair(attn, srt, dims, T, N, E, H, D, seed):
    """(CPU policy, CPU storage, their GPU copies, env_idx [N], rows per sample [T + 1, E]); the minibatch holds the all-ones env and the all-zeros env."""
    torch.manual_seed(seed)
    pol_c, ob_space, act_space = _policy(attn, srt, dims, T, E, H, D)
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(seed + 1))
    idx = perm[:N]
    env_ones, env_zeros = int(perm[0]), int(perm[1])
    det, vis = _counts(srt, T, N, E, H, idx, seed + 2)
    ro_c, next_value = _storage(pol_c, ob_space, act_space, T, E, H, D, det, vis, env_ones, env_zeros, seed + 3)
    pol = copy.deepcopy(pol_c).cuda()
    ro = copy.deepcopy(ro_c)
    ro.to(torch.device("cuda"))
    ro.compute_returns(next_value.cuda(), True, 0.99, 0.95, False)
    ro_c.compute_returns(next_value, True, 0.99, 0.95, False)
    return pol_c, ro_c, pol, ro, idx, det


def _case_pair(case):
    attn, srt, dims, T, N, E, H, D, _ = CASES[case]
    return _pair(attn, srt, dims, T, N, E, H, D, _seed(case))


def _bound(pol):
    from crowdnav_prediction_attngraph_amd.ppo import PPO
    agent = PPO(pol, 0.2, 2, 1, 0.5, 0.0, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
    agent._bind_flat()
    return agent


def _stepper(pol, ro):
    """The stepper ppo.PPO would build: the unsized class at the default tuple, the sized one elsewhere."""
    from crowdnav_prediction_attngraph_amd import hip
    if tuple(pol.base.dims) == A.DEFAULT_DIMS:
        assert hip.MinibatchStepper.supported(pol, ro)
        return hip.MinibatchStepper(pol)
    assert hip.SizedMinibatchStepper.supported(pol, ro) and not hip.MinibatchStepper.supported(pol, ro)
    return hip.SizedMinibatchStepper(pol)


def _fp64_graph(pol64, ro, adv, idx, T, clip, vcoef):
    """tests.test_gpu_minibatch_step._cpu_grads_in_chunks in one chunk, with the visibility bytes among the inputs."""
    N = idx.numel()
    B = T * N
    for p in pol64.parameters():
        p.grad = None

    def take(x, double=True):
        g = x[:T].index_select(1, idx)
        return (g.double() if double else g).reshape(B, *g.shape[2:])
    obs = {k: take(ro.obs[k], k != "visible_masks") for k in OBS_KEYS}
    h0 = ro.recurrent_hidden_states["human_node_rnn"][0].index_select(0, idx).double()
    v, lp, _, _ = pol64.evaluate_actions(obs, {"human_node_rnn": h0}, take(ro.masks), take(ro.actions))
    olp, a, vp, ret = take(ro.action_log_probs), take(adv), take(ro.value_preds), take(ro.returns)
    ratio = torch.exp(lp - olp)
    al = -torch.min(ratio * a, torch.clamp(ratio, 1 - clip, 1 + clip) * a).sum() / B
    vpc = vp + (v - vp).clamp(-clip, clip)
    vl = 0.5 * torch.max((v - ret).pow(2), (vpc - ret).pow(2)).sum() / B
    (vl * vcoef + al).backward()
    grads = {k: p.grad for k, p in pol64.named_parameters() if p.grad is not None}
    return v.detach().reshape(B), lp.detach().reshape(B), torch.stack([vl.detach(), al.detach()]), grads


def _bucket(pol, g):
    """{parameter name: its slice of the flat bucket g} (every slice starts on a multiple of four floats)."""
    off, out = 0, {}
    for name, p in pol.named_parameters():
        k = p.numel()
        out[name] = g[off:off + k]
        off += (k + 3) // 4 * 4
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_variant_minibatch_step_matches_the_fp64_cpu_graph(case):
    """See the module docstring; the case table is CASES."""
    attn, srt, dims, T, N, E, H, D, edge = CASES[case]
    pol_c, ro_c, pol, ro, idx, det = _case_pair(case)
    agent = _bound(pol)
    assert N < E or case == "both_h10"
    if not attn:
        assert not any(k.startswith("base.spatial_attn.") for k, _ in pol.named_parameters())
    adv = agent._advantages(ro)
    stepper = _stepper(pol, ro)
    assert (stepper.self_attn, stepper.sort_humans) == (attn, srt)
    rows = int(stepper.row_totals(ro)[idx].sum())
    vm = ro_c.obs["visible_masks"][:T][:, idx].numpy()
    host = int(np.maximum(vm.sum(-1), 1).sum()) if not srt else int(det[:T][:, idx.numpy()].sum())
    assert rows == host, (rows, host)
    if case == "noattn_rows_b":
        assert rows == T * N
    if not srt:                                                          # the three planted masks sit in the minibatch's first three samples
        first = vm.reshape(T * N, H)[:3]
        assert not first[0].any() and first[1].all() and first[2].sum() == 1 and first[2, H - 1]
    ro_masks = ro.masks[:T, idx.cuda()]
    assert bool((ro_masks[:, 0] == 1).all()) and bool((ro_masks[:, 1] == 0).all())
    idx_d = idx.to("cuda", torch.int32)
    losses = torch.zeros(3, device="cuda")
    vlp = torch.empty(2, T * N, device="cuda")
    flat = agent._flat
    flat["g"].fill_(float("nan"))                                       # the call must WRITE every gradient
    stepper.step(ro, adv, idx_d, rows, HYPER, losses, vlp)
    torch.cuda.synchronize()
    g1, l1, vlp1 = flat["g"].clone(), losses.clone(), vlp.clone()
    flat["g"].fill_(float("nan"))
    stepper.step(ro, adv, idx_d, rows, HYPER, losses, vlp)               # deterministic: a second call gives identical bits
    torch.cuda.synchronize()
    assert torch.equal(l1, losses) and torch.equal(vlp1, vlp)
    first, second = _bucket(pol, g1), _bucket(pol, flat["g"])
    got = {}
    for name, p in pol.named_parameters():
        got[name] = first[name].view_as(p).cpu().double()
        if name.startswith("base.human_node_final_linear"):              # never reached by the loss: untouched, still the fill
            assert bool(torch.isnan(first[name]).all()) and bool(torch.isnan(second[name]).all()), name
        else:
            assert bool(torch.isfinite(first[name]).all()), name
            assert torch.equal(first[name], second[name]), name
    v_c, lp_c, sums_c, g_c = _fp64_graph(pol_c.double(), ro_c, adv.cpu(), idx, T, 0.2, 0.5)
    v_g, lp_g = vlp1[0].cpu().double(), vlp1[1].cpu().double()
    ev, elp = float((v_c - v_g).abs().max()), float((lp_c - lp_g).abs().max())
    table = []
    for k, want in g_c.items():
        scale = float(want.abs().max())
        err = float((want - got[k]).abs().max())
        table.append((err / max(scale, 1e-6), k, err, scale))
    table.sort(reverse=True)
    for row in table[:6]:
        print("%.2e  %-60s err %.3e  max %.3e" % row)
    print("%s attn=%d sorted=%d %s (T=%d N=%d E=%d H=%d D=%d, %d rows): values %.2e  log-probs %.2e  worst relative gradient error %.2e (%s)"
          % (case, attn, srt, dims, T, N, E, H, D, rows, ev, elp, table[0][0], table[0][1]))
    assert ev <= 1e-4, ev
    assert elp <= 1e-4, elp
    np.testing.assert_allclose(l1[:2].cpu().double().numpy(), sums_c.numpy(), rtol=2e-4, atol=1e-6)
    ent = 0.5 + 0.5 * math.log(2 * math.pi) + float(pol_c.dist.logstd._bias.detach().mean())
    assert abs(float(l1[2]) - ent) <= 1e-6
    for rel, k, err, scale in table:
        assert err <= 5e-4 * scale + 1e-7, (k, err, scale)
    for k in got:
        if k not in g_c and not k.startswith("base.human_node_final_linear"):     # parameters the loss does not reach: exact zeros
            assert float(got[k].abs().max()) == 0.0, k


def _raw_variant(stepper, ro, adv, idx, rows, dims, v, ws_ptr, ws_bytes, losses, vlp):
    """cn_ppo_minibatch_step_variant called directly (no wrapper, no workspace cache): the status, and the library's message."""
    base = stepper.policy.base
    T, E = ro.rewards.shape[0], ro.rewards.shape[1]
    b = A.PpoBatch(T, int(idx.numel()), E, base.human_num, base.edge_width)
    ts = dict(env_idx=idx, robot_node=ro.obs["robot_node"], temporal_edges=ro.obs["temporal_edges"], spatial_edges=ro.obs["spatial_edges"],
              detected_human_num=ro.obs["detected_human_num"], h0=ro.recurrent_hidden_states["human_node_rnn"], masks=ro.masks, actions=ro.actions,
              value_preds=ro.value_preds, returns=ro.returns, old_logp=ro.action_log_probs, adv=adv)
    for k in A.PPO_BATCH_TENSORS:
        setattr(b, k, ts[k].data_ptr())
    w, g = stepper._structs()
    hy = A.PpoHyper(HYPER[0], HYPER[1], HYPER[2], 1)
    L = A.lib()
    with torch.cuda.device(ro.rewards.device):
        rc = L.cn_ppo_minibatch_step_variant(C.byref(b), rows, C.byref(w), C.byref(g), C.byref(hy), None if dims is None else C.byref(dims),
                                             None if v is None else C.byref(v), C.c_void_p(ws_ptr), ws_bytes, A.ptr(losses), A.ptr(vlp), A.stream_ptr())
    return rc, L.cn_last_error().decode()


@pytest.mark.parametrize("case", UNSORTED)
def test_the_compacting_gather_equals_a_compacted_storage_bit_for_bit(case):
    """The step on the unsorted storage against the step of a sort_humans = True policy with the same weights on a copy of that storage whose
    spatial_edges went through hip.compact_visible and whose detected_human_num is its count: losses, values / log-probs and the whole bucket."""
    from crowdnav_prediction_attngraph_amd import hip
    attn, srt, dims, T, N, E, H, D, _ = CASES[case]
    _, _, pol, ro, idx, _ = _case_pair(case)
    pol_s, _, _ = _policy(attn, True, dims, T, E, H, D)
    pol_s.load_state_dict(pol.state_dict())
    pol_s = pol_s.cuda()
    ro_s = copy.deepcopy(ro)
    se, det = hip.compact_visible(ro.obs["spatial_edges"].view((T + 1) * E, H, D), ro.obs["visible_masks"].view((T + 1) * E, H))
    ro_s.obs["spatial_edges"].copy_(se.view(T + 1, E, H, D))
    ro_s.obs["detected_human_num"].copy_(det.view(T + 1, E, 1))
    assert not torch.equal(ro_s.obs["spatial_edges"], ro.obs["spatial_edges"])
    idx_d = idx.to("cuda", torch.int32)
    res = []
    for p, r in ((pol, ro), (pol_s, ro_s)):
        agent = _bound(p)
        adv = agent._advantages(r)
        stepper = _stepper(p, r)
        rows = int(stepper.row_totals(r)[idx].sum())
        losses, vlp = torch.full((3,), float("nan"), device="cuda"), torch.full((2, T * N), float("nan"), device="cuda")
        agent._flat["g"].fill_(float("nan"))
        stepper.step(r, adv, idx_d, rows, HYPER, losses, vlp)
        torch.cuda.synchronize()
        res.append((rows, losses.clone(), vlp.clone(), torch.nan_to_num(agent._flat["g"], nan=7.0).clone()))
    assert res[0][0] == res[1][0]
    assert bool(torch.isfinite(res[0][1]).all()) and bool(torch.isfinite(res[0][2]).all())
    for a, b in zip(res[0][1:], res[1][1:]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("case", ["noattn_ragged", "both_sized"])
def test_the_step_stays_inside_the_workspace_the_variant_query_reports(case):
    """The call through the C entry point with a workspace of exactly cn_ppo_minibatch_workspace_bytes_variant bytes, NaN-filled, and a NaN guard
    tail behind it: the tail is untouched, the results are those of the wrapper, one byte less is CN_ERR_INVALID, and the query of the
    no-attention variant is smaller than the default query at the same shape."""
    attn, srt, dims, T, N, E, H, D, _ = CASES[case]
    _, _, pol, ro, idx, _ = _case_pair(case)
    agent = _bound(pol)
    adv = agent._advantages(ro)
    stepper = _stepper(pol, ro)
    rows = int(stepper.row_totals(ro)[idx].sum())
    idx_d = idx.to("cuda", torch.int32)
    d = A.PolicyDims(*dims)
    v = stepper._variant(ro)
    assert (v.self_attn, v.sort_humans) == (0, int(srt)) and (v.visible_masks is None) == srt
    L = A.lib()
    need = int(L.cn_ppo_minibatch_workspace_bytes_variant(T, N, H, D, rows, C.byref(d), C.byref(v)))
    assert 0 < need < int(L.cn_ppo_minibatch_workspace_bytes_sized(T, N, H, D, rows, C.byref(d))) and need % 256 == 0
    guard = 4096
    buf = torch.full((need // 4 + guard,), float("nan"), device="cuda")
    assert buf.data_ptr() % 256 == 0
    losses, vlp = torch.zeros(3, device="cuda"), torch.empty(2, T * N, device="cuda")
    flat = agent._flat
    flat["g"].fill_(float("nan"))
    rc, msg = _raw_variant(stepper, ro, adv, idx_d, rows, d, v, buf.data_ptr(), need, losses, vlp)
    torch.cuda.synchronize()
    assert rc == 0, msg
    assert bool(torch.isnan(buf[need // 4:]).all()), "the guard tail behind the workspace was written"
    g1, l1, vlp1 = flat["g"].clone(), losses.clone(), vlp.clone()
    flat["g"].fill_(float("nan"))
    stepper.step(ro, adv, idx_d, rows, HYPER, losses, vlp)               # the wrapper's own (larger, cached) workspace: the same bits
    torch.cuda.synchronize()
    assert torch.equal(l1, losses) and torch.equal(vlp1, vlp) and torch.equal(torch.nan_to_num(g1, nan=7.0), torch.nan_to_num(flat["g"], nan=7.0))
    flat["g"].fill_(float("nan"))
    losses.fill_(float("nan"))
    rc, msg = _raw_variant(stepper, ro, adv, idx_d, rows, d, v, buf.data_ptr(), need - 1, losses, vlp)
    torch.cuda.synchronize()
    assert rc == -1 and "workspace of" in msg, (rc, msg)                 # CN_ERR_INVALID
    assert bool(torch.isnan(flat["g"]).all()) and bool(torch.isnan(losses).all())


@pytest.mark.parametrize("dims", [A.DEFAULT_DIMS, SIZED], ids=["default", "sized"])
def test_null_and_the_all_on_variant_change_no_bit(dims):
    """cn_ppo_minibatch_step_sized against cn_ppo_minibatch_step_variant with v = NULL and with {1, 1, NULL} on one minibatch (T = 3, N = 5, E = 7,
    H = 6, D = 2) of the default network, NaN-filled buckets: bucket, losses and values / log-probs equal bit for bit, and so is the workspace size."""
    from crowdnav_prediction_attngraph_amd import hip
    from tests.test_gpu_minibatch_sized import _pair as sized_pair, _raw_step
    T, N, E, H, D = 3, 5, 7, 6, 2
    _, _, pol, ro, idx, _ = sized_pair(dims, T, N, E, H, D, seed=2025)
    agent = _bound(pol)
    adv = agent._advantages(ro)
    stepper = hip.SizedMinibatchStepper(pol)
    assert stepper._variant(ro) is None
    rows = int(stepper.row_totals(ro)[idx].sum())
    idx_d = idx.to("cuda", torch.int32)
    L = A.lib()
    d = A.PolicyDims(*dims)
    on = A.PpoVariant(1, 1, None)
    need = int(L.cn_ppo_minibatch_workspace_bytes_sized(T, N, H, D, rows, C.byref(d)))
    assert need == L.cn_ppo_minibatch_workspace_bytes_variant(T, N, H, D, rows, C.byref(d), None) == L.cn_ppo_minibatch_workspace_bytes_variant(T, N, H, D, rows, C.byref(d), C.byref(on))
    flat = agent._flat
    res = []
    for v in ("sized", None, on):
        buf = torch.full((need // 4,), float("nan"), device="cuda")
        losses, vlp = torch.full((3,), float("nan"), device="cuda"), torch.full((2, T * N), float("nan"), device="cuda")
        flat["g"].fill_(float("nan"))
        if v == "sized":
            rc, msg = _raw_step("sized", stepper, ro, adv, idx_d, rows, d, buf.data_ptr(), need, losses, vlp)
        else:
            rc, msg = _raw_variant(stepper, ro, adv, idx_d, rows, d, v, buf.data_ptr(), need, losses, vlp)
        torch.cuda.synchronize()
        assert rc == 0, msg
        res.append((torch.nan_to_num(flat["g"], nan=7.0).clone(), losses.clone(), vlp.clone()))
        assert int(torch.isnan(flat["g"]).sum()) < 2 * dims[3] + 100       # only human_node_final_linear and the bucket's padding keep the fill
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.equal(a, b)
    assert bool(torch.isfinite(res[0][1]).all()) and bool(torch.isfinite(res[0][2]).all())


def test_unsorted_without_the_masks_is_refused_before_any_launch():
    attn, srt, dims, T, N, E, H, D, _ = CASES["unsorted_planted"]
    _, _, pol, ro, idx, _ = _case_pair("unsorted_planted")
    agent = _bound(pol)
    adv = agent._advantages(ro)
    stepper = _stepper(pol, ro)
    rows = int(stepper.row_totals(ro)[idx].sum())
    buf = torch.full((1 << 22,), float("nan"), device="cuda")            # 16 MB: more than this shape needs
    losses = torch.full((3,), float("nan"), device="cuda")
    flat = agent._flat
    for v in (A.PpoVariant(1, 0, None), A.PpoVariant(0, 0, None)):
        flat["g"].fill_(float("nan"))
        rc, msg = _raw_variant(stepper, ro, adv, idx.to("cuda", torch.int32), rows, None, v, buf.data_ptr(), buf.numel() * 4, losses, None)
        torch.cuda.synchronize()
        assert rc == -1, (rc, msg)                                       # CN_ERR_INVALID
        assert "visible_masks" in msg and "sort_humans" in msg, msg
        assert bool(torch.isnan(flat["g"]).all()) and bool(torch.isnan(losses).all()) and bool(torch.isnan(buf).all())


# ---- PPO.update through the step ---------------------------------------------------------------------------------------------------------

def _count_steps(monkeypatch):
    from crowdnav_prediction_attngraph_amd import hip
    calls = []
    real = hip.MinibatchStepper.step                                     # SizedMinibatchStepper inherits it

    def counted(self, *a, **k):
        calls.append((type(self).__name__, self.self_attn, self.sort_humans))
        return real(self, *a, **k)
    monkeypatch.setattr(hip.MinibatchStepper, "step", counted)
    return calls


def _update_pair(attn, srt, T, E, H, seed):
    torch.manual_seed(seed)
    pol_c, ob_space, act_space = _policy(attn, srt, A.DEFAULT_DIMS, T, E, H, 2)
    det, vis = _counts(srt, T, E, E, H, torch.arange(E), seed + 2)
    ro, next_value = _storage(pol_c, ob_space, act_space, T, E, H, 2, det, vis, 0, 1, seed + 3)
    pol = copy.deepcopy(pol_c).cuda()
    ro.to(torch.device("cuda"))
    ro.compute_returns(next_value.cuda(), True, 0.99, 0.95, False)
    return pol, ro


@pytest.mark.parametrize("attn,srt", VARIANTS)
def test_update_routes_every_variant_through_the_step(monkeypatch, attn, srt):
    """T = 4, 8 envs of 5 humans: one update() calls the step ppo_epoch * num_mini_batch times with the policy's switches; with
    use_minibatch_step = False it is never called."""
    from crowdnav_prediction_attngraph_amd import hip
    from crowdnav_prediction_attngraph_amd.ppo import PPO
    pol, ro = _update_pair(attn, srt, 4, 8, 5, seed=91)
    calls = _count_steps(monkeypatch)
    agent = PPO(pol, 0.2, 3, 2, 0.5, 0.01, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
    assert agent._fast_path(ro) and hip.MinibatchStepper.supported(pol, ro)
    res = agent.update(ro)
    assert np.isfinite(res).all()
    assert calls == [("MinibatchStepper", attn, srt)] * 6 and type(agent._stepper) is hip.MinibatchStepper
    del calls[:]
    agent.use_minibatch_step = False
    assert not agent._fast_path(ro)
    agent.update(ro)
    assert calls == []


@pytest.mark.parametrize("attn,srt", VARIANTS)
def test_update_through_the_step_matches_the_autograd_joined_producer(attn, srt):
    """One PPO.update at T = 4, 8 envs of 5 humans, 2 epochs x 2 minibatches, with the step on and off from equal weights and storage: the bars
    tests/test_gpu_minibatch_step.py::test_ppo_update_through_the_minibatch_step_matches_the_cpu_update holds between the two GPU producers
    (losses rtol 1e-5 / atol 1e-6; every tensor max 1.6e-5, mean 1e-7)."""
    from crowdnav_prediction_attngraph_amd.ppo import PPO
    pol_a, ro = _update_pair(attn, srt, 4, 8, 5, seed=41)
    pol_b = copy.deepcopy(pol_a)
    out = []
    for pol, fast in ((pol_a, True), (pol_b, False)):
        agent = PPO(pol, 0.2, 2, 2, 0.5, 0.0, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
        agent.use_minibatch_step = fast
        assert agent._fast_path(ro) == fast
        torch.manual_seed(123)
        out.append((agent.update(ro), {k: v.detach().cpu().double() for k, v in pol.state_dict().items()}))
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=1e-5, atol=1e-6)
    for k, w in out[0][1].items():
        da = (w - out[1][1][k]).abs()
        assert float(da.max()) <= 1.6e-5 and float(da.mean()) <= 1e-7, (k, float(da.max()), float(da.mean()))


from tests.test_policy_variants import ROLL  # noqa: E402


@pytest.mark.parametrize("path", ROLL, ids=lambda p: os.path.basename(p)[8:-4])
def test_reference_golden_updates_go_through_the_step(monkeypatch, path):
    """The reference's PPO.update with the switches set (tests/golden/rollvar_*.npz) replayed on the GPU at atol 2e-6 / rtol 1e-5, every optimiser
    step of it through the one-call step."""
    from crowdnav_prediction_attngraph_amd.policy import Policy, make_spaces
    from tests import policy_util as PU
    from tests.test_policy_variants import check_update_against_the_reference, filled_rollouts
    z = np.load(path)
    meta = json.loads(str(z["meta"]))
    assert not (meta["use_self_attn"] and meta["sort_humans"])
    ob_space, act_space = make_spaces(meta["H"], meta["D"])
    pol = Policy(ob_space.spaces, act_space, base="selfAttn_merge_srnn",
                 base_kwargs=dict(env_name=meta["env_name"], num_processes=meta["E"], num_mini_batch=meta["nmb"], seq_length=meta["T"],
                                  use_self_attn=meta["use_self_attn"], sort_humans=meta["sort_humans"]))
    pol.load_state_dict({k: torch.from_numpy(v) for k, v in PU.formula_state_dict({k: tuple(v) for k, v in meta["shapes"].items()}).items()})
    pol.cuda()
    calls = _count_steps(monkeypatch)
    check_update_against_the_reference(z, meta, pol, filled_rollouts(z, meta, "cuda"), atol=2e-6, rtol=1e-5)
    assert calls == [("MinibatchStepper", meta["use_self_attn"], meta["sort_humans"])] * (meta["ppo_epoch"] * meta["nmb"]) and calls
