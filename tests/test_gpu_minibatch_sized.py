"""-m gpu: cn_ppo_minibatch_step_sized -- the one-call PPO minibatch step at the network sizes (R, M, A, O) of cn_policy_dims, every tuple of the
device box -- through hip.SizedMinibatchStepper and ppo.PPO.update.

  1. the step against the torch-op graph on the CPU in fp64 (tests.test_gpu_minibatch_step._cpu_grads_in_chunks: size-agnostic), one call per
     case on a shuffled strict subset of the storage's envs, one env with masks all 1 and one with masks all 0, at the bars of
     tests/test_gpu_minibatch_edges.py: values and log-probs of ALL samples 1e-4 absolute, value and action loss rtol 2e-4 / atol 1e-6, the
     entropy 1e-6 against its closed form, every gradient 5e-4 of the fp64 tensor's largest entry + 1e-7; NaN-filled bucket, every covered
     gradient finite, human_node_final_linear keeps the fill, unreached parameters exact zeros, a second call identical bits;
  2. the workspace: exactly cn_ppo_minibatch_workspace_bytes_sized bytes with a NaN guard tail behind it, one byte less refused;
  3. the default tuple through the sized entry: the bits of cn_ppo_minibatch_step;
  4. tuples outside the box: CN_ERR_INVALID naming the box, nothing launched;
  5. routing: PPO.update takes the step for a sized policy, once per optimiser step, and never with use_minibatch_step = False;
  6. one PPO.update with the step against the autograd-joined producer (bars of tests/test_gpu_minibatch_step.py for the same comparison);
  7. the reference's PPO.update golden at (192, 64, 48, 320) through the step.

Each case of 1 is the smallest shape that reaches its edge (CASES).  First seed of a case: 1000 + sum(map(ord, name)); all five pass with it.
A future gradient miss with values and log-probs inside 1e-4 is diagnosed as tests/test_gpu_minibatch_edges.py describes before any re-seed:
impose the GPU's ReLU gates, read from the saved activations, in the fp64 graph and look at what is left.

Measured on an MI355X, worst relative gradient error per case (error / largest fp64 entry of the tensor; the bar is 5e-4):
  smallest  (64,64,1,64)       1.8e-5  (attn.spatial_edge_layer.0.weight)    values 3.9e-6  log-probs 1.5e-6
  ragged    (192,64,48,320)    2.0e-5  (spatial_attn.q_linear.weight)        values 7.0e-6  log-probs 6.9e-6
  corner    (256,128,256,512)  1.7e-5  (spatial_attn.k_linear.weight)        values 4.4e-6  log-probs 3.4e-6
  m_only    (128,128,64,256)   1.5e-4  (attn.temporal_edge_layer.0.weight)   values 4.7e-6  log-probs 1.1e-6
  o_only    (128,64,64,448)    1.7e-5  (critic.2.weight)                     values 1.4e-6  log-probs 9.2e-7
(m_only: the three attn.* tensors of that storage have largest entries of 1e-8, so their absolute error of 1.5e-10 sits far under the bar's 1e-7
floor; the next tensor of the case is at 1.8e-5.)  No case missed a bar with its first seed: nothing was re-seeded and there is no diagnosis to record.
"""
import copy
import ctypes as C
import json
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from crowdnav_prediction_attngraph_amd import _abi as A  # noqa: E402

RAGGED = (192, 64, 48, 320)
# name: (R, M, A, O), T, N, E, H, D, edge
CASES = {
    "smallest": ((64, 64, 1, 64), 2, 3, 5, 3, 2, "smallest tuple; one 64-float h0 pass; rank-1 u fold; 3R and O on padded planes with the guarded store"),
    "ragged": (RAGGED, 3, 17, 19, 5, 12, "three h0 passes; streamed GRU; N past one 16-row GRU workgroup; partial K tile in the A fold; five ragged "
                                         "64-tiles in the O folds; the tuple of the reference golden"),
    "corner": ((256, 128, 256, 512), 2, 4, 4, 8, 2, "the corner; N == E; te 384 rows exact"),
    "m_only": ((128, 128, 64, 256), 2, 3, 4, 48, 2, "only M off default, at the widest crowd"),
    "o_only": ((128, 64, 64, 448), 1, 2, 3, 1, 16, "only O off default; one step; rows == B; widest D"),
}
HYPER = (0.2, 0.5, 0.0, True)


def _seed(name):
    return 1000 + sum(map(ord, name))


def _policy(dims, T, E, H, D):
    from crowdnav_prediction_attngraph_amd.policy import Policy, make_spaces
    from tests.test_policy_sizes import size_kwargs
    ob_space, act_space = make_spaces(H, D)
    kw = dict(env_name="CrowdSimVarNum-v0" if D == 2 else "CrowdSimPred-v0", num_processes=E, num_mini_batch=1, seq_length=T, **size_kwargs(dims))
    if D not in (2, 12):
        kw["predict_steps"] = D // 2 - 1
    pol = Policy(ob_space.spaces, act_space, base="selfAttn_merge_srnn", base_kwargs=kw)
    pol.base.nenv = E
    return pol, ob_space, act_space


def _storage(pol, ob_space, act_space, T, E, H, D, det, env_ones, env_zeros, seed):
    """tests.test_gpu_minibatch_edges._edge_storage with the node state as wide as the policy's GRU (trainer.new_rollouts)."""
    from crowdnav_prediction_attngraph_amd.trainer import new_rollouts
    rs = np.random.RandomState(seed)
    n = (T + 1) * E
    R = pol.base.dims[0]
    ro = new_rollouts(pol, T, E, ob_space.spaces, act_space)
    assert ro.recurrent_hidden_states["human_node_rnn"].shape == (T + 1, E, 1, R)
    robot = np.concatenate([rs.uniform(-6, 6, (n, 2)), np.full((n, 1), 0.3), rs.uniform(-6, 6, (n, 2)), np.ones((n, 1)), np.full((n, 1), np.pi / 2)], 1)
    p = rs.uniform(-4, 4, (n, H, 2))
    p = np.take_along_axis(p, np.argsort(np.linalg.norm(p, axis=2), axis=1)[:, :, None], 1)
    v = rs.uniform(-1, 1, (n, H, 2))
    se = np.concatenate([p + 0.25 * k * v for k in range(D // 2)], 2)
    se[np.arange(H)[None, :] >= det.reshape(n, 1)] = 15.0
    ro.obs["robot_node"].copy_(torch.from_numpy(robot.astype(np.float32)).view(T + 1, E, 1, 7))
    ro.obs["temporal_edges"].copy_(torch.from_numpy(rs.uniform(-1, 1, (n, 2)).astype(np.float32)).view(T + 1, E, 1, 2))
    ro.obs["spatial_edges"].copy_(torch.from_numpy(se.astype(np.float32)).view(T + 1, E, H, D))
    ro.obs["detected_human_num"].copy_(torch.from_numpy(det.astype(np.float32)).view(T + 1, E, 1))
    g = torch.Generator().manual_seed(seed + 9)
    ro.recurrent_hidden_states["human_node_rnn"].copy_(0.5 * torch.randn(T + 1, E, 1, R, generator=g))
    ro.masks.copy_((torch.rand(T + 1, E, 1, generator=g) > 0.15).float())
    ro.masks[:, env_ones] = 1.0
    if env_zeros is not None:
        ro.masks[:, env_zeros] = 0.0
    ro.actions.copy_(torch.randn(T, E, 2, generator=g))
    ro.rewards.copy_(0.2 * torch.randn(T, E, 1, generator=g))
    with torch.no_grad():
        flat = {k: ro.obs[k][:T].reshape(T * E, *ro.obs[k].shape[2:]) for k in ("robot_node", "temporal_edges", "spatial_edges", "detected_human_num")}
        val, lp, _, _ = pol.evaluate_actions(flat, {"human_node_rnn": ro.recurrent_hidden_states["human_node_rnn"][0]}, ro.masks[:T].reshape(T * E, 1),
                                             ro.actions.reshape(T * E, 2))
    ro.value_preds[:T].copy_((val + 0.15 * torch.randn(T * E, 1, generator=g)).view(T, E, 1))
    ro.action_log_probs.copy_((lp + 0.2 * torch.randn(T * E, 1, generator=g)).view(T, E, 1))
    return ro, torch.randn(E, 1, generator=g)


def _pair(dims, T, N, E, H, D, seed):
    """(CPU policy, CPU storage, their GPU copies, env_idx [N], det [T + 1, E]); the minibatch holds the all-ones env, and the all-zeros env when
    it has a second one; detected counts uniform in 1..H with 1 and H planted at its first two samples."""
    torch.manual_seed(seed)
    pol_c, ob_space, act_space = _policy(dims, T, E, H, D)
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(seed + 1))
    idx = perm[:N]
    env_ones, env_zeros = int(perm[0]), (int(perm[1]) if E > 1 else None)
    det = np.random.RandomState(seed + 2).randint(1, H + 1, size=(T + 1, E))
    for s, c in enumerate((1, H)[:T * N]):
        det[s // N, int(idx[s % N])] = c
    ro_c, next_value = _storage(pol_c, ob_space, act_space, T, E, H, D, det, env_ones, env_zeros, seed + 3)
    pol = copy.deepcopy(pol_c).cuda()
    ro = copy.deepcopy(ro_c)
    ro.to(torch.device("cuda"))
    ro.compute_returns(next_value.cuda(), True, 0.99, 0.95, False)
    ro_c.compute_returns(next_value, True, 0.99, 0.95, False)
    return pol_c, ro_c, pol, ro, idx, det


def _bound(pol):
    from crowdnav_prediction_attngraph_amd.ppo import PPO
    agent = PPO(pol, 0.2, 2, 1, 0.5, 0.0, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
    agent._bind_flat()
    return agent


@pytest.mark.parametrize("case", list(CASES))
def test_sized_minibatch_step_matches_the_fp64_cpu_graph(case):
    """See the module docstring; the case table is CASES."""
    from crowdnav_prediction_attngraph_amd import hip
    from tests.test_gpu_minibatch_step import _cpu_grads_in_chunks
    dims, T, N, E, H, D, edge = CASES[case]
    pol_c, ro_c, pol, ro, idx, det = _pair(dims, T, N, E, H, D, _seed(case))
    agent = _bound(pol)
    assert hip.SizedMinibatchStepper.supported(pol, ro) and not hip.MinibatchStepper.supported(pol, ro)
    assert N < E or case == "corner"
    adv = agent._advantages(ro)
    stepper = hip.SizedMinibatchStepper(pol)
    assert stepper.dims.astuple() == dims
    rows = int(stepper.row_totals(ro)[idx].sum())
    live = det[:T][:, idx.numpy()]
    assert rows == int(live.sum())
    if case == "o_only":
        assert rows == T * N
    ro_masks = ro.masks[:T, idx.cuda()]
    assert bool((ro_masks[:, 0] == 1).all()) and bool((ro_masks[:, 1] == 0).all())
    losses = torch.zeros(3, device="cuda")
    vlp = torch.empty(2, T * N, device="cuda")
    flat = agent._flat
    flat["g"].fill_(float("nan"))                                       # the call must WRITE every gradient
    stepper.step(ro, adv, idx.to("cuda", torch.int32), rows, HYPER, losses, vlp)
    torch.cuda.synchronize()
    g1, l1, vlp1 = flat["g"].clone(), losses.clone(), vlp.clone()
    flat["g"].fill_(float("nan"))
    stepper.step(ro, adv, idx.to("cuda", torch.int32), rows, HYPER, losses, vlp)     # deterministic: a second call gives identical bits
    torch.cuda.synchronize()
    assert torch.equal(l1, losses) and torch.equal(vlp1, vlp)
    off, got = 0, {}
    for name, p in pol.named_parameters():
        k = p.numel()
        got[name] = g1[off:off + k].view_as(p).cpu().double()
        if name.startswith("base.human_node_final_linear"):              # never reached by the loss: untouched, still the fill
            assert bool(torch.isnan(g1[off:off + k]).all()) and bool(torch.isnan(flat["g"][off:off + k]).all()), name
        else:
            assert bool(torch.isfinite(g1[off:off + k]).all()), name
            assert torch.equal(g1[off:off + k], flat["g"][off:off + k]), name
        off += (k + 3) // 4 * 4
    v_c, lp_c, sums_c, g_c = _cpu_grads_in_chunks(pol_c.double(), ro_c, adv.cpu(), idx, T, H, 0.2, 0.5, chunk=N)
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
    print("%s %s (T=%d N=%d E=%d H=%d D=%d, %d rows): values %.2e  log-probs %.2e  worst relative gradient error %.2e (%s)"
          % (case, dims, T, N, E, H, D, rows, ev, elp, table[0][0], table[0][1]))
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


def _raw_step(fn, stepper, ro, adv, idx, rows, dims, ws_ptr, ws_bytes, losses, vlp):
    """The C entry point `fn` called directly (no wrapper, no workspace cache): the status, and the library's message."""
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
        if fn == "cn_ppo_minibatch_step":
            rc = L.cn_ppo_minibatch_step(C.byref(b), rows, C.byref(w), C.byref(g), C.byref(hy), C.c_void_p(ws_ptr), ws_bytes, A.ptr(losses), A.ptr(vlp),
                                         A.stream_ptr())
        else:
            rc = L.cn_ppo_minibatch_step_sized(C.byref(b), rows, C.byref(w), C.byref(g), C.byref(hy), None if dims is None else C.byref(dims),
                                               C.c_void_p(ws_ptr), ws_bytes, A.ptr(losses), A.ptr(vlp), A.stream_ptr())
    return rc, L.cn_last_error().decode()


def test_the_step_stays_inside_the_workspace_the_sized_query_reports():
    """The call of case "ragged" through the C entry point with a workspace of exactly cn_ppo_minibatch_workspace_bytes_sized bytes, NaN-filled,
    and a NaN guard tail behind it: the tail is untouched, the results are those of the wrapper, and one byte less is CN_ERR_INVALID."""
    from crowdnav_prediction_attngraph_amd import hip
    dims, T, N, E, H, D, _ = CASES["ragged"]
    _, _, pol, ro, idx, _ = _pair(dims, T, N, E, H, D, _seed("ragged"))
    agent = _bound(pol)
    adv = agent._advantages(ro)
    stepper = hip.SizedMinibatchStepper(pol)
    rows = int(stepper.row_totals(ro)[idx].sum())
    idx_d = idx.to("cuda", torch.int32)
    d = A.PolicyDims(*dims)
    need = int(A.lib().cn_ppo_minibatch_workspace_bytes_sized(T, N, H, D, rows, C.byref(d)))
    assert need > 0 and need % 256 == 0
    guard = 4096
    buf = torch.full((need // 4 + guard,), float("nan"), device="cuda")
    assert buf.data_ptr() % 256 == 0
    losses, vlp = torch.zeros(3, device="cuda"), torch.empty(2, T * N, device="cuda")
    flat = agent._flat
    flat["g"].fill_(float("nan"))
    rc, msg = _raw_step("sized", stepper, ro, adv, idx_d, rows, d, buf.data_ptr(), need, losses, vlp)
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
    rc, msg = _raw_step("sized", stepper, ro, adv, idx_d, rows, d, buf.data_ptr(), need - 1, losses, vlp)
    torch.cuda.synchronize()
    assert rc == -1 and "workspace of" in msg, (rc, msg)                 # CN_ERR_INVALID
    assert bool(torch.isnan(flat["g"]).all()) and bool(torch.isnan(losses).all())


def test_the_default_tuple_changes_no_bit():
    """cn_ppo_minibatch_step, cn_ppo_minibatch_step_sized with the default tuple and with dims = NULL on one minibatch (T = 4, N = 9, E = 12, H = 20,
    D = 2), NaN-filled buckets: bucket, losses and values / log-probs are equal bit for bit, and so is the workspace size."""
    from crowdnav_prediction_attngraph_amd import hip
    T, N, E, H, D = 4, 9, 12, 20, 2
    _, _, pol, ro, idx, _ = _pair(A.DEFAULT_DIMS, T, N, E, H, D, seed=2024)
    agent = _bound(pol)
    assert hip.MinibatchStepper.supported(pol, ro) and hip.SizedMinibatchStepper.supported(pol, ro)
    adv = agent._advantages(ro)
    stepper = hip.MinibatchStepper(pol)
    rows = int(stepper.row_totals(ro)[idx].sum())
    idx_d = idx.to("cuda", torch.int32)
    L = A.lib()
    d = A.PolicyDims(*A.DEFAULT_DIMS)
    need = int(L.cn_ppo_minibatch_workspace_bytes(T, N, H, D, rows))
    assert need == L.cn_ppo_minibatch_workspace_bytes_sized(T, N, H, D, rows, C.byref(d)) == L.cn_ppo_minibatch_workspace_bytes_sized(T, N, H, D, rows, None)
    flat = agent._flat
    res = []
    for fn, dims in (("cn_ppo_minibatch_step", None), ("sized", d), ("sized", None)):
        buf = torch.full((need // 4,), float("nan"), device="cuda")
        losses, vlp = torch.full((3,), float("nan"), device="cuda"), torch.full((2, T * N), float("nan"), device="cuda")
        flat["g"].fill_(float("nan"))
        rc, msg = _raw_step(fn, stepper, ro, adv, idx_d, rows, dims, buf.data_ptr(), need, losses, vlp)
        torch.cuda.synchronize()
        assert rc == 0, msg
        res.append((torch.nan_to_num(flat["g"], nan=7.0).clone(), losses.clone(), vlp.clone()))
        assert int(torch.isnan(flat["g"]).sum()) < 600                   # only human_node_final_linear (514) and the bucket's padding keep the fill
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.equal(a, b)
    assert bool(torch.isfinite(res[0][1]).all()) and bool(torch.isfinite(res[0][2]).all())


@pytest.mark.parametrize("bad", [(96, 64, 64, 256), (128, 32, 64, 256), (128, 64, 64, 96), (128, 64, 0, 256), (128, 64, 257, 256), (128, 64, 64, 576)])
def test_a_tuple_outside_the_box_is_refused_before_any_launch(bad):
    from crowdnav_prediction_attngraph_amd import hip
    T, N, E, H, D = 2, 3, 4, 5, 2
    _, _, pol, ro, idx, _ = _pair(A.DEFAULT_DIMS, T, N, E, H, D, seed=7)
    agent = _bound(pol)
    adv = agent._advantages(ro)
    stepper = hip.MinibatchStepper(pol)
    rows = int(stepper.row_totals(ro)[idx].sum())
    d = A.PolicyDims(*bad)
    assert A.lib().cn_ppo_minibatch_workspace_bytes_sized(T, N, H, D, rows, C.byref(d)) == 0
    buf = torch.full((1 << 22,), float("nan"), device="cuda")            # 16 MB: more than any tuple of the box needs at this shape
    losses = torch.full((3,), float("nan"), device="cuda")
    flat = agent._flat
    flat["g"].fill_(float("nan"))
    rc, msg = _raw_step("sized", stepper, ro, adv, idx.to("cuda", torch.int32), rows, d, buf.data_ptr(), buf.numel() * 4, losses, None)
    torch.cuda.synchronize()
    assert rc == -1, (rc, msg)                                           # CN_ERR_INVALID
    assert "outside the device box" in msg and "rnn_size in {64, 128, 192, 256}" in msg and "attention_size in [1, 256]" in msg, msg
    assert bool(torch.isnan(flat["g"]).all()) and bool(torch.isnan(losses).all()) and bool(torch.isnan(buf).all())


# ---- PPO.update through the step ---------------------------------------------------------------------------------------------------------

def _count_steps(monkeypatch):
    from crowdnav_prediction_attngraph_amd import hip
    calls = []
    real = hip.SizedMinibatchStepper.step

    def counted(self, *a, **k):
        calls.append(type(self).__name__)
        return real(self, *a, **k)
    monkeypatch.setattr(hip.SizedMinibatchStepper, "step", counted)
    return calls


def _update_pair(T, E, H, nmb, seed):
    torch.manual_seed(seed)
    pol_c, ob_space, act_space = _policy(RAGGED, T, E, H, 2)
    det = np.random.RandomState(seed + 2).randint(1, H + 1, size=(T + 1, E))
    ro_c, next_value = _storage(pol_c, ob_space, act_space, T, E, H, 2, det, 0, 1, seed + 3)
    pol = copy.deepcopy(pol_c).cuda()
    ro_c.to(torch.device("cuda"))
    ro_c.compute_returns(next_value.cuda(), True, 0.99, 0.95, False)
    return pol, ro_c


def test_update_routes_a_sized_policy_through_the_sized_step(monkeypatch):
    """(192, 64, 48, 320) on the GPU: PPO._fast_path is true although MinibatchStepper.supported (default sizes) stays false; one update() calls
    SizedMinibatchStepper.step ppo_epoch * num_mini_batch times; with use_minibatch_step = False it is never called."""
    from crowdnav_prediction_attngraph_amd import hip
    from crowdnav_prediction_attngraph_amd.ppo import PPO
    pol, ro = _update_pair(4, 8, 5, 2, seed=91)
    calls = _count_steps(monkeypatch)
    agent = PPO(pol, 0.2, 3, 2, 0.5, 0.01, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
    assert agent._fast_path(ro)
    assert not hip.MinibatchStepper.supported(pol, ro) and hip.SizedMinibatchStepper.supported(pol, ro)
    res = agent.update(ro)
    assert np.isfinite(res).all()
    assert calls == ["SizedMinibatchStepper"] * 6 and type(agent._stepper) is hip.SizedMinibatchStepper
    del calls[:]
    agent.use_minibatch_step = False
    assert not agent._fast_path(ro)
    agent.update(ro)
    assert calls == []


def test_update_through_the_sized_step_matches_the_autograd_joined_producer():
    """One PPO.update at (192, 64, 48, 320), T = 30, 64 envs of 20 humans, 2 epochs x 2 minibatches, with the step on and off from equal weights
    and storage: the bars tests/test_gpu_minibatch_step.py::test_ppo_update_through_the_minibatch_step_matches_the_cpu_update holds between
    the two GPU producers at the default sizes (losses rtol 1e-5 / atol 1e-6; every tensor max 1.6e-5, mean 1e-7)."""
    from crowdnav_prediction_attngraph_amd.ppo import PPO
    pol_a, ro = _update_pair(30, 64, 20, 2, seed=41)
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


def test_reference_golden_update_goes_through_the_sized_step(monkeypatch):
    """The reference's PPO.update at (192, 64, 48, 320) (tests/golden/rollsize_r192_m64_a48_o320_e4_h8_t5.npz) replayed on the GPU at
    atol 2e-6 / rtol 1e-5, every optimiser step of it through SizedMinibatchStepper.step."""
    from tests.test_policy_sizes import ROLL, filled_rollouts, update_policy
    from tests.test_policy_variants import check_update_against_the_reference
    path = [p for p in ROLL if p.endswith("rollsize_r192_m64_a48_o320_e4_h8_t5.npz")][0]
    z = np.load(path)
    meta = json.loads(str(z["meta"]))
    assert tuple(meta["dims"]) == RAGGED
    pol = update_policy(meta).cuda()
    ro = filled_rollouts(z, meta, pol, "cuda")
    calls = _count_steps(monkeypatch)
    check_update_against_the_reference(z, meta, pol, ro, atol=2e-6, rtol=1e-5)
    assert len(calls) == meta["ppo_epoch"] * meta["nmb"] > 0
