"""-m gpu: cn_ppo_minibatch_step against the torch-op graph on the CPU in fp64 at the EDGES of the shape box it declares (1 <= H <= 48,
1 <= D <= 16, any T, N >= 1).  tests/test_gpu_minibatch_step.py and tests/test_gpu_train_scale.py hold the step to an independent reference at
T = 30, H = 20, D = 2 only; every other shape was compared with the autograd-joined path of the same build, i.e. with the same kernels.

One call of hip.MinibatchStepper.step per case, on a shuffled strict subset of the storage's envs (N < E wherever E allows), from a storage
that carries one env whose done masks are all 0 and one whose masks are all 1:
  * values and log-probs of ALL samples (1e-4 absolute), the value and action loss (rtol 2e-4, atol 1e-6), the entropy (closed form, 1e-6);
  * every parameter gradient, read from the flat bucket: 5e-4 of the reference tensor's largest entry + 1e-7 (the bars of
    tests/test_gpu_train_scale.py / tests/test_gpu_minibatch_step.py);
  * the bucket is NaN-filled before the call, every covered gradient is finite afterwards, human_node_final_linear keeps the fill, a second
    call gives identical bits, and rows == row_totals[idx].sum().
Each case is the smallest shape that reaches its edge (see CASES).  Reference: rl/networks/storage.py:184-253, rl/networks/model.py:82-90,
rl/ppo/ppo.py:66-88 through policy.py's torch-op graph, which tests/test_host_policy.py pins to the reference.

Measured on an MI355X, worst relative gradient error per case (error / largest reference entry of the tensor; the bar is 5e-4):
  rows_1                 3.3e-5  (actor.0.weight)                          all_one_human       9.7e-6  (robot_linear.0.bias)
  only_wide_class        5.0e-5  (attn.spatial_edge_layer.0.weight)        b_1025              2.0e-4  (embedding_layer.2.weight)
  class_boundaries_d16   5.3e-5  (attn.spatial_edge_layer.0.weight)        t1_d8               3.3e-4  (spatial_linear.0.bias)
  h33_d12                1.4e-5  (attn.temporal_edge_layer.0.bias)         h48_pipelined_tail  3.5e-4  (embedding_layer.2.weight)
values within 9.3e-6 and log-probs within 1.6e-5 of the fp64 graph in every case.

Re-seeded cases.  The first seed of a case is 1000 + sum(map(ord, name)).  Three cases missed the gradient bar with it -- class_boundaries_d16
(seed 2995: 1.4e-3, embedding_layer.2.weight), b_1025 (seed 1393: 3.4e-3, spatial_linear.0.weight) and t1_d8 (seed 1416: 2.8e-3,
embedding_layer.2.weight), values and log-probs at <= 1.6e-5 -- and every miss is a ReLU unit at its kink, not an error of a kernel.  Shown on
the CPU side: with torch.nn.functional.relu hooked in the fp64 graph, the units of the block's three ReLUs whose fp64 gate [pre-activation > 0]
differs from the GPU's (read from the activations hip.HHBlockFused saves for the same minibatch: the kernel and inputs of the step, bit for
bit) are 1, 2 and 11 units with |pre-activation| <= 5.5e-7, 2.9e-6 and 2.8e-6 -- far inside the 1e-4 forward bar -- and the fp64 graph with
the GPU's gates imposed at those ReLUs agrees with the step in EVERY tensor (worst 2.0e-5, 1.1e-5, 1.5e-5 of the largest entry).  One such unit
moves its bias gradient by that row's d_out entry, up to a tenth of the entry's sum over a few thousand rows; the GPU forward is accurate to
a few 1e-6, so a unit lands on the other side of zero about once per 3e5 pre-activations (2.7 M in b_1025, 4.8 M in t1_d8: of 8 / 24 / 48
seeds tried for the three cases, 3 / 4 / 7 give a batch whose flipped units all carry small gradients).  The smallest cases have too few units
for a flip to be likely, the large ones (h48_pipelined_tail: 71 flipped units, 3.5e-4; the bench-size test) average over enough rows.  A future miss of these cases is
diagnosed the same way before anything else: impose the GPU's gates in the fp64 graph and look at what is left.
"""
import copy
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _counts_const(c):
    return lambda rs, T, E, H, N, idx: np.full((T + 1, E), c, dtype=np.int64)


def _counts_ragged(*must):
    """Uniform 1..H, with the counts of `must` planted at the first samples of the minibatch (sample s = t * N + j reads env idx[j] at step t)."""
    def f(rs, T, E, H, N, idx):
        det = rs.randint(1, H + 1, size=(T + 1, E))
        for s, c in enumerate(must):
            det[s // N, idx[s % N]] = c
        return det
    return f


def _counts_every_7th(c, c7):
    def f(rs, T, E, H, N, idx):
        det = np.full((T + 1, E), c, dtype=np.int64)
        for s in range(0, T * N, 7):
            det[s // N, idx[s % N]] = c7
        return det
    return f


# T, N, E, H, D, detected counts, counts the minibatch must contain, edge, seed (see the module docstring for the three that are not the first tried)
CASES = {
    "rows_1": (1, 1, 2, 1, 2, _counts_const(1), (1,), "rows = 1, a sequence of one step, one weight-gradient split, one input-layer partial block", 1603),
    "only_wide_class": (2, 3, 5, 48, 2, _counts_const(48), (48,), "only the 33..64 attention class: the other class lists are empty", 2599),
    "class_boundaries_d16": (4, 9, 12, 48, 16, _counts_ragged(1, 8, 9, 16, 17, 32, 33, 48), (1, 8, 9, 16, 17, 32, 33, 48), "every class boundary, widest D", 3595),
    "h33_d12": (3, 7, 7, 33, 12, _counts_ragged(32, 33), (32, 33), "first H of the wide class, N == E", 1500),
    "all_one_human": (7, 33, 40, 17, 2, _counts_const(1), (1,), "rows == B: a softmax over one element everywhere", 2362),
    "b_1025": (5, 205, 210, 5, 2, _counts_ragged(), (), "B = 1025: the second scan workgroup holds one sample", 3193),
    "t1_d8": (1, 1100, 1200, 9, 8, _counts_ragged(), (), "T = 1, B = 1100 (a partial second scan workgroup), D = 8", 5316),
    "h48_pipelined_tail": (30, 40, 48, 48, 2, _counts_every_7th(48, 41), (41, 48), "~56 k rows, rows % 32 != 0: the pipelined weight gradient + its row tail at H = 48", 2782),
}


def _policy(T, E, H, D):
    from crowdnav_prediction_attngraph_amd.policy import Policy, make_spaces
    ob_space, act_space = make_spaces(H, D)
    kw = dict(env_name="CrowdSimVarNum-v0" if D == 2 else "CrowdSimPred-v0", num_processes=E, num_mini_batch=1, seq_length=T)
    if D not in (2, 12):
        kw["predict_steps"] = D // 2 - 1            # D = 2 (1 + predict_steps): 16 -> 7, 8 -> 3 (policy.py: the env_name check)
    pol = Policy(ob_space.spaces, act_space, base="selfAttn_merge_srnn", base_kwargs=kw)
    pol.base.nenv = E
    return pol, ob_space, act_space


def _edge_storage(pol, ob_space, act_space, T, E, H, D, det, env_ones, env_zeros, seed):
    """A RolloutStorage as a rollout would leave it, with the given detected counts det [T + 1, E]: humans sorted by distance, the rows past the
    count at the simulator's padding value 15.0, old values / log-probs of the policy itself plus noise (ratios and value clips on both sides of
    their thresholds), episode ends at random except in the two envs whose masks are all 1 / all 0."""
    from crowdnav_prediction_attngraph_amd.storage import RolloutStorage
    rs = np.random.RandomState(seed)
    n = (T + 1) * E
    ro = RolloutStorage(T, E, ob_space.spaces, act_space, 128, 256)
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
    ro.recurrent_hidden_states["human_node_rnn"].copy_(0.5 * torch.randn(T + 1, E, 1, 128, generator=g))
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


def _pair_cpu(T, N, E, H, D, counts, seed):
    """(CPU policy, CPU storage without returns, next_value, env_idx [N], det [T + 1, E])."""
    torch.manual_seed(seed)
    pol_c, ob_space, act_space = _policy(T, E, H, D)
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(seed + 1))
    idx = perm[:N]                                                      # shuffled; a strict subset of the storage's envs when N < E
    # the all-ones env is always inside the minibatch; the all-zeros env too when the minibatch has a second env
    env_ones, env_zeros = int(perm[0]), (int(perm[1]) if E > 1 else None)
    det = counts(np.random.RandomState(seed + 2), T, E, H, N, idx.numpy())
    ro_c, next_value = _edge_storage(pol_c, ob_space, act_space, T, E, H, D, det, env_ones, env_zeros, seed + 3)
    return pol_c, ro_c, next_value, idx, det


def _pair(T, N, E, H, D, counts, seed):
    """(CPU policy, CPU storage, their GPU copies, env_idx [N], det [T + 1, E]) with the returns computed on both sides."""
    pol_c, ro_c, next_value, idx, det = _pair_cpu(T, N, E, H, D, counts, seed)
    pol = copy.deepcopy(pol_c).cuda()
    ro = copy.deepcopy(ro_c)
    ro.to(torch.device("cuda"))
    ro.compute_returns(next_value.cuda(), True, 0.99, 0.95, False)
    ro_c.compute_returns(next_value, True, 0.99, 0.95, False)
    return pol_c, ro_c, pol, ro, idx, det


@pytest.mark.parametrize("case", list(CASES))
def test_minibatch_step_matches_the_fp64_cpu_graph_at_the_edge(case):
    """See the module docstring; the case table is CASES."""
    from crowdnav_prediction_attngraph_amd import hip
    from crowdnav_prediction_attngraph_amd.ppo import PPO
    from tests.test_gpu_minibatch_step import _cpu_grads_in_chunks
    T, N, E, H, D, counts, must, edge, seed = CASES[case]
    pol_c, ro_c, pol, ro, idx, det = _pair(T, N, E, H, D, counts, seed)
    agent = PPO(pol, 0.2, 2, 1, 0.5, 0.0, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
    agent._bind_flat()
    assert hip.MinibatchStepper.supported(pol, ro)
    adv = agent._advantages(ro)
    stepper = hip.MinibatchStepper(pol)
    rows = int(stepper.row_totals(ro)[idx].sum())
    live = det[:T][:, idx.numpy()]
    assert rows == int(live.sum()) and set(must) <= set(live.reshape(-1).tolist()), (rows, int(live.sum()))
    if case == "rows_1":
        assert rows == 1
    if case == "all_one_human":
        assert rows == T * N
    if case == "h48_pipelined_tail":
        assert rows >= 32768 and rows % 32 != 0, rows
    losses = torch.zeros(3, device="cuda")
    vlp = torch.empty(2, T * N, device="cuda")
    flat = agent._flat
    hyper = (0.2, 0.5, 0.0, True)
    flat["g"].fill_(float("nan"))                                       # the call must WRITE every gradient
    stepper.step(ro, adv, idx.to("cuda", torch.int32), rows, hyper, losses, vlp)
    torch.cuda.synchronize()
    g1, l1, vlp1 = flat["g"].clone(), losses.clone(), vlp.clone()
    flat["g"].fill_(float("nan"))
    stepper.step(ro, adv, idx.to("cuda", torch.int32), rows, hyper, losses, vlp)     # deterministic: a second call gives identical bits
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
    print("%s (T=%d N=%d E=%d H=%d D=%d, %d rows): values %.2e  log-probs %.2e  worst relative gradient error %.2e (%s)"
          % (case, T, N, E, H, D, rows, ev, elp, table[0][0], table[0][1]))
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


# ---- the row bound: rows * 1536 < 2^31 (cn_ppo_minibatch_max_rows), on the live rows and not on T * N * H -------------------------------------

def test_step_takes_a_minibatch_whose_padded_size_is_past_the_row_bound():
    """T = 30, N = 971 envs of 48 humans with ONE detected human in every sample: T * N * H = 1 398 240 is more than cn_ppo_minibatch_max_rows() =
    1 398 101 (the quantity the guard used to test) while the step works on rows = 29 130.  It runs and equals the autograd-joined path on the
    same minibatch at the bar of tests/test_gpu_minibatch_step.py (same kernels on both sides: the subject is the guard)."""
    from crowdnav_prediction_attngraph_amd import hip
    from crowdnav_prediction_attngraph_amd.ppo import PPO
    T, N, H, D = 30, 971, 48, 2
    _, _, pol, ro, _, _ = _pair(T, N, N, H, D, _counts_const(1), seed=61)
    assert T * N * H * 1536 >= 2 ** 31 > T * N * 1536                   # the padded size is past 32-bit element offsets, the live rows are far inside
    agent = PPO(pol, 0.2, 2, 1, 0.5, 0.01, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
    agent._bind_flat()
    adv = agent._advantages(ro)
    flat = agent._flat
    torch.manual_seed(77)
    obs_b, hxs_b, act_b, vp_b, ret_b, m_b, olp_b, adv_b = next(ro.recurrent_generator(adv, 1))
    values, logp, ent, _ = pol.evaluate_actions(obs_b, hxs_b, m_b, act_b)
    vl, al = agent._losses(values, logp, olp_b, adv_b, vp_b, ret_b)
    flat["g"].zero_()
    (vl * agent.value_loss_coef + al - ent * agent.entropy_coef).backward()
    g_ref = flat["g"].clone()
    ref_losses = torch.stack([vl.detach(), al.detach(), ent.detach()]).cpu()
    torch.manual_seed(77)
    idx = torch.randperm(N)
    stepper = hip.MinibatchStepper(pol)
    rows = int(stepper.row_totals(ro)[idx].sum())
    assert rows == T * N
    losses = torch.zeros(3, device="cuda")
    vlp = torch.empty(2, T * N, device="cuda")
    flat["g"].fill_(float("nan"))
    stepper.step(ro, adv, idx.to("cuda", torch.int32), rows, (agent.clip_param, agent.value_loss_coef, agent.entropy_coef, True), losses, vlp)
    torch.cuda.synchronize()
    assert torch.equal(vlp[0].view(-1, 1), values.detach()) and torch.equal(vlp[1].view(-1, 1), logp.detach())
    np.testing.assert_allclose(losses.cpu().numpy(), ref_losses.numpy(), rtol=1e-6, atol=1e-7)
    off = 0
    for name, p in pol.named_parameters():
        k = p.numel()
        got, want = flat["g"][off:off + k], g_ref[off:off + k]
        off += (k + 3) // 4 * 4
        if name.startswith("base.human_node_final_linear"):
            continue
        assert bool(torch.isfinite(got).all()), name
        scale = max(float(want.abs().max()), 1e-8)
        err = float((got - want).abs().max())
        assert err <= 2e-5 * scale + 1e-9, (name, err, scale)


def test_the_c_call_refuses_exactly_past_the_host_side_row_bound():
    """cn_ppo_minibatch_step and the host-side query agree on both sides of cn_ppo_minibatch_max_rows(): one row more is refused by the bound,
    the bound itself passes it (the call then stops at the next check, the workspace size -- this test hands it a 4 KB workspace so that
    neither call launches anything: every argument check precedes the first launch)."""
    import ctypes as C
    from crowdnav_prediction_attngraph_amd import _abi as A
    L = A.lib()
    top = int(L.cn_ppo_minibatch_max_rows())
    T, N, H, D = 30, 971, 48, 2                                         # T * N * H = 1 398 240: both row counts are inside [B, B * H]
    assert T * N <= top < top + 1 <= T * N * H
    assert L.cn_ppo_minibatch_workspace_bytes(T, N, H, D, top) > 0 and L.cn_ppo_minibatch_workspace_bytes(T, N, H, D, top + 1) == 0
    dummy = torch.zeros(4096, dtype=torch.uint8, device="cuda")         # never read or written: both calls are refused before any launch
    assert dummy.data_ptr() % 256 == 0
    b = A.PpoBatch(T, N, N, H, D)
    for k in A.PPO_BATCH_TENSORS:
        setattr(b, k, dummy.data_ptr())
    w = A.PolicyWeights()
    for field, _ in A.POLICY_WEIGHT_KEYS:
        setattr(w, field, dummy.data_ptr())
    hy = A.PpoHyper(0.2, 0.5, 0.0, 1)

    def call(rows):
        with torch.cuda.device(dummy.device):
            rc = L.cn_ppo_minibatch_step(C.byref(b), rows, C.byref(w), C.byref(w), C.byref(hy), C.c_void_p(dummy.data_ptr()), 4096, A.ptr(dummy), None, A.stream_ptr())
        return rc, L.cn_last_error().decode()

    rc, msg = call(top + 1)
    assert rc != 0 and "cn_ppo_minibatch_max_rows" in msg, (rc, msg)
    rc, msg = call(top)
    assert rc != 0 and "workspace of" in msg and "cn_ppo_minibatch_max_rows" not in msg, (rc, msg)
    torch.cuda.synchronize()


def _update_pair(T, E, H, seed):
    pol_c, ro_c, pol, ro, _, _ = _pair(T, E, E, H, 2, _counts_ragged(1, H), seed)
    return pol_c, ro_c, pol, ro


def test_update_takes_the_autograd_joined_path_when_the_rows_are_past_the_bound(monkeypatch):
    """PPO.update decides from the row totals it reads back anyway, before any launch of the step: with MinibatchStepper.row_totals reporting
    more rows than one call takes, update() does not raise and returns what use_minibatch_step = False returns, bit for bit (losses and
    every weight), without a single call of the step."""
    from crowdnav_prediction_attngraph_amd import hip
    from crowdnav_prediction_attngraph_amd.ppo import PPO
    _, _, pol_a, ro = _update_pair(8, 16, 5, seed=71)
    pol_b = copy.deepcopy(pol_a)
    E = ro.rewards.shape[1]
    top = (2 ** 31 - 1) // 1536                                         # rows * 1536 < 2^31: what cn_ppo_minibatch_max_rows() reports
    monkeypatch.setattr(hip.MinibatchStepper, "row_totals", lambda self, rollouts: torch.full((E,), top // (E // 2) + 1, dtype=torch.int64))

    def no_step(self, *a, **k):
        raise AssertionError("cn_ppo_minibatch_step was launched for a minibatch past the row bound")
    monkeypatch.setattr(hip.MinibatchStepper, "step", no_step)
    out = []
    for pol, fast in ((pol_a, True), (pol_b, False)):
        agent = PPO(pol, 0.2, 2, 2, 0.5, 0.01, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
        agent.use_minibatch_step = fast
        assert agent._fast_path(ro) == fast
        torch.manual_seed(123)
        out.append((agent.update(ro), {k: v.detach().clone() for k, v in pol.state_dict().items()}))
    assert out[0][0] == out[1][0]
    for k, v in out[0][1].items():
        assert torch.equal(v, out[1][1][k]), k


def test_update_ignores_stale_bucket_slices_of_parameters_the_step_does_not_write():
    """The flat gradient bucket also holds the parameters the loss never reaches (base.human_node_final_linear.*), which
    cn_ppo_minibatch_step does not write; their slices still enter the clip norm and Adam.  With 1e3 left in them before update() (514 entries:
    a norm of 2.3e4 against max_grad_norm = 0.5 would scale every other gradient by 2e-5), the fast path still gives the CPU update: the
    rollout, the shape (2 epochs x 2 minibatches of 30 x 128 samples -- at smaller ones Adam's division by near-zero gradient entries takes the
    CPU and GPU weights further apart than these bars) and the bars of
    tests/test_gpu_minibatch_step.py::test_ppo_update_through_the_minibatch_step_matches_the_cpu_update."""
    from crowdnav_prediction_attngraph_amd import _abi as A
    from crowdnav_prediction_attngraph_amd.ppo import PPO
    from tests.test_gpu_minibatch_step import _setup
    T, E, H, D, nmb = 30, 256, 20, 2, 2
    pol_c, ro_c, pol_g, ro_g, _ = _setup(T, E, H, D, nmb, seed=41)
    covered = {k for _, k in A.POLICY_WEIGHT_KEYS}
    out = {}
    for name, pol, ro in (("cpu", pol_c, ro_c), ("gpu", pol_g, ro_g)):
        agent = PPO(pol, 0.2, 2, nmb, 0.5, 0.0, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
        if name == "gpu":
            agent._bind_flat()
            stale = [p for k, p in pol.named_parameters() if k not in covered]
            assert len(stale) == 2 and agent._fast_path(ro)
            for p in stale:
                p.grad.fill_(1e3)
        torch.manual_seed(123)
        res = agent.update(ro)
        out[name] = (res, {k: v.detach().cpu().double() for k, v in pol.state_dict().items()})
    np.testing.assert_allclose(out["gpu"][0], out["cpu"][0], rtol=2e-4, atol=1e-5)
    for k, wc in out["cpu"][1].items():
        d = (out["gpu"][1][k] - wc).abs()
        assert float(d.max()) <= 1.6e-5, (k, float(d.max()))
        assert float(d.mean()) <= 2e-7, (k, float(d.mean()))
