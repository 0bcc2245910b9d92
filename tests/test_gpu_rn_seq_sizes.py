"""-m gpu: the robot-node sequence of the training path at off-default network sizes -- cn_rn_seq_fwd_sized / cn_rn_seq_bwd_sized called directly
on synthetic inputs with the formula weights of tests/policy_util.py, against the fp64 graph of tests/rn_seq_util.py (tied to Policy(...).double()
in tests/test_rn_seq_sizes.py, which also shows the fp32 mirror within a quarter of every bar here); the sized GRU pair alone; and
Policy.evaluate_actions reaching the sized sequence.

Bars (set before the kernels ran): value, logp, h_T 1e-4 absolute (the project bar); every gradient 3e-4 of the tensor's largest fp64 entry +
1e-7 (tests/test_gpu_policy_sizes.py:279-282).  Every output, saved and workspace buffer is NaN-filled with a NaN guard tail behind it: a padded
product that writes past a row's real columns lands in a neighbour's NaN-checked row or in a tail."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from crowdnav_prediction_attngraph_amd import _abi as A  # noqa: E402
from tests import rn_seq_util as U  # noqa: E402

GUARD = 96


def guarded(shape, dev="cuda"):
    """NaN-filled tensor of `shape` with GUARD floats of NaN behind it: (view, whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), float("nan"), device=dev)
    return buf[:n].view(*shape), buf


def run_device(dims, T, N, H, ws, inp, sized=True):
    """One forward and one backward through the C entry points into NaN-filled, guarded buffers.  Returns (results as float64 numpy, saved
    buffers as tensors); asserts the guards and that nothing readable was left unwritten."""
    R, M, _, O = dims
    B = T * N
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()   # noqa: E731
    rows, row_off = U.compact(inp)
    rn, te, osp, h0, m, act = f(inp["robot_node"]), f(inp["temporal"]), f(rows), f(inp["h0"]), f(inp["masks"]), f(inp["actions"])
    dv, dl = f(inp["d_value"]), f(inp["d_logp"])
    ro = torch.from_numpy(row_off).cuda()
    wd = [w.detach().float().cuda().contiguous() for w in ws]
    d = A.PolicyDims(*dims)
    L = A.lib()
    widths = A.rn_saved_widths(dims, H)
    bufs = {k: guarded((B, widths[k])) for k in A.RN_SAVED_FIELDS}
    bufs.update(value=guarded((B,)), logp=guarded((B,)), d_out_sp=guarded(tuple(osp.shape)), d_h0=guarded((N, R)))
    for name, w in zip(A.RN_WEIGHT_FIELDS, wd):
        bufs["g_" + name] = guarded(tuple(w.shape))
    fws = int(L.cn_rn_seq_fwd_workspace_floats_sized(C.byref(d)) if sized else L.cn_rn_seq_fwd_workspace_floats())
    bws = int(L.cn_rn_seq_workspace_floats_sized(T, N, C.byref(d)) if sized else L.cn_rn_seq_workspace_floats(T, N))
    bufs["fwd_ws"], bufs["bwd_ws"] = guarded((fws,)), guarded((bws,))
    v = {k: b[0] for k, b in bufs.items()}
    wst = A.RnWeights(*[w.data_ptr() for w in wd])
    sst = A.RnSaved(*[v[k].data_ptr() for k in A.RN_SAVED_FIELDS])
    gst = A.RnWeights(*[v["g_" + n].data_ptr() for n in A.RN_WEIGHT_FIELDS])
    tail = (C.byref(d), A.stream_ptr()) if sized else (A.stream_ptr(),)
    sfx = "_sized" if sized else ""
    A.call("cn_rn_seq_fwd" + sfx, T, N, H, A.ptr(rn), A.ptr(te), A.ptr(osp), A.ptr(ro), A.ptr(h0), A.ptr(m), A.ptr(act), C.byref(wst), C.byref(sst),
           A.ptr(v["fwd_ws"]), A.ptr(v["value"]), A.ptr(v["logp"]), *tail)
    A.call("cn_rn_seq_bwd" + sfx, T, N, H, A.ptr(rn), A.ptr(te), A.ptr(osp), A.ptr(ro), A.ptr(m), A.ptr(act), C.byref(wst), C.byref(sst), A.ptr(dv), A.ptr(dl),
           A.ptr(v["bwd_ws"]), A.ptr(v["d_out_sp"]), A.ptr(v["d_h0"]), C.byref(gst), *tail)
    torch.cuda.synchronize()
    for k, (view, whole) in bufs.items():
        assert torch.isnan(whole[view.numel():]).all(), "guard tail behind %s was written" % k
        if not k.endswith("_ws"):
            assert not torch.isnan(view).any(), "%s has entries the call did not write" % k
    res = {k: t.detach().double().cpu().numpy() for k, t in v.items() if not k.endswith("_ws")}
    res["h_T"] = res["hs"][(T - 1) * N:]
    dense = np.zeros((B, H, 256))
    dense[inp["valid"]] = res["d_out_sp"]
    res["d_out_sp_dense"] = dense
    return res, {k: v[k].clone() for k in v if not k.endswith("_ws")}


@pytest.fixture(scope="module")
def references():
    """fp64 graph per case, computed once and shared (read only)."""
    out = {}
    for dims, (T, N, H) in U.CASES:
        ws = U.folded_weights(U.sized_policy(dims, H).double())
        inp = U.make_inputs(dims, T, N, H)
        out[(dims, (T, N, H))] = (ws, inp, U.run_graph(ws, inp, dims, T, N, H, torch.float64))
    return out


@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_sized_sequence_against_the_fp64_graph_with_guards_and_reruns(case, references):
    dims, (T, N, H) = case
    ws, inp, ref = references[case]
    got, raw = run_device(dims, T, N, H, ws, inp)
    rows = []
    for k in ("value", "logp", "h_T"):
        rows.append((k, float(np.abs(got[k] - ref[k]).max()), U.VALUE_BAR))
    rows.append(("d_out_sp", float(np.abs(got["d_out_sp_dense"] - ref["d_out_sp"]).max()), U.grad_bar(ref["d_out_sp"])))
    for k in ["d_h0"] + ["g_" + n for n in A.RN_WEIGHT_FIELDS]:
        rows.append((k, float(np.abs(got[k].reshape(ref[k].shape) - ref[k]).max()), U.grad_bar(ref[k])))
    for k, err, bar in rows:
        print("%s %-10s max |device - fp64| = %.3e  bar %.3e  (%.3f)" % (U.case_id(case), k, err, bar, err / bar))
    for k, err, bar in rows:
        assert err <= bar, (k, err, bar)
    # the same call again: identical bits, forward, saved and every gradient
    _, again = run_device(dims, T, N, H, ws, inp)
    for k, t in raw.items():
        assert torch.equal(t, again[k]), "%s differs between two calls on the same inputs" % k


def test_sized_entries_at_the_default_dims_give_the_unsized_bits():
    dims, (T, N, H) = A.DEFAULT_DIMS, (3, 33, 5)
    ws = U.folded_weights(U.sized_policy(dims, H).double())
    inp = U.make_inputs(dims, T, N, H)
    _, a = run_device(dims, T, N, H, ws, inp, sized=True)
    _, b = run_device(dims, T, N, H, ws, inp, sized=False)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("bad", [(96, 64, 64, 256), (128, 32, 64, 256), (128, 64, 64, 576), (128, 64, 0, 256)], ids=str)
def test_dims_outside_the_box_are_refused_before_anything_is_launched(bad):
    d = A.PolicyDims(*bad)
    L = A.lib()
    z = torch.zeros(4096, device="cuda")
    out = torch.full((4096,), float("nan"), device="cuda")
    wst = A.RnWeights(*[z.data_ptr()] * len(A.RN_WEIGHT_FIELDS))
    sst = A.RnSaved(*[out.data_ptr()] * len(A.RN_SAVED_FIELDS))
    ro = torch.zeros(2, dtype=torch.int32, device="cuda")
    rc = L.cn_rn_seq_fwd_sized(1, 1, 1, A.ptr(z), A.ptr(z), A.ptr(z), A.ptr(ro), A.ptr(z), A.ptr(z), A.ptr(z), C.byref(wst), C.byref(sst), A.ptr(out), A.ptr(out),
                               A.ptr(out), C.byref(d), A.stream_ptr())
    msg = L.cn_last_error().decode()
    assert rc == -1 and "device box" in msg and "rnn_size in {64, 128, 192, 256}" in msg, (rc, msg)
    rc = L.cn_rn_seq_bwd_sized(1, 1, 1, A.ptr(z), A.ptr(z), A.ptr(z), A.ptr(ro), A.ptr(z), A.ptr(z), C.byref(wst), C.byref(sst), A.ptr(z), A.ptr(z), A.ptr(out),
                               A.ptr(out), A.ptr(out), C.byref(wst), C.byref(d), A.stream_ptr())
    assert rc == -1 and "device box" in L.cn_last_error().decode()      # CN_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.isnan(out).all()      # nothing ran
    with pytest.raises(A.CnError):
        A.call("cn_rn_seq_fwd_sized", 1, 1, 1, A.ptr(z), A.ptr(z), A.ptr(z), A.ptr(ro), A.ptr(z), A.ptr(z), A.ptr(z), C.byref(wst), C.byref(sst), A.ptr(out),
               A.ptr(out), A.ptr(out), C.byref(d), A.stream_ptr())


GRU_CASES = [(R, 3, 17, False) for R in (64, 128, 192, 256)] + [(128, 1, 1, False), (192, 1, 1, False), (64, 3, 17, True)]


def gru_case_id(c):
    R, T, N, null_ws = c
    return str(R) + ("" if (T, N) == (3, 17) else "_T%d_N%d" % (T, N)) + ("_null_workspace" if null_ws else "")


@pytest.mark.parametrize("case", GRU_CASES, ids=gru_case_id)
def test_sized_gru_pair_against_the_fp64_loop(case):
    """cn_gru_seq_fwd_sized / cn_gru_seq_bwd_sized alone: T = 3 with interior done masks, N = 17 (two workgroups, the second with one row) at every R;
    one step of one row (no next step to publish or to request) on the resident and on the streamed form; and a resident R without a workspace."""
    R, T, N, null_ws = case
    rs = np.random.RandomState(R)
    gi = rs.uniform(-1, 1, (T, N, 3 * R))
    h0 = rs.uniform(-1, 1, (N, R))
    whh = rs.uniform(-1, 1, (3 * R, R)) * (1.6 / np.sqrt(R))
    bhh = rs.uniform(-0.1, 0.1, 3 * R)
    m = np.ones((T, N))
    if T == 3:
        m[0, 0] = m[1, 1] = m[2, 2] = 0.0      # (a single step keeps its mask: the one zero it could hold would wipe h0, and with it z * h and d(h0))
    d_hs = rs.uniform(-1, 1, (T, N, R))
    t64 = lambda x: torch.from_numpy(x).double().requires_grad_(True)   # noqa: E731
    g, h, w, b = t64(gi), t64(h0), t64(whh), t64(bhh)
    mt = torch.from_numpy(m).double()
    hs, hms, gates, ghs = [], [], [], []
    hc = h
    for t in range(T):
        hm = hc * mt[t].view(N, 1)
        gh = hm @ w.t() + b
        gh.retain_grad()
        r = torch.sigmoid(g[t][:, :R] + gh[:, :R])
        z = torch.sigmoid(g[t][:, R:2 * R] + gh[:, R:2 * R])
        n = torch.tanh(g[t][:, 2 * R:] + r * gh[:, 2 * R:])
        hc = (1.0 - z) * n + z * hm
        hs.append(hc); hms.append(hm); gates.append(torch.cat([r, z, n, gh[:, 2 * R:]], 1)); ghs.append(gh)
    (torch.stack(hs) * torch.from_numpy(d_hs).double()).sum().backward()
    ref = dict(hs=torch.stack(hs), hms=torch.stack(hms), gates=torch.stack(gates), dgi=g.grad, dgh=torch.stack([x.grad for x in ghs]), dh0=h.grad)
    ref = {k: v.detach().numpy() for k, v in ref.items()}

    f = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()   # noqa: E731
    shapes = dict(hs=(T, N, R), hms=(T, N, R), gates=(T, N, 4 * R), dgi=(T, N, 3 * R), dgh=(T, N, 3 * R), dh0=(N, R), ws_f=(3 * R * R,), ws_b=(3 * R * R,))
    ws = (lambda t: None) if null_ws else A.ptr   # noqa: E731
    outs = []
    d_gi, d_h0, d_m, d_whh, d_bhh, d_dhs = f(gi), f(h0), f(m), f(whh), f(bhh), f(d_hs)
    for _ in range(2):
        bufs = {k: guarded(s) for k, s in shapes.items()}
        v = {k: x[0] for k, x in bufs.items()}
        A.call("cn_gru_seq_fwd_sized", T, N, R, A.ptr(d_gi), A.ptr(d_h0), A.ptr(d_m), A.ptr(d_whh), A.ptr(d_bhh), A.ptr(v["hs"]), A.ptr(v["hms"]),
               A.ptr(v["gates"]), ws(v["ws_f"]), A.stream_ptr())
        A.call("cn_gru_seq_bwd_sized", T, N, R, A.ptr(v["gates"]), A.ptr(v["hms"]), A.ptr(d_m), A.ptr(d_whh), A.ptr(d_dhs), A.ptr(v["dgi"]), A.ptr(v["dgh"]),
               A.ptr(v["dh0"]), ws(v["ws_b"]), A.stream_ptr())
        torch.cuda.synchronize()
        for k, (view, whole) in bufs.items():
            assert torch.isnan(whole[view.numel():]).all(), "guard tail behind %s was written" % k
            assert k.startswith("ws_") or not torch.isnan(view).any(), k
            assert R > 128 or not k.startswith("ws_") or torch.isnan(view).all(), "the resident form wrote into %s" % k
        outs.append({k: v[k].clone() for k in ref})
    for k, r in ref.items():
        got = outs[0][k].double().cpu().numpy()
        err = float(np.abs(got - r).max())
        bar = U.VALUE_BAR if k in ("hs", "hms", "gates") else U.grad_bar(r)
        print("%s %-5s max |device - fp64| = %.3e  bar %.3e" % (gru_case_id(case), k, err, bar))
        assert err <= bar, (k, err, bar)
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_evaluate_actions_of_a_sized_policy_reaches_the_sized_sequence(monkeypatch):
    """Policy.evaluate_actions at (256, 128, 128, 512), E = 4 envs, H = 8, T = 5: two boundary calls each way, the second one cn_rn_seq_fwd_sized;
    values, log-probs and every parameter gradient agree with the same module on the torch-op route (train_fused_rn = False)."""
    import copy
    from tests import policy_util as PU
    dims, E, H, T = (256, 128, 128, 512), 4, 8, 5
    B = T * E
    pol = U.sized_policy(dims, H).cuda()
    pol_t = copy.deepcopy(pol)
    pol_t.base.train_fused_rn = False
    ob = PU.synth_obs(B, H, 2, seed=5)
    obs = {k: torch.from_numpy(v).cuda() for k, v in ob.items()}
    rs = np.random.RandomState(3)
    hxs = {"human_node_rnn": torch.from_numpy(rs.uniform(-1, 1, (E, 1, dims[0])).astype(np.float32)).cuda(),
           "human_human_edge_rnn": torch.zeros(E, H + 1, 256, device="cuda")}
    masks = torch.ones(B, 1, device="cuda")
    masks[E + 1] = 0.0
    masks[2 * E + 2] = 0.0
    actions = torch.from_numpy(rs.uniform(-1, 1, (B, 2)).astype(np.float32)).cuda()
    seen = []
    real = A.call
    monkeypatch.setattr(A, "call", lambda name, *a, **k: (seen.append(name), real(name, *a, **k))[1])
    res = {}
    for name, p in (("fused", pol), ("torch", pol_t)):
        del seen[:]
        v, lp, _, hx = p.evaluate_actions(obs, hxs, masks, actions)
        p.zero_grad()
        (v.mean() + 0.3 * lp.mean()).backward()
        res[name] = (v.detach().double().cpu(), lp.detach().double().cpu(), hx["human_node_rnn"].detach().double().cpu().reshape(E, -1),
                     {k: q.grad.detach().double().cpu() for k, q in p.named_parameters() if q.grad is not None}, list(seen))
    calls = res["fused"][4]
    assert "cn_rn_seq_fwd_sized" in calls and "cn_rn_seq_bwd_sized" in calls and "cn_hh_block_fwd" in calls, calls
    assert "cn_rn_seq_fwd_sized" not in res["torch"][4]
    for i, what in ((0, "value"), (1, "logp"), (2, "h_T")):
        err = float((res["fused"][i] - res["torch"][i]).abs().max())
        assert err <= U.VALUE_BAR, (what, err)
    assert set(res["fused"][3]) == set(res["torch"][3])
    for k, g in res["torch"][3].items():
        err = float((g - res["fused"][3][k]).abs().max())
        assert err <= U.grad_bar(g.numpy()), (k, err, float(g.abs().max()))
