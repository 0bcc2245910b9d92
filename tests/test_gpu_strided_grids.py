"""GPU tests of the PPO update's grid-capped kernels past their caps: the launchers cap the grid at what is resident and every wavefront or block
walks the rest of the work in a loop, which the small direct tests never enter.  Each case here is at least two full trips plus a ragged one past
today's cap (tests/strided_util.py restates the caps, tests/test_strided_refs.py pins them to the host code), writes into NaN-filled buffers with a
NaN guard behind them, and compares every sample (row, element) on its own with the fp64 CPU reference at the bar the kernel's small test uses.
Families: the human-human attention one size class at a time, the DS-RNN edge attention, the PPO losses and the advantage normalisation (with exact
ties planted), embed0."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from crowdnav_prediction_attngraph_amd import _abi as A  # noqa: E402
from tests import srnn_seq_util as Q  # noqa: E402
from tests import strided_util as U  # noqa: E402
from tests.test_gpu_srnn_node import _attn_params, _attn_reference, _dev, _guarded, _raw_calls  # noqa: E402


def _check_guarded(o, sizes):
    for k, n in sizes.items():
        assert not bool(torch.isnan(o[k][:n]).any()), "%s: elements left unwritten" % k
        assert bool(torch.isnan(o[k][n:]).all()), "%s: the guard behind it was written" % k


# ---- 1. human-human attention, one class at a time ----
# name: (H, [(lo, hi, samples)]); the sizes are 2 x the larger of the class's forward / backward cap + an odd remainder (mixed: backward caps)
HH_CASES = {
    "class8": (20, [(1, 8, 2 * 1024 + 37)]),
    "class16": (20, [(9, 16, 2 * 512 + 21)]),
    "class32": (48, [(17, 32, 2 * 192 + 13)]),
    "class64": (64, [(33, 64, 2 * 96 + 7)]),
    "mixed": (64, [(1, 8, 2 * 512 + 37), (9, 16, 2 * 256 + 21), (17, 32, 2 * 128 + 13), (33, 64, 2 * 32 + 7)]),
}


@functools.lru_cache(maxsize=None)
def _hh_case(name):
    H, groups = HH_CASES[name]
    nd = U.hh_counts(groups, seed=1000 * H + len(groups))
    row_off, qkv, d_out = U.hh_inputs(nd, seed=1000 * H + int(nd.numel()))
    out64, d_qkv64 = U.hh_reference(qkv, d_out, row_off)
    return dict(H=H, nd=nd, row_off=row_off, qkv=qkv, d_out=d_out, out64=out64, d_qkv64=d_qkv64)


def _hh_raw(qkv, row_off, d_out, B, H):
    """cn_hh_attention_fwd and cn_hh_attention_bwd (on the forward's class lists) into guarded buffers: (out [R,512], d_qkv [R,1536], cls)."""
    dev, R = qkv.device, qkv.shape[0]
    cls = torch.zeros(int(A.lib().cn_hh_attention_workspace_ints(B)), dtype=torch.int32, device=dev)
    sizes = dict(out=R * 512, d_qkv=R * 1536)
    o = {k: _guarded(n, dev) for k, n in sizes.items()}
    A.call("cn_hh_attention_fwd", B, H, A.ptr(qkv), A.ptr(row_off), 0.125, A.ptr(o["out"]), A.ptr(cls), A.stream_ptr())
    A.call("cn_hh_attention_bwd", B, H, A.ptr(qkv), A.ptr(row_off), A.ptr(d_out), 0.125, A.ptr(o["d_qkv"]), A.ptr(cls), 1, A.stream_ptr())
    torch.cuda.synchronize()
    _check_guarded(o, sizes)
    return o["out"][:R * 512].view(R, 512).clone(), o["d_qkv"][:R * 1536].view(R, 1536).clone(), cls.cpu()


@pytest.mark.parametrize("name", list(HH_CASES), ids=list(HH_CASES))
def test_hh_attention_class_launches_past_their_caps(name):
    """hh_attention_kernel<CAP> with class lists and the backward kernels of the same class (hh_attention_bwd_kernel<8>, hh_attention_bwd_mfma_kernel<1>,
    <2>, hh_attention_bwd_kernel<64>), samples of one class per trip, forward / backward:
      class8   cap 1024 / 512, B = 2085 of counts 1 .. 8:   3 / 5 trips, the last of 37 samples
      class16  cap  512 / 256, B = 1045 of counts 9 .. 16:  3 / 5 trips, the last of 21
      class32  cap  192 / 128, B =  397 of counts 17 .. 32: 3 / 4 trips, the last of 13
      class64  cap   96 /  32, B =  199 of counts 33 .. 64: 3 / 7 trips, the last of 7
      mixed    H = 64, B = 1934 in one seeded order: 1061 / 533 / 269 / 71 samples of the four classes, each 3 trips of its backward cap
               (forward: 2 / 2 / 2 / 1 trips)
    Per sample against fp64 (strided_util.hh_reference): output <= 2e-5, d_qkv <= 5e-5 max(1, max |reference| of that sample) -- the bars of
    test_gpu_train.py::_check_hh_attention, the second against the sample's own scale, which is never above the batch's.  Every element written, no
    guard touched; HHAttention.apply (lists rebuilt in another atomic order) gives the raw calls' bits; seven samples run alone (B = 1) give the
    bits of their rows in the batch, forward and backward."""
    from crowdnav_prediction_attngraph_amd import hip
    c, dev = _hh_case(name), _dev()
    H, nd, row_off = c["H"], c["nd"], c["row_off"]
    B = int(nd.numel())
    caps = U.hh_caps()
    cls_of = np.array([U.hh_class(int(n)) for n in nd])
    for lo, hi, n in HH_CASES[name][1]:
        assert n > 2 * (caps[hi][1] if name == "mixed" else max(caps[hi])) and int((cls_of == hi).sum()) == n, "no longer two trips past the cap: move the sizes"
    qkv, ro, d_out = c["qkv"].to(dev), row_off.to(dev), c["d_out"].to(dev)
    out, d_qkv, cls = _hh_raw(qkv, ro, d_out, B, H)
    counts, lists = cls[:4].numpy(), cls[4:].view(4, B).numpy()
    assert counts.tolist() == [int((cls_of == k).sum()) for k in U.HH_CLASSES]
    pos = np.zeros(B, np.int64)                                  # the place of every sample in its class list: what decides its trip
    for k in range(4):
        assert sorted(lists[k][:counts[k]].tolist()) == np.nonzero(cls_of == U.HH_CLASSES[k])[0].tolist()
        pos[lists[k][:counts[k]]] = np.arange(counts[k])

    def where(i):
        f, b = caps[int(cls_of[i])]
        return "nd %d, class %d, place %d in its list: forward trip %d of cap %d, backward trip %d of cap %d" % (int(nd[i]), cls_of[i], pos[i], pos[i] // f, f,
                                                                                                                 pos[i] // b, b)
    e_out = U.per_sample_max(out.cpu().double() - c["out64"], row_off)
    e_g = U.per_sample_max(d_qkv.cpu().double() - c["d_qkv64"], row_off)
    bar_g = 5e-5 * np.maximum(1.0, U.per_sample_max(c["d_qkv64"], row_off))
    m_out, ok_out = U.worst(e_out, None, "hh attention %s out" % name, 2e-5, where)
    m_g, ok_g = U.worst(e_g, None, "hh attention %s d_qkv" % name, bar_g, where)
    assert ok_out, m_out
    assert ok_g, m_g
    qg = c["qkv"].to(dev).requires_grad_()
    out2 = hip.HHAttention.apply(qg, ro, B, H, 0.125)
    out2.backward(d_out)
    assert torch.equal(out2.detach(), out) and torch.equal(qg.grad, d_qkv)
    f_cap, b_cap = (caps[HH_CASES[name][1][0][1]] if name != "mixed" else caps[8])
    alone = {0, f_cap, 2 * f_cap - 1, b_cap, 2 * b_cap - 1, B - 1} | set(np.random.RandomState(B).choice(B, 3, replace=False).tolist())
    for i in sorted(i for i in alone if i < B):
        r0, r1 = int(row_off[i]), int(row_off[i + 1])
        o1, g1, _ = _hh_raw(qkv[r0:r1].contiguous(), torch.tensor([0, r1 - r0], dtype=torch.int32, device=dev), d_out[r0:r1].contiguous(), 1, H)
        assert torch.equal(o1, out[r0:r1]), "forward of sample %d alone: %s" % (i, where(i))
        assert torch.equal(g1, d_qkv[r0:r1]), "backward of sample %d alone: %s" % (i, where(i))


# ---- 2. DS-RNN edge attention ----
SRNN_CASES = [(2 * U.SA_CAP + 53, 1), (2 * U.SA_CAP + 53, 9)]


@pytest.mark.parametrize("case", SRNN_CASES, ids=lambda c: "b%d_h%d" % c)
def test_srnn_attention_past_its_cap(case):
    """srnn_attn_fwd_kernel / srnn_attn_bwd_kernel: cap 256 workgroups x 16 wavefronts = 4096 samples a trip; B = 8245: 3 trips, the last of 53
    samples (4 workgroups, the last with 5 wavefronts at work).  H = 1: a softmax of one; H = 9: the second chunk of SA_CHUNK = 8 rows, in flight
    across the trips, with d_t_direct NULL and given (H = 1: NULL).  Reference, inputs and bars of test_gpu_srnn_node.py: forward at max(1e-4, 4 d),
    gradients by srnn_seq_util.check_grads, the bias of spatial_edge_layer an exact zero; on top, per sample: weighted and attn at the forward bar,
    d_h_all at 5e-4 of the batch's largest entry.  SrnnAttention.apply gives the raw calls' bits; samples 0, 4095, 4096, 8191, 8192 and B - 1 alone
    give the bits of their batch rows in all seven outputs.
    At H = 1 the softmax is constant: the gradients of Wt, bt and Ws are exact zeros in fp64 and check_grads holds them to its floor of 1e-7.  The
    kernel's d_u is an exact zero there too (the subtraction in it is not contracted into an fma); as a rounding residual per sample it summed to
    1.2e-6 .. 1.4e-6 over these 8245 samples, which this case found."""
    from crowdnav_prediction_attngraph_amd.hip import SrnnAttention
    B, H = case
    assert B > 2 * U.SA_CAP, "no longer two trips past the cap: move the sizes"
    ref, dev = _attn_reference(case), _dev()
    bar = max(1e-4, 4 * ref["d"])
    flat, d_w = ref["h_all"].to(dev), ref["d_w"].to(dev)
    T, N = 5, B // 5
    for direct in ((False, True) if H == 9 else (False,)):
        tag = "srnn attention b%d_h%d %s" % (B, H, "direct" if direct else "null")
        d_t = ref["d_t"].to(dev) if direct else None
        want = dict(ref[direct])
        params = _attn_params(dev)
        raw = _raw_calls(flat, params, d_w, d_t, H)
        e_w = (raw["weighted"].cpu().double().view(B, 256) - ref["w64"]).abs().amax(1).numpy()
        e_a = (raw["attn"].cpu().double().view(B, H) - ref["a64"]).abs().amax(1).numpy()
        e_h = (raw["d_h_all"].cpu().double().view(B, -1) - want["d_h_all"].reshape(B, -1)).abs().amax(1).numpy()
        print("%s: d = %.3g" % (tag, ref["d"]))
        for err, what, b in ((e_w, "weighted", bar), (e_a, "attn", bar), (e_h, "d_h_all", 5e-4 * float(want["d_h_all"].abs().max()))):
            msg, ok = U.worst(err, U.SA_CAP, "%s %s" % (tag, what), b)
            assert ok, msg
        h_all = flat.view(T, N, H + 1, 256).clone().requires_grad_(True)
        out = SrnnAttention.apply(h_all, *params, True) if direct else SrnnAttention.apply(h_all, *params)
        assert torch.equal(out[0].detach().reshape(-1), raw["weighted"]) and torch.equal(out[1].reshape(-1), raw["attn"])
        loss = (out[0].view(B, 256) * d_w).sum()
        if direct:
            assert torch.equal(out[2].reshape(B, 256), flat[:, 0])
            loss = loss + (out[2].view(B, 256) * d_t).sum()
        loss.backward()
        assert torch.equal(h_all.grad.reshape(-1), raw["d_h_all"])
        got = dict(d_h_all=h_all.grad.cpu().double().view(B, H + 1, 256), **{k: p.grad.cpu().double() for k, p in zip(("Wt", "bt", "Ws", "bs"), params)})
        assert got["bs"].shape == (64,) and not bool(got["bs"].any()), "the bias of spatial_edge_layer must get an exact zero"
        Q.check_grads(got, {k: v for k, v in want.items() if k != "bs"}, "fp32", tag)
        assert float(want["bs"].abs().max()) <= 1e-9
        del h_all, out, loss, got
    for r in (0, U.SA_CAP - 1, U.SA_CAP, 2 * U.SA_CAP - 1, 2 * U.SA_CAP, B - 1):
        one = _raw_calls(flat[r:r + 1].contiguous(), params, d_w[r:r + 1].contiguous(), None if d_t is None else d_t[r:r + 1].contiguous(), H)
        for k, t in one.items():
            assert torch.equal(t, raw[k].view(B, -1)[r]), "%s of sample %d (trip %d) alone" % (k, r, r // U.SA_CAP)


# ---- 3. PPO losses and advantage normalisation ----
PPO_NS = [12, 3 * U.PPO_FWD_CAP + 77, 2 * U.PPO_BWD_CAP + 77]


@functools.lru_cache(maxsize=None)
def _ppo_case(n):
    inputs, pos, kind = U.ppo_inputs(n, seed=n)
    return inputs, pos, kind, U.ppo_reference(inputs)


@pytest.mark.parametrize("n", PPO_NS)
def test_ppo_loss_past_its_caps_with_planted_ties(n):
    """ppo_loss_partial_kernel: cap 256 blocks x 256 = 65 536 elements a trip; ppo_loss_bwd_kernel: 2048 x 256 = 524 288.
      n = 12          every tie of strided_util.PPO_TIES and one random sample, one block
      n = 196 685     forward 4 trips (the last of 77 elements), backward one
      n = 1 048 653   forward 17 trips, backward 3 (the last of 77)
    clip = 0.25, clipped value loss; random samples as test_gpu_ppo.py draws them (kept off the gradient's kinks, strided_util.ppo_inputs), every tie
    planted at two seeded positions and at one of the last 77 elements.  Against fp64 autograd over test_gpu_ppo.py::_ref_losses: losses at rtol
    2e-6; d_values and d_logp per element at rtol 1e-5, atol 1e-9; at the planted positions at rtol 1e-6 with zeros exact, against the reference and
    against the hand-written closed form.  PPOLoss.apply gives the raw calls' bits."""
    from crowdnav_prediction_attngraph_amd import hip
    inputs, pos, kind, (vl, al, dv64, dlp64) = _ppo_case(n)
    dev = _dev()
    assert n == 12 or (n > 3 * U.PPO_FWD_CAP if n < U.PPO_BWD_CAP else n > 2 * U.PPO_BWD_CAP), "no longer past the cap: move the sizes"
    ts = [t.reshape(-1).to(dev) for t in inputs]
    sizes = dict(losses=2, d_values=n, d_logp=n)
    o = {k: _guarded(m, dev) for k, m in sizes.items()}
    ws = torch.empty(A.lib().cn_ppo_loss_workspace_doubles(), dtype=torch.float64, device=dev)
    g = torch.tensor([0.5, 1.0], device=dev)                     # the gradient of 0.5 value_loss + action_loss
    A.call("cn_ppo_loss_fwd", n, *[A.ptr(t) for t in ts], U.PPO_CLIP, 1, A.ptr(ws), A.ptr(o["losses"]), A.stream_ptr())
    A.call("cn_ppo_loss_bwd", n, *[A.ptr(t) for t in ts], U.PPO_CLIP, 1, A.ptr(g), A.ptr(o["d_values"]), A.ptr(o["d_logp"]), A.stream_ptr())
    torch.cuda.synchronize()
    _check_guarded(o, sizes)
    losses = o["losses"][:2].cpu().double().numpy()
    print("ppo loss n = %d: value_loss %.9g (fp64 %.9g, rel %.3g), action_loss %.9g (fp64 %.9g, rel %.3g), bar 2e-6"
          % (n, losses[0], vl, abs(losses[0] - vl) / abs(vl), losses[1], al, abs(losses[1] - al) / abs(al)))
    np.testing.assert_allclose(losses, [vl, al], rtol=2e-6)
    want_v, want_l = U.ppo_tie_gradients(kind, n)
    for name, want64, closed in (("d_values", dv64, want_v), ("d_logp", dlp64, want_l)):
        got = o[name][:n].cpu().double().numpy()
        want = want64.reshape(-1).numpy()
        msg, ok = U.worst(np.abs(got - want), U.PPO_BWD_CAP, "ppo loss n = %d %s" % (n, name), 1e-9 + 1e-5 * np.abs(want))
        assert ok, msg
        tie = np.abs(got[pos] - want[pos]) / np.where(want[pos] == 0, 1.0, np.abs(want[pos]))
        print("ppo loss n = %d %s at the %d planted ties: worst relative error %.3g (bar 1e-6, zeros exact), %d of them in the last trip"
              % (n, name, pos.size, tie.max(), int((pos >= n - 77).sum())))
        np.testing.assert_allclose(got[pos], want[pos], rtol=1e-6, atol=0, err_msg="%s at %s" % (name, [U.PPO_TIES[k][0] for k in kind]))
        np.testing.assert_allclose(got[pos], closed, rtol=1e-6, atol=0, err_msg="%s against the closed form" % name)
    vg, lg = inputs[0].to(dev).requires_grad_(), inputs[1].to(dev).requires_grad_()
    l2 = hip.PPOLoss.apply(vg, lg, *[t.to(dev) for t in inputs[2:]], U.PPO_CLIP, True)
    (0.5 * l2[0] + l2[1]).backward()
    assert torch.equal(l2.detach(), o["losses"][:2])
    assert torch.equal(vg.grad.reshape(-1), o["d_values"][:n]) and torch.equal(lg.grad.reshape(-1), o["d_logp"][:n])


def test_advantage_normalisation_past_its_cap():
    """adv_norm_kernel: cap 2048 blocks x 256 = 524 288 elements a trip; n = 1 048 653: 3 trips, the last of 77 elements (adv_stats_kernel: one block
    of 1024 threads, 1025 trips).  Against (a - mean) / (std(ddof = 1) + 1e-5) in fp64 numpy on a = the float32 difference returns - values, which
    is what the kernels take: every element at atol 1e-5; the count exact; a second run gives the same bits."""
    from crowdnav_prediction_attngraph_amd import hip
    n = PPO_NS[2]
    assert n > 2 * U.ADV_CAP, "no longer two trips past the cap: move the sizes"
    inputs = _ppo_case(n)[0]
    dev = _dev()
    ret, val = inputs[5].to(dev), inputs[0].to(dev)
    want = U.adv_reference(inputs[5], inputs[0])
    runs = []
    for _ in range(2):
        stats = hip.adv_stats(ret, val, n)
        out = _guarded(n, dev)
        hip.adv_normalize(ret, val, stats, n, out)
        torch.cuda.synchronize()
        _check_guarded(dict(adv=out), dict(adv=n))
        runs.append((stats.cpu(), out[:n].cpu()))
    assert float(runs[0][0][2]) == n
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    msg, ok = U.worst(np.abs(runs[0][1].double().numpy() - want), U.ADV_CAP, "advantage normalisation n = %d" % n, 1e-5)
    assert ok, msg


# ---- 4. embed0 ----
EMBED0_RS = [2 * U.EMBED0_FWD_CAP + 5, 2 * U.EMBED0_BWD_CAP + 3]


def _embed0_raw(x, w, b, dy, y=None):
    """cn_embed0_fwd (y = None) and cn_embed0_bwd with Embed0.backward's block count into guarded buffers: (y [R,128], dWb [128, D+1])."""
    dev, (R, D) = x.device, x.shape
    blocks = min(R, U.EMBED0_BWD_CAP // 8)
    sizes = dict(part=blocks * 128 * (D + 1), dWb=128 * (D + 1))
    if y is None:
        sizes["y"] = R * 128
    o = {k: _guarded(n, dev) for k, n in sizes.items()}
    if y is None:
        A.call("cn_embed0_fwd", R, D, A.ptr(x), A.ptr(w), A.ptr(b), A.ptr(o["y"]), A.stream_ptr())
        y = o["y"][:R * 128].view(R, 128).clone()
    A.call("cn_embed0_bwd", R, D, A.ptr(x), A.ptr(y), A.ptr(dy), blocks, A.ptr(o["part"]), A.ptr(o["dWb"]), A.stream_ptr())
    torch.cuda.synchronize()
    _check_guarded(o, sizes)
    return y, o["dWb"][:128 * (D + 1)].view(128, D + 1).clone()


@pytest.mark.parametrize("D", [2, 12])
@pytest.mark.parametrize("R", EMBED0_RS)
def test_embed0_past_its_caps(R, D):
    """embed0_fwd_kernel: cap 8192 blocks, one row a trip each; embed0_bwd_kernel: 4096 blocks (hip_train.Embed0), eight rows a trip each = 32 768.
      R = 16 389   forward 3 trips (the last of 5 rows), backward one (blocks 0 .. 4 hold five rows, the others four)
      R = 65 539   forward 9 trips, backward 3 (the last of 3 rows: one row in blocks 0 .. 2, the other seven slots past the end)
    Inputs, reference and bars of test_gpu_train.py::test_embed0_forward_and_gradients_match_fp64 (padding rows of 15.0; the kernel's own active
    set, which may differ from the fp64 one only below the bar): y per row, dW and db at 2e-5 of the largest reference magnitude.  A second
    backward with dy zero but on eight rows spread over the trips (the first row of each later trip, the ragged tail) sees single rows, which the
    sums over all R rows hide.  Embed0.apply gives the raw calls' bits."""
    from crowdnav_prediction_attngraph_amd import hip
    assert R > 2 * (U.EMBED0_FWD_CAP if R == EMBED0_RS[0] else U.EMBED0_BWD_CAP), "no longer two trips past the cap: move the sizes"
    dev = _dev()
    x, w, b, dy = U.embed0_inputs(R, D)
    xd, wd, bd, dyd = (t.to(dev) for t in (x, w, b, dy))
    y, dwb = _embed0_raw(xd, wd, bd, dyd)
    act = y.cpu() > 0
    pre, dw64, db64 = U.embed0_reference(x, w, b, dy, act)
    want_y = pre.clamp(min=0)
    bar_y = 2e-5 * max(float(want_y.max()), 1.0)
    flipped = pre[act != (pre > 0)].abs()
    assert flipped.numel() == 0 or float(flipped.max()) <= bar_y
    tag = "embed0 R = %d D = %d" % (R, D)
    msg, ok = U.worst((y.cpu().double() - want_y).abs().amax(1).numpy(), U.EMBED0_FWD_CAP, tag + " y", bar_y)
    assert ok, msg

    def grads(dwb, dw64, db64, what):
        for got, want, name in ((dwb[:, :D], dw64, "dW"), (dwb[:, D], db64, "db")):
            err, bar_g = float((got.cpu().double() - want).abs().max()), 2e-5 * max(float(want.abs().max()), 1.0)
            print("%s %s%s: worst %.3g (bar %.3g)" % (tag, name, what, err, bar_g))
            assert err <= bar_g, (name, what, err, bar_g)
    grads(dwb, dw64, db64, "")
    rows = sorted({0, 4096, U.EMBED0_FWD_CAP, min(U.EMBED0_BWD_CAP, R - 4), min(2 * U.EMBED0_BWD_CAP - 1, R - 5), R - 3, R - 2, R - 1})
    few = torch.zeros_like(dy)
    few[rows] = dy[rows]
    _, dwb_few = _embed0_raw(xd, wd, bd, few.to(dev), y)
    _, dw_few, db_few = U.embed0_reference(x, w, b, few, act)
    assert float(db_few.abs().max()) > 0.5
    grads(dwb_few, dw_few, db_few, " of %d rows" % len(rows))
    wg, bg = w.to(dev).requires_grad_(), b.to(dev).requires_grad_()
    y2 = hip.Embed0.apply(xd, wg, bg)
    y2.backward(dyd)
    assert torch.equal(y2.detach(), y) and torch.equal(wg.grad, dwb[:, :D]) and torch.equal(bg.grad, dwb[:, D])
