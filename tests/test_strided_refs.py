"""CPU tests of tests/strided_util.py, the references of tests/test_gpu_strided_grids.py: the vectorised fp64 human-human attention against the
per-sample loop, the planted PPO ties against their closed form, the caps restated from the launchers against the host code they restate, and the
cap comments in the sources that point at the strided tests."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import strided_util as U  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crowdnav_prediction_attngraph_amd")


def test_vectorised_hh_reference_equals_the_per_sample_loop():
    """B = 40, H = 33 (counts 1 .. 33 with 1, 8, 9 and 33 planted: all four classes): output and gradient within 1e-12."""
    g = torch.Generator().manual_seed(33040)
    nd = torch.randint(1, 34, (40,), generator=g)
    nd[:4] = torch.tensor([1, 8, 9, 33])
    row_off, qkv, d_out = U.hh_inputs(nd, 33040)
    out, d_qkv = U.hh_reference(qkv, d_out, row_off)
    out_l, d_qkv_l = U.hh_reference_loop(qkv, d_out, row_off)
    assert out.shape == out_l.shape and d_qkv.shape == d_qkv_l.shape and out.dtype == d_qkv.dtype == torch.float64
    assert float((out - out_l).abs().max()) <= 1e-12 and float((d_qkv - d_qkv_l).abs().max()) <= 1e-12
    assert float(out_l.abs().max()) > 0.1 and float(d_qkv_l.abs().max()) > 0.1
    per = U.per_sample_max(out, row_off)
    assert per.shape == (40,) and per[3] == float(out[int(row_off[3]):int(row_off[4])].abs().max())


def test_hh_counts_fill_their_classes():
    nd = U.hh_counts([(17, 32, 50)], 1)
    assert int(nd.min()) == 17 and int(nd.max()) == 32 and nd.numel() == 50
    mixed = U.hh_counts([(1, 8, 30), (9, 16, 20), (17, 32, 10), (33, 64, 5)], 2)
    cls = np.array([U.hh_class(int(n)) for n in mixed])
    assert [int((cls == c).sum()) for c in U.HH_CLASSES] == [30, 20, 10, 5]
    assert len(set(cls[:30].tolist())) > 1                  # the classes are interleaved, not concatenated


@pytest.mark.parametrize("n", [12, 5000])
def test_planted_ties_follow_the_closed_form(n):
    """The fp64 autograd reference at the planted positions equals the hand-written table (gradients of 0.5 value_loss + action_loss, 1e-12
    relative, zeros exact); every tie of the table is planted, at n = 5000 also among the last 77 elements; at n = 12 the loss itself."""
    inputs, pos, kind = U.ppo_inputs(n, seed=n)
    assert sorted(set(kind.tolist())) == list(range(len(U.PPO_TIES))) and len(set(pos.tolist())) == pos.size
    assert n == 12 or int((pos >= n - 77).sum()) == len(U.PPO_TIES)
    vl, al, dv, dlp = U.ppo_reference(inputs)
    want_v, want_l = U.ppo_tie_gradients(kind, n)
    np.testing.assert_allclose(dv.numpy()[pos, 0], want_v, rtol=1e-12, atol=0)
    np.testing.assert_allclose(dlp.numpy()[pos, 0], want_l, rtol=1e-12, atol=0)
    assert {0.0, 0.5, -0.75} <= set(np.round(want_l * n, 9).tolist()) and np.count_nonzero(want_v == 0) >= 3
    if n == 12:
        # the planted eleven by hand: 0.5 max((v - ret)^2, (vpc - ret)^2) and -min(surr1, surr2) of PPO_TIES, in order; the twelfth from the formula
        v_terms = [0.5, 0.5, 0.5, 0.5, 0.28125, 0.28125, 0.5, 0.0, 0.0, 0.28125, 0.5]
        a_terms = [0.0, -0.75, 0.5, 0.0, -0.5, -0.5, -0.5, -0.5, -0.5, -0.5, -0.5]
        v, lp, old, adv, vp, ret = (float(t[11, 0]) for t in inputs)
        ratio = np.exp(lp - old)
        vpc = vp + min(max(v - vp, -0.25), 0.25)
        v_terms.append(0.5 * max((v - ret) ** 2, (vpc - ret) ** 2))
        a_terms.append(-min(ratio * adv, min(max(ratio, 0.75), 1.25) * adv))
        assert vl == pytest.approx(sum(v_terms) / 12, rel=1e-12) and al == pytest.approx(sum(a_terms) / 12, rel=1e-12)


def test_random_ppo_samples_keep_off_the_kinks():
    inputs, pos, _ = U.ppo_inputs(200000, seed=3)
    values, logp, old, adv, vp, ret = (t.double().reshape(-1) for t in inputs)
    free = np.ones(200000, bool)
    free[pos] = False
    ratio = torch.exp(logp - old).numpy()[free]
    d = (values - vp).numpy()[free]
    assert np.abs(ratio - 0.75).min() >= U.PPO_KINK_MARGIN and np.abs(ratio - 1.25).min() >= U.PPO_KINK_MARGIN
    assert np.abs(np.abs(d) - 0.25).min() >= U.PPO_KINK_MARGIN
    past = np.abs(d) > 0.25
    mid = (values.numpy()[free] + vp.numpy()[free] + np.clip(d, -0.25, 0.25)) / 2
    assert np.abs(ret.numpy()[free] - mid)[past].min() >= U.PPO_KINK_MARGIN
    assert (ratio < 0.75).any() and (ratio > 1.25).any() and (np.abs(d) > 0.25).any() and (np.abs(d) < 0.25).any()


def test_adv_reference_takes_the_fp32_difference():
    ret, val = torch.tensor([[1.0], [2.0], [4.0]]), torch.tensor([[0.5], [0.5], [0.5]])
    np.testing.assert_allclose(U.adv_reference(ret, val), (np.array([0.5, 1.5, 3.5]) - 11 / 6) / (np.sqrt(7 / 3) + 1e-5), rtol=1e-14)
    big, one = torch.tensor([[16777216.0]] * 2), torch.tensor([[1.0], [-1.0]])
    # 2^24 - 1 is a float32, 2^24 + 1 is not: the float32 difference rounds it to 2^24 and the reference follows the kernel there
    np.testing.assert_allclose(U.adv_reference(big, one), (np.array([-0.5, 0.5])) / (np.sqrt(0.5) + 1e-5), rtol=1e-14)


def test_embed0_reference_is_the_masked_linear_layer():
    x, w, b, dy = U.embed0_inputs(37, 5)
    assert bool((x[37 // 2] == 15.0).all())
    act = torch.nn.functional.linear(x, w, b) > 0
    pre, dw, db = U.embed0_reference(x, w, b, dy, act)
    wr, br = w.double().requires_grad_(), b.double().requires_grad_()
    (torch.nn.functional.linear(x.double(), wr, br) * act.double() * dy.double()).sum().backward()
    assert float((pre - torch.nn.functional.linear(x.double(), w.double(), b.double())).abs().max()) <= 1e-12
    assert float((dw - wr.grad).abs().max()) <= 1e-12 and float((db - br.grad).abs().max()) <= 1e-12


def _text(*parts):
    with open(os.path.join(PKG, *parts)) as f:
        return f.read()


def test_caps_are_the_launchers():
    """The numbers the strided tests size themselves by, against the host code: a retuned cap fails here first and names the test to move."""
    assert U.hh_caps() == {8: (1024, 512), 16: (512, 256), 32: (192, 128), 64: (96, 32)}
    att = _text("csrc", "attention.h")
    assert len(re.findall(r"blocks > 256 \* per_cu\) blocks = 256 \* per_cu;", att)) == 3
    assert "int wpb = (int)(65536 / per_wave); wpb = wpb < 1 ? 1 : (wpb > 4 ? 4 : wpb);" in att and "const int wpb = CAP == 16 ? 4 : 2, per_cu = 2;" in att
    sa = _text("csrc", "srnn_node_train.hip")
    waves, blocks = (int(re.search(r"constexpr int %s = (\d+)" % k, sa).group(1)) for k in ("SA_WAVES", "SA_MAX_BLOCKS"))
    assert waves * blocks == U.SA_CAP and int(re.search(r"constexpr int SA_CHUNK = (\d+)", sa).group(1)) == 8
    ppo = _text("csrc", "ppo.hip")
    assert int(re.search(r"constexpr int PPO_BLOCKS = (\d+)", ppo).group(1)) * 256 == U.PPO_FWD_CAP
    bwd = ppo[ppo.index('extern "C" int cn_ppo_loss_bwd'):ppo.index('extern "C" int cn_adam_workspace_doubles')]
    assert int(re.search(r"if \(blocks > (\d+)\) blocks = \1;", bwd).group(1)) * 256 == U.PPO_BWD_CAP
    ro = _text("csrc", "rollout.hip")
    norm = ro[ro.index('extern "C" int cn_adv_normalize'):]
    assert int(re.search(r"if \(blocks > (\d+)\) blocks = \1;", norm).group(1)) * 256 == U.ADV_CAP
    lin = _text("csrc", "linear.hip")
    assert int(re.search(r"const int blocks = R < (\d+) \? R : \1;", lin).group(1)) == U.EMBED0_FWD_CAP
    assert "r0 += 8 * gridDim.x" in lin
    ht = _text("hip_train.py")
    assert [8 * int(m) for m in re.findall(r"blocks = min\(R, (\d+)\)", ht)] == [U.EMBED0_BWD_CAP] * 2


def test_every_cap_names_the_strided_tests():
    """A comment beside each cap points at tests/test_gpu_strided_grids.py."""
    where = [(("csrc", "attention.h"), r"blocks = 256 \* per_cu;", 3), (("csrc", "srnn_node_train.hip"), r"constexpr int SA_MAX_BLOCKS", 1),
             (("csrc", "ppo.hip"), r"constexpr int PPO_BLOCKS", 1), (("csrc", "ppo.hip"), r"if \(blocks > 2048\) blocks = 2048;", 2),
             (("csrc", "rollout.hip"), r"if \(blocks > 2048\) blocks = 2048;", 1), (("csrc", "linear.hip"), r"const int blocks = R < 8192", 1),
             (("hip_train.py",), r"blocks = min\(R, 4096\)", 2)]
    for parts, pattern, count in where:
        lines = [ln for ln in _text(*parts).splitlines() if re.search(pattern, ln)]
        assert len(lines) == count, (parts, pattern, len(lines))
        named = [ln for ln in lines if "test_gpu_strided_grids.py" in ln]
        # (ppo.hip's second 2048 is the Adam step's grid, which tests/test_gpu_ppo.py walks 2.5 M elements through: it carries no pointer here)
        assert len(named) == (1 if parts[-1] == "ppo.hip" and "2048" in pattern else count), (parts, pattern)
