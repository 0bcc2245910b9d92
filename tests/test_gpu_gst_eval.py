"""-m gpu: evaluation of the GST predictor on the device (cn_gst_eval_step / HipGstEvaluator / gst_train.evaluate and .test with backend='hip').

Validation mode is pinned to the reference's numbers (tests/golden/gst_train_h20.npz items, tests/golden/gst_eval_h20.npz validation split) and to
the torch-op graph on random weights, ragged presence and padded batches; test mode (S sampled decodes on the caller's draws) to the reference's
recorded draws and to the torch graph with the same draws.

Bars.  Loss and Gaussian parameters 2e-5 (what cn_gst_train_step holds against the same numbers); per-pedestrian aoe / foe 1.5e-4 (the norm of
a five-step cumulative sum of mean errors of at most 2e-5 per coordinate: 5 x sqrt(2) x 2e-5).  Test mode against the reference: max(2e-5, 4 d) per
quantity, d = the largest |float32 - float64| of the sampling torch graph on the CPU over the golden sequences with the golden's draws, computed and
printed by the test itself.  Measured on the CPU: d = 4.6e-8 (per-sample loss), 4.5e-6 (per-sample aoe sum), 5.4e-6 (per-sample foe sum), which
gives bars of 2e-5, 2e-5 and 2.16e-5; the aggregates' d are printed alongside."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.test_gst_train import GOLDEN, ITEMS, _model  # noqa: E402

BAR, BAR_OE = 2e-5, 1.5e-4
CASES = [(1, 3, 0), (2, 20, 1), (3, 37, 2), (1, 64, 3), (33, 20, 4)]
AGG = ("loss", "aoe_mean", "aoe_std", "aoe_min", "foe_mean", "foe_std", "foe_min")     # column order of gst_train._test_row


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "gst_train_h20.npz"))


@pytest.fixture(scope="module")
def gold_eval():
    return np.load(os.path.join(GOLDEN, "gst_eval_h20.npz"))


@pytest.fixture(scope="module")
def data_dir(gold, tmp_path_factory):
    d = tmp_path_factory.mktemp("gstds_gpu_eval")
    with open(str(d / "0.txt"), "w") as f:
        f.write(str(gold["file_lines"]) + "\n")
    return str(d)


def _loader(ds, idx=None):
    from torch.utils.data import DataLoader, Subset
    return DataLoader(ds if idx is None else Subset(ds, list(idx)), batch_size=1, shuffle=False)


def _ragged(B, N, seed):
    """The generator of test_hip_training_step_equals_torch_autograd_on_batches_and_ragged_presence: random weights, a pedestrian present
    throughout, one without a last observed step, one never present, -999 where missing."""
    from crowdnav_prediction_attngraph_amd.gst import GSTPredictor
    torch.manual_seed(100 + seed)
    model = GSTPredictor().cuda()
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.05 * torch.randn_like(p))
    model.eval()
    g = torch.Generator().manual_seed(seed)
    lm = (torch.rand(B, N, 10, generator=g) > 0.25).float()
    lm[:, 0] = 1.0
    lm[:, 1, 4] = 0.0
    if N > 2:
        lm[:, 2, :] = 0.0
    v_obs = torch.where(lm[:, :, :5].permute(0, 2, 1).unsqueeze(-1) > 0, 0.4 * torch.randn(B, 5, N, 2, generator=g), torch.full((B, 5, N, 2), -999.0))
    v_pred = torch.where(lm[:, :, 5:].permute(0, 2, 1).unsqueeze(-1) > 0, 0.4 * torch.randn(B, 5, N, 2, generator=g), torch.full((B, 5, N, 2), -999.0))
    return model, lm, v_obs, v_pred, g


def _torch_rows(T, model, lm, v_obs, v_pred, noise=None):
    """The op graph per sequence (and per sample) on the device -> seq [B,R,4], ped [B,R,N,3], gauss [B,R,5,N,5] like evaluate_batch."""
    B, N = lm.shape[:2]
    R = 1 if noise is None else noise.shape[1]
    seq, ped, gauss = torch.zeros(B, R, 4), torch.zeros(B, R, N, 3), torch.zeros(B, R, 5, N, 5)
    with torch.no_grad():
        for b in range(B):
            l1 = lm[b:b + 1].cuda()
            am = (l1[0].t().unsqueeze(2) * l1[0].t().unsqueeze(1))[:5].unsqueeze(0)
            for s in range(R):
                nz = None if noise is None else noise[b, s:s + 1].cuda()
                gp, xs, info = T.forward_train(model, v_obs[b:b + 1].cuda(), am, l1, 0.0, nz)
                vp = v_pred[b:b + 1].cuda()
                pl, elm = T.negative_log_likelihood_full_partial(gp, vp, info["loss_mask_rel_full_partial"], l1[:, :, 5:])
                lpp = info["loss_mask_per_pedestrian"]
                aoe, foe = T.average_offset_error(xs, vp, lpp), T.final_offset_error(xs, vp, lpp)
                seq[b, s] = torch.stack((pl.sum(), elm.sum(), aoe.sum(), foe.sum())).cpu()
                ped[b, s] = torch.stack((aoe, foe, lpp[0]), -1).cpu()
                gauss[b, s] = torch.cat(gp, -1)[0].cpu()
    return seq, ped, gauss


def _close(a, b, bar, what, tensor_scale=False):
    """|a - b| <= bar x max(1, |b|), element by element (tensor_scale: |b|'s largest entry, the training test's rule for the Gaussian parameters)."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert torch.isfinite(a).all(), what
    scale = b.abs().max().clamp(min=1.0) if tensor_scale else b.abs().clamp(min=1.0)
    err = float(((a - b).abs() / scale).max())
    print("%-70s err = %.3e  bar = %.1e" % (what, err, bar))
    assert err <= bar, (what, err, bar)


def _compare(hip, ref, what):
    (seq, ped, gauss), (rseq, rped, rgauss) = hip, ref
    assert torch.equal(seq[..., 1].cpu(), rseq[..., 1]), what + ": valid (step, pedestrian) pairs"
    assert torch.equal(ped[..., 2].cpu(), rped[..., 2]), what + ": loss_mask_per_pedestrian"
    _close(seq[..., 0] / seq[..., 1], rseq[..., 0] / rseq[..., 1], BAR, what + ": loss")
    _close(gauss, rgauss, BAR, what + ": Gaussian parameters", tensor_scale=True)
    _close(ped[..., :2], rped[..., :2], BAR_OE, what + ": aoe / foe per pedestrian")
    absent = rped[..., 2] == 0
    assert float(ped[..., :2].cpu()[absent].abs().max() if absent.any() else 0.0) == 0.0, what + ": aoe / foe of a pedestrian not present throughout"
    _close(seq[..., 2:], ped[..., :2].sum(2), BAR, what + ": sums of aoe / foe")


def test_validation_mode_matches_the_reference_items_and_validation_split(gold, gold_eval, data_dir):
    from crowdnav_prediction_attngraph_amd import gst_train as T
    model = _model(gold).cuda()
    ev = T.HipGstEvaluator(model)
    ds = T.TrajectoriesDataset(data_dir)
    for it in ITEMS:
        item = ds[it]
        seq, ped, gauss = ev.evaluate_batch(item[6].unsqueeze(0), item[8].unsqueeze(0), item[4].unsqueeze(0))
        assert abs(float(seq[0, 0, 0] / seq[0, 0, 1]) - float(gold["item%d_loss" % it])) <= BAR
        g = gauss[0, 0].cpu().numpy()
        for n, sl in (("mu", slice(0, 2)), ("sx", slice(2, 3)), ("sy", slice(3, 4)), ("corr", slice(4, 5))):
            np.testing.assert_allclose(g[..., sl], gold["item%d_%s" % (it, n)][0], rtol=0, atol=BAR)
        np.testing.assert_allclose(ped[0, 0, :, 0].cpu().numpy(), gold["item%d_aoe" % it], rtol=0, atol=BAR_OE)
        np.testing.assert_allclose(ped[0, 0, :, 1].cpu().numpy(), gold["item%d_foe" % it], rtol=0, atol=BAR_OE)
    dv = T.TrajectoriesDataset(data_dir, mode="val")
    items = [dv[i] for i in range(len(dv))]
    seq, ped, _ = ev.evaluate_batch([i[6] for i in items], [i[8] for i in items], [i[4] for i in items])
    seq = seq.cpu().numpy()
    np.testing.assert_allclose(seq[:, 0, 0] / seq[:, 0, 1], gold_eval["val_loss"], rtol=0, atol=BAR)
    np.testing.assert_allclose(seq[:, 0, 2], gold_eval["val_aoe_sum"], rtol=0, atol=BAR_OE)
    np.testing.assert_allclose(seq[:, 0, 3], gold_eval["val_foe_sum"], rtol=0, atol=BAR_OE)
    np.testing.assert_array_equal(ped[:, 0, :, 2].sum(1).cpu().numpy(), gold_eval["val_m"])
    triple = T.evaluate(model, _loader(dv), "cuda", backend="hip")
    for a, b, bar in zip(triple, gold_eval["val_triple"], (BAR, BAR_OE, BAR_OE)):
        assert abs(a - float(b)) <= bar, (triple, gold_eval["val_triple"])


@pytest.mark.parametrize("B,N,seed", CASES)
def test_validation_mode_equals_the_torch_graph_on_batches_and_ragged_presence(B, N, seed):
    from crowdnav_prediction_attngraph_amd import gst_train as T
    model, lm, v_obs, v_pred, _ = _ragged(B, N, seed)
    ev = T.HipGstEvaluator(model)
    hip = ev.evaluate_batch(v_obs, v_pred, lm)
    assert tuple(hip[0].shape) == (B, 1, 4) and tuple(hip[1].shape) == (B, 1, N, 3) and tuple(hip[2].shape) == (B, 1, 5, N, 5)
    _compare(hip, _torch_rows(T, model, lm, v_obs, v_pred), "validation B=%d N=%d" % (B, N))


def test_batching_and_padding_change_nothing_beyond_rounding_and_calls_repeat_bit_for_bit():
    from crowdnav_prediction_attngraph_amd import gst_train as T
    model, lm, v_obs, v_pred, g = _ragged(4, 30, 9)
    sizes = (30, 3, 17, 8)
    vo, vp, l = [v_obs[b, :, :n] for b, n in enumerate(sizes)], [v_pred[b, :, :n] for b, n in enumerate(sizes)], [lm[b, :n] for b, n in enumerate(sizes)]
    noise = [torch.randn(3, 5, n, 2, generator=g) for n in sizes]
    ev = T.HipGstEvaluator(model)
    for nz in (None, noise):
        seq, ped, gauss = ev.evaluate_batch(vo, vp, l, nz)
        again = ev.evaluate_batch(vo, vp, l, nz)
        assert all(torch.equal(a, b) for a, b in zip((seq, ped, gauss), again))
        for b, n in enumerate(sizes):
            alone = ev.evaluate_batch(vo[b].unsqueeze(0), vp[b].unsqueeze(0), l[b].unsqueeze(0), None if nz is None else nz[b].unsqueeze(0))
            _compare((seq[b:b + 1], ped[b:b + 1, :, :n], gauss[b:b + 1, :, :, :n]), tuple(t.cpu() for t in alone), "sequence %d alone vs in the padded batch" % b)
            assert float(ped[b, :, n:].abs().max() if n < 30 else 0.0) == 0.0           # padding pedestrians: aoe = foe = mask = 0


def _fp32_fp64_distance(T, gold, gold_eval, ds):
    """d per quantity: the sampling torch graph in float32 against float64 on the CPU, golden sequences, golden draws."""
    m32, m64 = _model(gold).eval(), _model(gold).double().eval()
    d = {k: 0.0 for k in ("loss", "aoe_sum", "foe_sum") + tuple("agg_" + k for k in AGG)}
    rows = {32: [], 64: []}
    for it in ITEMS:
        item = [t.unsqueeze(0) for t in ds[it]]
        nz = torch.from_numpy(gold_eval["test%d_noise" % it])
        a = T.test_sequence(m32, item, nz, "cpu")
        b = T.test_sequence(m64, [t.double() for t in item], nz.double(), "cpu")
        for k, x, y in zip(("loss", "aoe_sum", "foe_sum"), a, b):
            d[k] = max(d[k], float((x.double() - y).abs().max()))
        ra = T._test_row(a[0].view(1, -1), a[1].view(1, -1), a[2].view(1, -1), a[3].view(1))[0].double()
        rb = T._test_row(b[0].view(1, -1), b[1].view(1, -1), b[2].view(1, -1), b[3].view(1))[0].double()
        for i, k in enumerate(AGG):
            d["agg_" + k] = max(d["agg_" + k], float((ra[i] - rb[i]).abs()))
    return d


def test_test_mode_matches_the_reference_with_its_recorded_draws(gold, gold_eval, data_dir):
    """Sequences 0, 41, 77, S = 20, the draws the reference consumed: per-sample loss / aoe sum / foe sum, the per-sequence aggregates and the
    pass's seven numbers.  Bar per quantity max(2e-5, 4 d), d measured here on the CPU graph (float32 vs float64) and printed; measured
    d = 4.6e-8 / 4.5e-6 / 5.4e-6 for the per-sample loss / aoe sum / foe sum (bars 2e-5 / 2e-5 / 2.16e-5) and 1.7e-8 .. 2.0e-6 for the seven
    aggregates (bars 2e-5).  The std and min aggregates of a sequence are sums over its pedestrians and are compared at their bar times the number
    of fully present pedestrians.  Measured on the MI355X against the reference: 6.7e-8 (loss), 3.8e-6 (aoe sum), 3.8e-6 (foe sum), 1.2e-7 (Gaussian
    parameters, reported only), <= 1.9e-6 (per-sequence aggregates), <= 7.6e-8 (the pass's seven numbers)."""
    from crowdnav_prediction_attngraph_amd import gst_train as T
    ds = T.TrajectoriesDataset(data_dir)
    d = _fp32_fp64_distance(T, gold, gold_eval, ds)
    bar = {k: max(BAR, 4.0 * v) for k, v in d.items()}
    for k in d:
        print("test mode %-14s d = %.3e  bar = %.3e" % (k, d[k], bar[k]))
    model = _model(gold).cuda()
    ev = T.HipGstEvaluator(model)
    items = [ds[it] for it in ITEMS]
    draws = [torch.from_numpy(gold_eval["test%d_noise" % it]) for it in ITEMS]
    seq, ped, gauss = ev.evaluate_batch([i[6] for i in items], [i[8] for i in items], [i[4] for i in items], draws)
    rows = T._test_row(seq[:, :, 0] / seq[:, :, 1], seq[:, :, 2], seq[:, :, 3], ped[:, 0, :, 2].sum(1)).cpu().numpy()
    seq = seq.cpu().numpy()
    errs = {}
    for b, it in enumerate(ITEMS):
        m = float(gold_eval["test%d_m" % it])
        assert rows[b, 7] == m
        errs[(it, "loss")] = (np.abs(seq[b, :, 0] / seq[b, :, 1] - gold_eval["test%d_loss" % it]).max(), bar["loss"])
        errs[(it, "aoe_sum")] = (np.abs(seq[b, :, 2] - gold_eval["test%d_aoe_sum" % it]).max(), bar["aoe_sum"])
        errs[(it, "foe_sum")] = (np.abs(seq[b, :, 3] - gold_eval["test%d_foe_sum" % it]).max(), bar["foe_sum"])
        n = gold_eval["test%d_gauss" % it].shape[2]
        errs[(it, "gauss")] = (np.abs(gauss[b, :, :, :n].cpu().numpy() - gold_eval["test%d_gauss" % it]).max(), None)
        for i, k in enumerate(AGG):
            scale = m if k.endswith(("_std", "_min")) else 1.0
            errs[(it, "agg_" + k)] = (abs(float(rows[b, i]) - float(gold_eval["test%d_agg_%s" % (it, k)])), bar["agg_" + k] * scale)
    seven = T.test(model, _loader(ds, ITEMS), "cuda", num_samples=20, backend="hip", draws=draws)
    for i, k in enumerate(("loss", "aoe_mean", "foe_mean", "aoe_std", "foe_std", "aoe_min", "foe_min")):
        errs[("seven", k)] = (abs(seven[i] - float(gold_eval["test_seven"][i])), bar["agg_" + k])
    for k, (e, b) in errs.items():
        print("test mode vs reference %-22s err = %.3e  bar = %s" % (k, e, "%.3e" % b if b is not None else "(reported)"))
    bad = {k: v for k, v in errs.items() if v[1] is not None and not v[0] <= v[1]}
    assert not bad, bad


@pytest.mark.parametrize("S", [1, 20])
@pytest.mark.parametrize("B,N,seed", CASES)
def test_test_mode_equals_the_torch_graph_with_the_same_draws(B, N, seed, S):
    from crowdnav_prediction_attngraph_amd import gst_train as T
    model, lm, v_obs, v_pred, g = _ragged(B, N, seed)
    noise = torch.randn(B, S, 5, N, 2, generator=g)
    ev = T.HipGstEvaluator(model)
    hip = ev.evaluate_batch(v_obs, v_pred, lm, noise)
    assert tuple(hip[0].shape) == (B, S, 4) and tuple(hip[1].shape) == (B, S, N, 3) and tuple(hip[2].shape) == (B, S, 5, N, 5)
    if B * S <= 80:      # (the torch graph runs one decode at a time: the largest case is checked on a slice)
        _compare(hip, _torch_rows(T, model, lm, v_obs, v_pred, noise), "test mode B=%d N=%d S=%d" % (B, N, S))
    else:
        sl = slice(0, B, 8)
        _compare(tuple(t[sl] for t in hip), _torch_rows(T, model, lm[sl], v_obs[sl], v_pred[sl], noise[sl]), "test mode B=%d N=%d S=%d (every 8th sequence)" % (B, N, S))
    if S == 1:           # zero draws: the sample is the mean, on the same kernel path -> validation mode's bits
        zero = ev.evaluate_batch(v_obs, v_pred, lm, torch.zeros(B, 1, 5, N, 2))
        val = ev.evaluate_batch(v_obs, v_pred, lm)
        assert all(torch.equal(a, b) for a, b in zip(zero, val))


def test_the_observed_period_is_shared_by_the_samples_of_a_sequence():
    from crowdnav_prediction_attngraph_amd import gst_train as T
    model, lm, v_obs, v_pred, g = _ragged(3, 20, 5)
    noise = torch.randn(3, 1, 5, 20, 2, generator=g).expand(3, 20, 5, 20, 2).contiguous()
    seq, ped, gauss = T.HipGstEvaluator(model).evaluate_batch(v_obs, v_pred, lm, noise)
    for t in (seq, ped, gauss):
        assert torch.equal(t, t[:, :1].expand_as(t))
    other = T.HipGstEvaluator(model).evaluate_batch(v_obs, v_pred, lm, torch.randn(3, 20, 5, 20, 2, generator=g))[0]
    assert not torch.equal(other[:, 0], other[:, 1])


def test_evaluate_test_and_train_through_the_interface(gold, gold_eval, data_dir, tmp_path):
    from crowdnav_prediction_attngraph_amd import gst_train as T
    model = _model(gold).cuda()
    ds, dv = T.TrajectoriesDataset(data_dir), T.TrajectoriesDataset(data_dir, mode="val")
    a, b = T.evaluate(model, _loader(dv), "cuda", backend="hip", batch_size=5), T.evaluate(model, _loader(dv), "cuda", backend="torch")
    assert T.evaluate(model, _loader(dv), "cuda") == b
    for x, y, bar in zip(a, b, (BAR, BAR_OE, BAR_OE)):
        assert abs(x - y) <= bar, (a, b)
    d = _fp32_fp64_distance(T, gold, gold_eval, ds)
    bars = [max(BAR, 4.0 * d["agg_" + k]) for k in ("loss", "aoe_mean", "foe_mean", "aoe_std", "foe_std", "aoe_min", "foe_min")]
    a, b = T.test(model, _loader(ds), "cuda", seed=3, batch_size=16), T.test(model, _loader(ds), "cuda", seed=3, backend="torch")
    print("test() hip   %s\ntest() torch %s\nbars         %s" % (a, b, bars))
    for x, y, bar in zip(a, b, bars):
        assert abs(x - y) <= bar, (a, b, bars)
    # training with the validation on the device: the same weights bit for bit, the validation columns within the bars
    runs = []
    for name, vb in (("hip", None), ("torch", "torch")):
        m, hist = T.train(data_dir, str(tmp_path / name), num_epochs=3, temp_epochs=4, save_epochs=3, device="cuda", log=lambda s: None, backend="hip", val_backend=vb)
        runs.append(({k: v.clone() for k, v in m.state_dict().items()}, hist))
    for k, v in runs[0][0].items():
        assert torch.equal(v, runs[1][0][k]), k
    for col, bar in (("loss", BAR), ("aoe", BAR_OE), ("foe", BAR_OE)):
        x, y = np.array(runs[0][1]["val_%s_task" % col]), np.array(runs[1][1]["val_%s_task" % col])
        assert len(x) == 3 and np.abs(x - y).max() <= bar * max(1.0, np.abs(y).max()), (col, x, y)
        assert runs[0][1]["train_%s_task" % col] == runs[1][1]["train_%s_task" % col]


def test_a_sequence_of_more_than_64_pedestrians_takes_the_op_graph_inside_a_batch():
    """Three sequences of 5, 65 and 4 pedestrians (ragged presence) at batch_size = 2: the second takes the op-graph detour while the first is
    pending, the third sits at the padding floor of four pedestrians.  The pass returns one row per sequence, the detour's ahead of the batch that was
    pending (every row against the op graph's row of the same sequence, whose losses lie far apart); the detour's row has the op graph's own bits; validation and test(2 samples, recorded
    draws) agree with the torch backend at the ragged-batch bars (loss 2e-5, offset errors 1.5e-4)."""
    from crowdnav_prediction_attngraph_amd import gst_train as T
    sizes, items, model = (5, 65, 4), [], None
    for i, n in enumerate(sizes):
        mdl, lm, v_obs, v_pred, g = _ragged(1, n, 20 + i)
        model = model or mdl
        am = (lm[0].t().unsqueeze(2) * lm[0].t().unsqueeze(1)).unsqueeze(0)
        item = [None] * 12
        item[4], item[6], item[8], item[10], item[11] = lm, v_obs, v_pred, am[:, :5], am[:, 5:]
        items.append(item)
    draws = [torch.randn(2, 5, n, 2, generator=g) for n in sizes]
    seqs = lambda: ((it[6].shape[2], it) for it in items)     # noqa: E731
    for what, row, draw in (("validation", T._val_row, None), ("test", T._test_row, lambda n, d=iter(draws): next(d))):
        hip = T._eval_pass(model, seqs(), "cuda", row, T.HipGstEvaluator(model), 2, draw)
        assert hip.shape[0] == 3, what
        hip = hip[[1, 0, 2]]                                  # entry order: the detour, then the batch of the first and the third sequence
        ref = T._eval_pass(model, seqs(), "cuda", row, None, 2, None if draw is None else (lambda n, d=iter(draws): next(d)))
        assert hip.shape == ref.shape == (3, 4 if draw is None else 8), what
        m = [float((it[4].sum(2) == 10).sum()) for it in items]
        assert list(hip[:, -1]) == m and list(ref[:, -1]) == m and abs(hip[0, 0] - hip[2, 0]) > 100 * BAR, (what, m, hip)
        assert np.array_equal(hip[1], ref[1]), what + ": the detour is the op graph"
        _close(torch.from_numpy(hip[:, 0]), torch.from_numpy(ref[:, 0]), BAR, what + " rows: loss")
        _close(torch.from_numpy(hip[:, 1:-1]), torch.from_numpy(ref[:, 1:-1]), BAR_OE, what + " rows: sums of aoe / foe")
    a, b = T.evaluate(model, items, "cuda", backend="hip", batch_size=2), T.evaluate(model, items, "cuda", backend="torch")
    for x, y, bar in zip(a, b, (BAR, BAR_OE, BAR_OE)):
        assert abs(x - y) <= bar, (a, b)
    a, b = (T.test(model, items, "cuda", num_samples=2, backend=be, batch_size=2, draws=draws) for be in ("hip", "torch"))
    for x, y, bar in zip(a, b, (BAR,) + (BAR_OE,) * 6):
        assert abs(x - y) <= bar, (a, b)


def test_bad_arguments_are_refused_with_a_message_and_launch_nothing(gold):
    from crowdnav_prediction_attngraph_amd import _abi as A
    from crowdnav_prediction_attngraph_amd import gst_train as T
    model = _model(gold).cuda()
    ev = T.HipGstEvaluator(model)
    w = A.GstWeights()
    for (field, _), p in zip(A.GST_WEIGHT_KEYS, ev._params()):
        setattr(w, field, p.data_ptr())
    L = A.lib()
    B, N, S = 2, 8, 3
    vo, vp, lm, nz = torch.zeros(B, 5, 64, 2).cuda(), torch.zeros(B, 5, 64, 2).cuda(), torch.ones(B, 64, 10).cuda(), torch.zeros(B, 64, 5, 64, 2).cuda()
    ws = torch.empty(int(L.cn_gst_eval_workspace_bytes(B, 64, 64)), dtype=torch.uint8, device="cuda")
    seq = torch.full((B, 64, 4), -7.0).cuda()

    def call(N, S, noise, ws_bytes):
        torch.cuda.synchronize()
        rc = L.cn_gst_eval_step(B, N, S, A.ptr(vo), A.ptr(vp), A.ptr(lm), C.byref(w), A.ptr(noise), C.c_void_p(ws.data_ptr()), ws_bytes, A.ptr(seq), None, None, A.stream_ptr())
        torch.cuda.synchronize()
        return rc, L.cn_last_error().decode()

    assert L.cn_gst_eval_workspace_bytes(B, 65, 0) == 0 and L.cn_gst_eval_workspace_bytes(B, N, 65) == 0 and L.cn_gst_eval_workspace_bytes(B, 3, 0) == 0
    for args, word in (((65, 0, None, ws.numel()), "N=65"), ((N, 65, nz, ws.numel()), "S=65"), ((N, S, None, ws.numel()), "noise"),
                       ((N, S, nz, int(L.cn_gst_eval_workspace_bytes(B, N, S)) - 1), "workspace")):
        rc, msg = call(*args)
        assert rc != 0 and word in msg, (args[:2], rc, msg)
    assert float(seq.min()) == -7.0 and float(seq.max()) == -7.0          # nothing ran
    rc, msg = call(N, S, nz, int(L.cn_gst_eval_workspace_bytes(B, N, S)))
    assert rc == 0, msg
    with pytest.raises(A.CnError):
        ev.evaluate_batch(torch.zeros(1, 5, 65, 2), torch.zeros(1, 5, 65, 2), torch.ones(1, 65, 10))
    with pytest.raises(A.CnError):
        T.HipGstEvaluator(_model(gold))                                   # a CPU model: no fallback
