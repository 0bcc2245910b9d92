"""GST evaluation path on the CPU op graph: validation (gst_train.evaluate) unchanged, the sampling variant of forward_train, and the test
protocol (gst_train.test) against the reference's own numbers (tests/golden/gst_eval_h20.npz, made by tests/golden/make_golden_gst_eval.py from
the reference's st_model / negative_log_likelihood_full_partial / average_offset_error / final_offset_error driven like eval.py's `inference`,
with the standard-normal draws the reference consumed recorded in the file)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gst_train import GOLDEN, ITEMS, _model  # noqa: E402

BAR = 2e-5          # the project's bar of the CPU graph against the reference (tests/test_gst_train.py)
SEVEN = ("loss", "aoe_mean", "foe_mean", "aoe_std", "foe_std", "aoe_min", "foe_min")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "gst_train_h20.npz"))


@pytest.fixture(scope="module")
def gold_eval():
    return np.load(os.path.join(GOLDEN, "gst_eval_h20.npz"))


@pytest.fixture(scope="module")
def data_dir(gold, tmp_path_factory):
    d = tmp_path_factory.mktemp("gstds_eval")
    with open(str(d / "0.txt"), "w") as f:
        f.write(str(gold["file_lines"]) + "\n")
    return str(d)


def _loader(ds, idx=None):
    from torch.utils.data import DataLoader, Subset
    return DataLoader(ds if idx is None else Subset(ds, list(idx)), batch_size=1, shuffle=False)


def _parent_evaluate(T, model, loader, device):
    """gst_train.evaluate as it stood before the backend argument existed, statement for statement."""
    model.eval()
    losses, aoes, foes, ms = [], [], [], []
    with torch.no_grad():
        for item in loader:
            if item[6].shape[2] > 128:
                continue
            loss, gp, xs, info, v_pred_gt = T.sequence_loss(model, item, device, 0.0)
            lm = info["loss_mask_per_pedestrian"]
            losses.append(loss.item())
            aoes.append(T.average_offset_error(xs, v_pred_gt, lm).cpu().numpy()); foes.append(T.final_offset_error(xs, v_pred_gt, lm).cpu().numpy())
            ms.append(lm[0].cpu().numpy())
    m = max(float(np.concatenate(ms).sum()), 1.0)
    return float(np.mean(losses)), float(np.concatenate(aoes).sum() / m), float(np.concatenate(foes).sum() / m)


def test_validation_pass_on_the_op_graph_is_unchanged_and_matches_the_reference(gold, gold_eval, data_dir):
    from crowdnav_prediction_attngraph_amd import gst_train as T
    ds = T.TrajectoriesDataset(data_dir, mode="val")
    assert len(ds) == int(gold_eval["val_num_seq"]) and np.array_equal(np.array(ds.frame_id_seq), gold_eval["val_frame_id_seq"])
    model = _model(gold)
    parent = _parent_evaluate(T, model, _loader(ds), "cpu")
    assert T.evaluate(model, _loader(ds), "cpu") == parent
    assert T.evaluate(model, _loader(ds), "cpu", backend="torch") == parent
    np.testing.assert_allclose(parent, gold_eval["val_triple"], rtol=0, atol=BAR)
    with pytest.raises(ValueError):
        T.evaluate(model, _loader(ds), "cpu", backend="triton")


def test_forward_without_noise_is_the_mean_fed_decode_and_zero_noise_equals_it(gold, data_dir):
    from crowdnav_prediction_attngraph_amd import gst_train as T
    ds = T.TrajectoriesDataset(data_dir)
    model = _model(gold)
    model.eval()
    with torch.no_grad():
        for it in ITEMS:
            item = [t.unsqueeze(0) for t in ds[it]]
            loss, gp, xs, info, v_pred_gt = T.sequence_loss(model, item, "cpu", 0.0)
            assert abs(loss.item() - float(gold["item%d_loss" % it])) <= BAR
            for n, t in zip(("mu", "sx", "sy", "corr"), gp):
                np.testing.assert_allclose(t.numpy(), gold["item%d_%s" % (it, n)], rtol=0, atol=BAR)
            loss_n, gp_n, xs_n = T.sequence_loss(model, item, "cpu", 0.0, noise=None)[:3]
            loss_z, gp_z, xs_z = T.sequence_loss(model, item, "cpu", 0.0, noise=torch.zeros(1, 5, item[6].shape[2], 2))[:3]
            for a, b, c in zip((loss, xs) + tuple(gp), (loss_n, xs_n) + tuple(gp_n), (loss_z, xs_z) + tuple(gp_z)):
                assert torch.equal(a, b) and torch.equal(a, c)


def test_sampled_test_protocol_on_the_op_graph_matches_the_reference(gold, gold_eval, data_dir):
    """Per-sample loss, Gaussian parameters, aoe sum and foe sum of sequences 0, 41, 77 with the reference's recorded draws, the per-sequence
    aggregates and the pass's seven numbers through gst_train.test(draws=...)."""
    from crowdnav_prediction_attngraph_amd import gst_train as T
    ds = T.TrajectoriesDataset(data_dir)
    model = _model(gold)
    model.eval()
    S = int(gold_eval["samples"])
    assert tuple(gold_eval["items"]) == ITEMS and S == 20
    for it in ITEMS:
        item = [t.unsqueeze(0) for t in ds[it]]
        noise = torch.from_numpy(gold_eval["test%d_noise" % it])
        assert tuple(noise.shape) == (S, 5, item[6].shape[2], 2)
        loss, aoe, foe, m = T.test_sequence(model, item, noise, "cpu")
        assert float(m) == float(gold_eval["test%d_m" % it])
        np.testing.assert_allclose(loss.numpy(), gold_eval["test%d_loss" % it], rtol=0, atol=BAR)
        np.testing.assert_allclose(aoe.numpy(), gold_eval["test%d_aoe_sum" % it], rtol=0, atol=BAR)
        np.testing.assert_allclose(foe.numpy(), gold_eval["test%d_foe_sum" % it], rtol=0, atol=BAR)
        with torch.no_grad():
            for s in (0, S - 1):
                gp = T.sequence_loss(model, item, "cpu", 0.0, noise[s:s + 1])[1]
                np.testing.assert_allclose(torch.cat(gp, -1)[0].numpy(), gold_eval["test%d_gauss" % it][s], rtol=0, atol=BAR)
        row = T._test_row(loss.view(1, -1), aoe.view(1, -1), foe.view(1, -1), m.view(1))[0].numpy()
        for k, v in zip(("loss", "aoe_mean", "aoe_std", "aoe_min", "foe_mean", "foe_std", "foe_min"), row):
            assert abs(float(v) - float(gold_eval["test%d_agg_%s" % (it, k)])) <= BAR, (it, k)
    seven = T.test(model, _loader(ds, ITEMS), "cpu", num_samples=S, backend="torch", draws=[torch.from_numpy(gold_eval["test%d_noise" % it]) for it in ITEMS])
    np.testing.assert_allclose(seven, gold_eval["test_seven"], rtol=0, atol=BAR)


def test_test_protocol_draws_come_from_the_seed_in_loader_order(gold, data_dir):
    from crowdnav_prediction_attngraph_amd import gst_train as T
    ds = T.TrajectoriesDataset(data_dir)
    model = _model(gold)
    a = T.test(model, _loader(ds, (3, 50)), "cpu", num_samples=4, seed=7)
    g = torch.Generator().manual_seed(7)
    draws = [torch.randn(4, 5, ds[i][6].shape[1], 2, generator=g) for i in (3, 50)]
    assert a == T.test(model, _loader(ds, (3, 50)), "cpu", num_samples=4, seed=99, draws=draws)
    assert a != T.test(model, _loader(ds, (3, 50)), "cpu", num_samples=4, seed=8) and len(a) == 7 and np.isfinite(a).all()


def test_eval_command_line_prints_the_reference_lines(gold, data_dir, tmp_path, capsys):
    from crowdnav_prediction_attngraph_amd import gst_train as T
    T.train(data_dir, str(tmp_path / "run"), num_epochs=1, temp_epochs=4, save_epochs=1, device="cpu", log=lambda s: None)
    T.main(["eval", str(tmp_path / "run"), data_dir, "--samples", "3", "--device", "cpu"])
    out = capsys.readouterr().out.splitlines()
    stored = float(out[1].split(":")[1])
    again = float(out[2].split(":")[1])
    assert out[1].startswith("Validation loss in the checkpoint") and out[2].startswith("Validation loss from loaded model") and stored == again
    assert out[3].startswith("Test loss from loaded model") and "test aoe std" in out[4] and "min foe" in out[4]
