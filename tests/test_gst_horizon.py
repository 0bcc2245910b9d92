"""No GPU: the prediction horizon P = pred_seq_len = sim.predict_steps of the GST path.  The refusals outside the device box (P in 1 .. 8, five
observed frames) are raised in Python before anything is allocated; a run directory's pred_seq_len reaches the predictor that is loaded from it;
and the cases of tests/test_gpu_gst_horizon*.py reach what they are in the tables for."""
import argparse
import json
import os
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from crowdnav_prediction_attngraph_amd import _abi as A  # noqa: E402
from crowdnav_prediction_attngraph_amd import gst as G  # noqa: E402
from tests import gst_horizon_util as HU  # noqa: E402
from tests import gst_shape_util as U  # noqa: E402


@pytest.mark.parametrize("P", [0, 9, -1, 2.5])
def test_a_horizon_outside_the_box_is_refused_in_python_and_names_the_box(P):
    from crowdnav_prediction_attngraph_amd.gst_data import DeviceTrajectories
    from crowdnav_prediction_attngraph_amd.gst_hip import HipGST
    with pytest.raises(NotImplementedError, match=r"prediction horizon .* in \[1, 8\]"):
        A.gst_horizon(P)
    with pytest.raises(NotImplementedError, match=r"in \[1, 8\]"):
        HipGST(8, 4, pred_steps=P)                        # before the library, the device or a handle is touched
    with pytest.raises(NotImplementedError, match=r"in \[1, 8\]"):
        DeviceTrajectories.from_log(None, pred_seq_len=P)
    if P == int(P):
        with pytest.raises(NotImplementedError, match=r"in \[1, 8\]"):
            G.PretextProcessor(G.GSTPredictor(5, int(P)), 4, 8, int(P), 0.3, 0.3, -20.0, "cpu", use_hip=True)


def test_the_box_holds_one_to_eight_and_five_observed_frames():
    assert [A.gst_horizon(P) for P in range(1, 9)] == list(range(1, 9)) and A.CN_MAX_PRED == 8
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "crowdnav_hip.h")).read()
    assert "#define CN_MAX_PRED %d" % A.CN_MAX_PRED in hdr
    with pytest.raises(NotImplementedError, match="observed length of 6"):
        A.gst_horizon(5, obs_len=6)
    with pytest.raises(NotImplementedError, match="observed length of 6"):
        G.PretextProcessor(G.GSTPredictor(6, 3), 4, 8, 3, 0.3, 0.3, -20.0, "cpu", use_hip=True)


def test_predictor_and_env_must_agree_on_the_horizon():
    with pytest.raises(ValueError, match=r"pred_len = 5 .*predict_steps is 3"):
        G.PretextProcessor(G.GSTPredictor(), 4, 8, 3, 0.3, 0.3, -20.0, "cpu", use_hip=False)
    w = G.PretextProcessor(G.GSTPredictor(5, 3), 4, 8, 3, 0.3, 0.3, -20.0, "cpu", use_hip=False)
    assert w.P == 3 and w.hip is None


def _run_dir(tmp_path, name, P=None, how=None):
    d = tmp_path / name / "checkpoint"
    d.mkdir(parents=True)
    torch.manual_seed(3)
    m = G.GSTPredictor(5, P or 5)
    torch.save({"epoch": 2, "model_state_dict": m.state_dict()}, str(d / "epoch_2.pt"))
    args = dict(num_epochs=2, obs_seq_len=5, pred_seq_len=P)
    if how == "json":
        with open(str(d / "args.json"), "w") as f:
            json.dump(args, f)
    if how == "pickle":
        with open(str(d / "args.pickle"), "wb") as f:
            pickle.dump(argparse.Namespace(**args), f)
    return str(tmp_path / name), m


@pytest.mark.parametrize("how,P,want", [("json", 3, 3), ("pickle", 8, 8), (None, None, 5), ("json", None, 5)])
def test_from_checkpoint_reads_the_horizon_the_run_recorded(tmp_path, how, P, want):
    run, m = _run_dir(tmp_path, "run", P, how)
    path = G.find_checkpoint(run)
    assert os.path.basename(path) == "epoch_2.pt"
    got = G.GSTPredictor.from_checkpoint(path, "cpu")
    assert (got.obs_len, got.pred_len) == (5, want)
    for (k, a), (_, b) in zip(m.state_dict().items(), got.state_dict().items()):
        assert torch.equal(a, b), k
    cfg = argparse.Namespace(pred=argparse.Namespace(model_dir=run))
    assert G.load_predictor(cfg, "cpu").pred_len == want
    E, H = 3, 4
    out, om = got(torch.zeros(E, H, 5, 2), torch.ones(E, H, 5, 1))
    assert tuple(out.shape) == (E, H, want, 5) and tuple(om.shape) == (E, H, 1)


def test_an_args_pickle_of_anything_but_a_namespace_is_not_loaded(tmp_path):
    run, _ = _run_dir(tmp_path, "run", 3, None)
    with open(os.path.join(run, "checkpoint", "args.pickle"), "wb") as f:
        pickle.dump({"pred_seq_len": 3, "fn": os.getcwd}, f)
    with pytest.warns(UserWarning, match="pred_seq_len is taken as 5"):
        assert G.run_pred_seq_len(os.path.join(run, "checkpoint")) == 5
    # a file that cannot be read is not a five-step run: it raises
    with open(os.path.join(run, "checkpoint", "args.pickle"), "wb") as f:
        f.write(pickle.dumps(argparse.Namespace(pred_seq_len=3, num_epochs=2))[:-9])
    with pytest.raises((pickle.UnpicklingError, EOFError)):
        G.run_pred_seq_len(os.path.join(run, "checkpoint"))


def test_train_records_the_horizon_and_the_run_loads_with_it(tmp_path):
    from crowdnav_prediction_attngraph_amd import gst_train as T
    from tests import gst_data_util as D
    dirs = D.write_files(HU.hand_made_log()[:, :1], tmp_path / "data")
    model, hist = T.train(dirs[0], str(tmp_path / "run"), num_epochs=1, temp_epochs=4, save_epochs=1, device="cpu", log=lambda s: None, backend="torch",
                          pred_seq_len=3)
    assert model.pred_len == 3 and np.isfinite(hist["train_loss_task"]).all()
    with open(str(tmp_path / "run" / "checkpoint" / "args.json")) as f:
        assert json.load(f)["pred_seq_len"] == 3
    assert G.load_predictor(argparse.Namespace(pred=argparse.Namespace(model_dir=str(tmp_path / "run"))), "cpu").pred_len == 3
    val, t = T.eval_run(str(tmp_path / "run"), dirs[0], num_samples=2, device="cpu", backend="torch", log=lambda s: None)
    assert np.isfinite(val).all() and np.isfinite(t).all()
    with pytest.raises(NotImplementedError, match=r"in \[1, 8\]"):
        T.train(dirs[0], str(tmp_path / "run9"), num_epochs=1, device="cpu", log=lambda s: None, backend="hip", pred_seq_len=9)
    assert not os.path.exists(str(tmp_path / "run9"))


def test_trainer_names_the_edge_width_of_eight_steps_with_the_attention_policy():
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd.trainer import train
    cfg = C.non_randomized(**{"sim.human_num": 8, "sim.predict_method": "inferred", "sim.predict_steps": 8})
    with pytest.raises(NotImplementedError, match=r"predict_steps = 8 .* width 18, .* at most 16"):
        train("CrowdSimPredRealGST-v0", num_processes=8, num_steps=6, num_updates=1, config=cfg, log=None, device="cpu")


# ---- what the GPU cases reach ----
@pytest.mark.parametrize("case", list(HU.PREDICT_CASES), ids=["x".join(map(str, c)) for c in HU.PREDICT_CASES])
def test_predict_cases_reach_what_they_are_in_the_table_for(case):
    assert HU.PREDICT_CASES[case](U.launch_plan(*case)), {k: v for k, v in U.launch_plan(*case).items() if not callable(v)}


@pytest.mark.parametrize("P", HU.HORIZONS)
def test_wrapper_stream_of_a_horizon_is_the_stream_at_another_edge_width(P):
    E, H, _ = HU.WRAPPER_CASE
    a, b = U.wrapper_stream(E, H, U.WRAPPER_STEPS, HU.WRAPPER_SEED), HU.wrapper_stream(E, H, U.WRAPPER_STEPS, HU.WRAPPER_SEED, P)
    assert U.key_condition(b)[0] == 0
    for o, w in zip(a, b):
        assert w["spatial_edges"].shape == (E, H, 2 * (P + 1)) and np.array_equal(o["spatial_edges"][:, :, :2], w["spatial_edges"][:, :, :2])
        assert all(w[k] is o[k] for k in ("robot_node", "visible_masks", "rews_in"))
        assert (w["spatial_edges"][~w["visible_masks"]] == 15.0).all() and len(np.unique(w["spatial_edges"][2, :, 2:])) == 2 * P * H


@pytest.mark.parametrize("H", HU.CV_SIZES)
@pytest.mark.parametrize("P", HU.HORIZONS)
def test_constant_velocity_streams_reach_every_horizon_and_leave_no_env_out(P, H):
    seen, violations, kept = HU.cv_plan(H, P)
    assert seen == set(range(-1, P)), seen
    assert violations == 0
    assert kept > 0                                        # rows that keep their input columns 2 .. 2P+1


@pytest.mark.parametrize("H", HU.CV_SIZES)
def test_the_restated_stream_is_the_existing_one_at_five_steps(H):
    """Seven envs, the same positions, markers, visibility and rewards; env 6's pair arrives at horizons 3 and 1 (one human at horizon 2 at H = 1)."""
    a, b = U.cv_stream(H), HU.cv_stream(H, 5)
    assert len(a) == len(b) == 6 and HU.cv_plan(H, 5)[0] == {-1, 0, 1, 2, 3, 4}
    for o, w in zip(a, b):
        for k in ("robot_node", "spatial_edges", "visible_masks", "rews_in"):
            assert o[k].shape == w[k].shape and np.array_equal(o[k], w[k]), k


def test_the_restated_closed_form_is_the_existing_one_at_five_steps():
    H = 21
    hist = U.History(7, H)
    for o in U.cv_stream(H):
        hist.push(o)
        for a, b in zip(U.cv_expected(hist, o), HU.cv_expected(hist, o, 5)):
            assert np.array_equal(a, b)


def test_the_host_wrapper_follows_the_closed_form_at_every_horizon():
    """The torch-op statement of the wrapper (what CPU tensors run) over the restated stream: the closed form is what the wrapper computes."""
    H = 21
    for P in HU.HORIZONS:
        m = U.const_velocity_predictor(HU.model(100 + H, P), *HU.CV_V)
        w = G.PretextProcessor(m, P + 2, H, P, 0.3, 0.3, HU.PENALTY, torch.device("cpu"), use_hip=False)
        hist = U.History(P + 2, H)
        for o in HU.cv_stream(H, P):
            obs = {k: torch.from_numpy(np.array(o[k])) for k in ("robot_node", "spatial_edges", "visible_masks")}
            se, rews = w.process(obs, torch.from_numpy(o["rews_in"].copy()))
            hist.push(o)
            want_se, want_r, _ = HU.cv_expected(hist, o, P)
            assert np.array_equal(se.numpy()[:, :, :2], want_se[:, :, :2])
            assert np.abs(se.numpy() - want_se).max() <= 1e-6 and np.abs(rews.numpy() - want_r).max() <= 1e-6


# ---- the reference's own numbers at 3 and 8 predicted steps (tests/golden/make_golden_gst_horizon.py) ----
@pytest.mark.parametrize("P", HU.GOLDEN_HORIZONS)
def test_host_mirror_reproduces_the_reference_at_a_horizon(P):
    """Interface forward of 4 envs within 1e-4 and one training step on 4 sequences (loss and Gaussian parameters within 5e-5, every gradient
    within 5e-5 x max(1, its largest entry)): the bars of the P = 5 goldens (tests/test_gst_host.py, tests/test_gst_train.py)."""
    from crowdnav_prediction_attngraph_amd import gst_train as T
    z, m = HU.golden(P)
    out, mask = m(torch.from_numpy(z["in_traj"]), torch.from_numpy(z["in_mask"]))
    np.testing.assert_array_equal(mask.numpy(), z["out_mask"])
    valid = z["out_mask"][..., 0] > 0
    assert out.shape == z["out_traj"].shape == (4, 8, P, 5) and 0 < valid.sum() < valid.size
    np.testing.assert_allclose(out.numpy()[valid], z["out_traj"][valid], rtol=0, atol=1e-4)
    assert np.all(out.numpy()[~valid][..., :2] == -999.0)
    lm, v_obs, v_pred = (torch.from_numpy(z[k]) for k in ("loss_mask_rel", "v_obs", "v_pred"))
    m.zero_grad()
    num, den, gps = 0.0, 0.0, []
    for b in range(lm.shape[0]):
        l1 = lm[b:b + 1]
        am = (l1[0].t().unsqueeze(2) * l1[0].t().unsqueeze(1))[:5].unsqueeze(0)
        gp, xs, info = T.forward_train(m, v_obs[b:b + 1], am, l1, 0.0)
        pl, elm = T.negative_log_likelihood_full_partial(gp, v_pred[b:b + 1], info["loss_mask_rel_full_partial"], l1[:, :, 5:])
        num, den = num + pl.sum(), den + elm.sum()
        gps.append(torch.cat(gp, -1)[0].detach().numpy())
    loss = num / den
    loss.backward()
    assert float(den) == float(z["count"]) and abs(float(loss) - float(z["loss"])) <= 5e-5
    np.testing.assert_allclose(np.stack(gps), z["gauss"], rtol=0, atol=5e-5)
    for k, p in m.named_parameters():
        ref = z["grad_" + k]
        assert float(np.abs(p.grad.numpy() - ref).max()) <= 5e-5 * max(1.0, float(np.abs(ref).max())), k
