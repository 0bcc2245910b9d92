"""The product's GST predictor + wrapper logic (torch ops; CPU here, the same code runs on the GPU) against the reference goldens."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from crowdnav_prediction_attngraph_amd.gst import GSTPredictor, PretextProcessor
from tests.golden_util import GOLDEN

sys.path.insert(0, GOLDEN)
from make_golden_gst import gst_formula_state_dict  # noqa: E402


def _model(meta, device="cpu"):
    sd = gst_formula_state_dict({k: tuple(v) for k, v in meta["shapes"].items()})
    m = GSTPredictor().to(device)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v)) for k, v in meta["shapes"].items()]  # checkpoint-compatible
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m


def _check(device, use_hip=False):
    z = np.load(os.path.join(GOLDEN, "gst_e4_h20.npz"))
    meta = json.loads(str(z["meta"]))
    m = _model(meta, device)
    for case in ("a", "b"):
        out, mask = m(torch.from_numpy(z["in_traj_" + case]).to(device), torch.from_numpy(z["in_mask_" + case]).to(device))
        np.testing.assert_array_equal(mask.cpu().numpy(), z["out_mask_" + case])
        valid = z["out_mask_" + case][..., 0] > 0
        np.testing.assert_allclose(out.cpu().numpy()[valid], z["out_traj_" + case][valid], rtol=0, atol=1e-4)
        assert np.all(out.cpu().numpy()[~valid][..., :2] == -999.0)
    E, H, T = meta["E"], meta["H"], meta["T"]
    w = PretextProcessor(m, E, H, 5, 0.3, 0.3, -20.0, torch.device(device), use_hip=use_hip)
    for t in range(T):
        obs = {"robot_node": torch.from_numpy(z["w_in_robot_node_%d" % t]).to(device), "spatial_edges": torch.from_numpy(z["w_in_spatial_edges_%d" % t]).to(device),
               "visible_masks": torch.from_numpy(z["w_in_visible_masks_%d" % t]).to(device)}
        se, rews = w.process(obs, torch.from_numpy(z["w_in_rews_%d" % t]).to(device))
        np.testing.assert_allclose(se.cpu().numpy(), z["w_out_spatial_edges_%d" % t], rtol=0, atol=1e-4, err_msg="edges @%d" % t)
        np.testing.assert_allclose(rews.cpu().numpy().reshape(E, 1), z["w_out_rews_%d" % t], atol=1e-5, err_msg="rews @%d" % t)


def test_gst_predictor_and_wrapper_match_reference_cpu():
    _check("cpu")


def test_inference_forward_is_the_training_graph_with_dropout_off():
    """GSTPredictor.forward is gst_train.forward_train(p_drop=0) on forward's own preprocessing, followed by its cumulative post-processing
    (both written out here), bit for bit: inference, training and test share one op graph, and a later edit cannot split them again unnoticed.
    E = 7 envs, H = 11 humans, 5 steps, about a quarter of the observations absent, weights drawn with normal std 0.3."""
    from crowdnav_prediction_attngraph_amd import gst_train as T
    E, H, Tn, INVALID = 7, 11, 5, -999.0
    g = torch.Generator().manual_seed(11)
    model = GSTPredictor()
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(0.3 * torch.randn(p.shape, generator=g))
    in_mask = (torch.rand(E, H, Tn, 1, generator=g) > 0.25).float()
    in_traj = torch.where(in_mask > 0, 3.0 * torch.randn(E, H, Tn, 2, generator=g), torch.full((E, H, Tn, 2), INVALID))
    out, out_mask = model(in_traj, in_mask)
    assert tuple(out.shape) == (E, H, 5, 5) and 0 < float(out_mask.mean()) < 1
    # crowd_nav_interface_parallel.py:76-78 in the dataset's layout: v_obs [E,T,H,2], attn_mask_obs [E,T,H,H] (neighbour, target), loss_mask_rel [E,H,T+P]
    m = in_mask[..., 0]
    m_rel = torch.cat([m[:, :, :1], m[:, :, :-1] * m[:, :, -1:]], dim=2)
    rel = torch.cat([torch.zeros(E, H, 1, 2), in_traj[:, :, 1:] - in_traj[:, :, :-1]], dim=2)
    rel = INVALID * (1 - m_rel.unsqueeze(-1)) + rel * m_rel.unsqueeze(-1)
    mt = m_rel.permute(0, 2, 1)
    with torch.no_grad():
        (mu, sx, sy, corr), xs, info = T.forward_train(model, rel.permute(0, 2, 1, 3), mt.unsqueeze(2) * mt.unsqueeze(3),
                                                       torch.cat([m_rel, torch.zeros(E, H, 5)], dim=2), p_drop=0.0)
    lm_fp = info["loss_mask_rel_full_partial"]
    assert torch.equal(lm_fp, m_rel[:, :, -1]) and torch.equal(xs, mu * lm_fp[:, None, :, None])
    # crowd_nav_interface_parallel.py:92-114: displacements to positions, the Gaussians of a sum of independent steps
    sxc, syc = (sx ** 2).cumsum(1).sqrt(), (sy ** 2).cumsum(1).sqrt()
    corrc = (corr * sx * sy).cumsum(1) / (sxc * syc)
    lm_pred = lm_fp[:, None, :, None]
    pos = (mu.cumsum(1) + in_traj[:, :, -1].unsqueeze(1)) * lm_pred + INVALID * (1 - lm_pred)
    want = torch.cat([pos, sxc, syc, corrc], dim=3).permute(0, 2, 1, 3)
    assert torch.equal(out, want) and torch.equal(out_mask, lm_fp.unsqueeze(-1))


def _save_as_numpy1(obj, path):
    """torch.save, with numpy scalars named as numpy 1.x pickled them (numpy.core.multiarray.scalar; numpy >= 2 writes numpy._core...),
    as in the checkpoints the reference ships.  Protocol-2 GLOBAL opcodes are newline-terminated text: the rename is a byte replacement."""
    import io
    import zipfile
    buf = io.BytesIO()
    torch.save(obj, buf)
    src = zipfile.ZipFile(io.BytesIO(buf.getvalue()))
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as dst:
        for info in src.infolist():
            data = src.read(info.filename)
            if info.filename.endswith("/data.pkl"):
                data = data.replace(b"cnumpy._core.multiarray\nscalar\n", b"cnumpy.core.multiarray\nscalar\n")
                assert b"cnumpy.core.multiarray\nscalar\n" in data
            dst.writestr(info.filename, data)


def test_reference_checkpoint_loads_when_available(tmp_path):
    """A checkpoint in the layout of the reference's shipped epoch_100.pt (the GST training script's dict: model / optimizer / scheduler
    state, numpy-scalar epoch metrics, date), holding the shipped weights (the w/ arrays of gst_real_e4_h20.npz), written here and loaded."""
    from collections import OrderedDict
    z = np.load(os.path.join(GOLDEN, "gst_real_e4_h20.npz"))
    keys = list(GSTPredictor().state_dict())
    sd = OrderedDict((k, torch.from_numpy(z["w/" + k].copy())) for k in keys)
    src = GSTPredictor()
    src.load_state_dict(sd)
    opt = torch.optim.Adam(src.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=10, gamma=0.1)
    ck = {"epoch": 100, "model_state_dict": sd, "optimizer_state_dict": opt.state_dict(), "lr_scheduler_state_dict": sched.state_dict(),
          "train_loss_epoch": np.float64(-5.0), "val_loss_epoch": np.float64(-3.5), "train_aoe_epoch": np.float32(5.5),
          "val_aoe_epoch": np.float32(5.0), "train_foe_epoch": np.float32(11.5), "val_foe_epoch": np.float32(10.5), "training_date": "211230"}
    path = str(tmp_path / "epoch_100.pt")
    _save_as_numpy1(ck, path)
    m = GSTPredictor.from_checkpoint(path, "cpu")
    assert sum(p.numel() for p in m.parameters()) == 67269   # SURVEY.md 8a-G3 [probed]
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k


@pytest.mark.gpu
def test_gst_torch_path_matches_reference_gpu():
    _check("cuda", use_hip=False)


@pytest.mark.gpu
def test_hip_gst_wrapper_matches_reference_golden():
    """cn_gst_wrapper_step (history ring, predictor kernels, social penalty, edge write-back, sort) on the reference's trace."""
    _check("cuda", use_hip=True)


@pytest.mark.gpu
def test_hip_gst_predict_matches_reference_golden_and_torch_path():
    from crowdnav_prediction_attngraph_amd.hip import HipGST
    z = np.load(os.path.join(GOLDEN, "gst_e4_h20.npz"))
    meta = json.loads(str(z["meta"]))
    m = _model(meta, "cuda")
    g = HipGST(20, 512)
    g.set_weights(m.state_dict())
    for case in ("a", "b"):
        out, mask = g.predict(torch.from_numpy(z["in_traj_" + case]).cuda(), torch.from_numpy(z["in_mask_" + case]).cuda())
        np.testing.assert_array_equal(mask.cpu().numpy(), z["out_mask_" + case])
        valid = z["out_mask_" + case][..., 0] > 0
        np.testing.assert_allclose(out.cpu().numpy()[valid], z["out_traj_" + case][valid], rtol=0, atol=1e-4)
        assert np.all(out.cpu().numpy()[~valid][..., :2] == -999.0)
    # larger ragged batch against the torch expression of the same model
    sys.path.insert(0, GOLDEN)
    from make_golden_gst import synth_traj
    traj, mask = synth_traj(300, 20, 7)
    t_d, m_d = torch.from_numpy(traj).cuda(), torch.from_numpy(mask).cuda()
    ref_out, ref_mask = m(t_d, m_d)
    out, om = g.predict(t_d, m_d)
    assert torch.equal(om, ref_mask)
    v = ref_mask[..., 0] > 0
    assert torch.allclose(out[v], ref_out[v], rtol=0, atol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("H,E", [(1, 70), (5, 301), (12, 130), (16, 97), (33, 41), (50, 23), (64, 17)])
def test_hip_gst_kernels_match_torch_expression_for_other_crowd_sizes(H, E):
    """The fused encoder-layer / LSTM kernels tile whole groups of H nodes (<= 80 rows per tile, ragged last tiles, padding rows):
    every group size class against the torch expression of the same model, seeded random weights."""
    from crowdnav_prediction_attngraph_amd.gst import GSTPredictor
    from crowdnav_prediction_attngraph_amd.hip import HipGST
    torch.manual_seed(100 + H)
    m = GSTPredictor().cuda()
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.5)
    g = HipGST(H, E)
    g.set_weights(m.state_dict())
    rs = np.random.RandomState(H)
    pos0 = rs.uniform(-6, 6, (E, H, 1, 2)); vel = rs.uniform(-0.3, 0.3, (E, H, 1, 2))
    traj = (pos0 + vel * np.arange(5).reshape(1, 1, 5, 1) + 0.02 * rs.standard_normal((E, H, 5, 2))).astype(np.float32)
    mask = (rs.uniform(size=(E, H, 5, 1)) > 0.3)
    mask[0] = True
    mask[-1] = False
    traj = np.where(mask, traj, -999.0).astype(np.float32)
    t_d, m_d = torch.from_numpy(traj).cuda(), torch.from_numpy(mask.astype(np.float32)).cuda()
    ref_out, ref_mask = m(t_d, m_d)
    out, om = g.predict(t_d, m_d)
    assert torch.equal(om, ref_mask)
    v = ref_mask[..., 0] > 0
    assert int(v.sum()) > 0 and torch.allclose(out[v], ref_out[v], rtol=0, atol=1e-4)
    assert bool((out[~v][..., :2] == -999.0).all())


@pytest.mark.gpu
def test_predrealgst_env_with_wrapper_steps_on_device():
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd.vec_env import make_vec_envs
    z = np.load(os.path.join(GOLDEN, "gst_e4_h20.npz"))
    meta = json.loads(str(z["meta"]))
    pred = _model(meta, "cuda")
    cfg = C.non_randomized(**{"sim.human_num": 20, "sim.predict_method": "inferred"})
    envs = make_vec_envs("CrowdSimPredRealGST-v0", 425, 32, 0.99, None, torch.device("cuda"), False, config=cfg, pretext_wrapper=True, predictor=pred)
    obs = envs.reset()
    assert obs["spatial_edges"].shape == (32, 20, 12)
    for t in range(12):
        obs, rew, done, infos = envs.step(torch.full((32, 2), 0.3, device="cuda"))
        se = obs["spatial_edges"]
        d = se[:, :, :2].norm(dim=-1)
        assert torch.all(d[:, 1:] >= d[:, :-1])               # sorted by current distance
        assert torch.isfinite(se).all() and rew.shape == (32, 1)
    envs.close()
    # and through the fused trainer loop
    from crowdnav_prediction_attngraph_amd.trainer import train
    import crowdnav_prediction_attngraph_amd.vec_env as V
    orig = V.make_vec_envs
    try:
        V_make = lambda *a, **k: orig(*a, **dict(k, pretext_wrapper=True, predictor=pred))  # noqa: E731
        import crowdnav_prediction_attngraph_amd.trainer as TR
        TR.make_vec_envs = V_make
        hist, _ = train("CrowdSimPredRealGST-v0", num_processes=16, num_steps=6, num_updates=1, config=cfg, log=None)
        assert np.isfinite(hist[0]["value_loss"])
    finally:
        TR.make_vec_envs = orig


def _real():
    z = np.load(os.path.join(GOLDEN, "gst_real_e4_h20.npz"))
    return z, {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}


def test_predictor_with_the_shipped_weights_matches_reference_cpu():
    z, sd = _real()
    m = GSTPredictor()
    m.load_state_dict(sd)
    for case in ("a", "b", "c"):
        out, mask = m(torch.from_numpy(z["in_traj_" + case]), torch.from_numpy(z["in_mask_" + case]))
        np.testing.assert_array_equal(mask.numpy(), z["out_mask_" + case])
        valid = z["out_mask_" + case][..., 0] > 0
        np.testing.assert_allclose(out.detach().numpy()[valid], z["out_traj_" + case][valid], rtol=0, atol=1e-4)


@pytest.mark.gpu
def test_hip_gst_predict_with_the_shipped_weights_matches_reference_golden():
    """cn_gst_predict with the reference's real epoch_100.pt weights (committed tensor fixture) against the reference's outputs."""
    from crowdnav_prediction_attngraph_amd.hip import HipGST
    z, sd = _real()
    g = HipGST(20, 64)
    g.set_weights({k: v.cuda() for k, v in sd.items()})
    for case in ("a", "b", "c"):
        out, mask = g.predict(torch.from_numpy(z["in_traj_" + case]).cuda(), torch.from_numpy(z["in_mask_" + case]).cuda())
        np.testing.assert_array_equal(mask.cpu().numpy(), z["out_mask_" + case])
        valid = z["out_mask_" + case][..., 0] > 0
        np.testing.assert_allclose(out.cpu().numpy()[valid], z["out_traj_" + case][valid], rtol=0, atol=1e-4)


@pytest.mark.gpu
def test_predrealgst_vec_env_resume_is_bit_exact():
    """state_dict() / load_state_dict() of a vec-env WITH the prediction wrapper: simulator snapshot + the wrapper's 5-step observation
    history (rl/vec_env/vec_pretext_normalize.py:85-101 traj_buffer / mask_buffer).  A run restored at step 17 continues exactly like the
    uninterrupted one: observations (predictions included), rewards (social penalty included), dones -- equal bit for bit over 25 steps."""
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd.vec_env import make_vec_envs
    z = np.load(os.path.join(GOLDEN, "gst_e4_h20.npz"))
    pred = _model(json.loads(str(z["meta"])), "cuda")
    cfg = C.non_randomized(**{"sim.human_num": 20, "sim.predict_method": "inferred"})
    E = 48
    mk = lambda: make_vec_envs("CrowdSimPredRealGST-v0", 425, E, 0.99, None, torch.device("cuda"), False, config=cfg, pretext_wrapper=True, predictor=pred)  # noqa: E731

    def act(t):
        g = torch.Generator(device="cuda").manual_seed(100 + t)
        return torch.randn(E, 2, device="cuda", generator=g) * 0.7

    a = mk()
    a.reset()
    for t in range(17):
        a.step(act(t))
    sd = a.state_dict()
    assert "pretext" in sd and tuple(sd["pretext"]["traj"].shape) == (5, E, 20, 2)
    want = [a.step(act(t)) for t in range(17, 42)]
    a.close()
    b = mk()
    b.reset()
    for t in range(5):           # a different past: everything that matters must come from the checkpoint
        b.step(act(900 + t))
    b.load_state_dict(sd)
    n_done = 0
    for t, (o_w, r_w, d_w, _) in zip(range(17, 42), want):
        o, r, d, _ = b.step(act(t))
        for k in o_w:
            assert torch.equal(o[k], o_w[k]), (k, t)
        assert torch.equal(r, r_w) and np.array_equal(d, d_w), t
        n_done += int(d.sum())
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("interval", [2, 3])
def test_hip_gst_wrapper_with_a_prediction_stride_matches_torch_expression(interval):
    """data.pred_timestep = interval x env.time_step (vec_pretext_normalize.py:56-57, :133-134): the history keeps 4 * interval + 1
    observations and every interval-th one feeds the predictor.  HIP wrapper vs the torch-op expression of the same processing on identical
    observation streams, from the dummy history through more than two full turns of the ring; then a save / load round trip of the history."""
    z = np.load(os.path.join(GOLDEN, "gst_e4_h20.npz"))
    pred = _model(json.loads(str(z["meta"])), "cuda")
    E, H = 37, 20
    w_hip = PretextProcessor(pred, E, H, 5, 0.3, 0.3, -20.0, torch.device("cuda"), use_hip=True, pred_interval=interval)
    w_ref = PretextProcessor(pred, E, H, 5, 0.3, 0.3, -20.0, torch.device("cuda"), use_hip=False, pred_interval=interval)
    assert w_ref.buffer_len == 4 * interval + 1
    g = torch.Generator(device="cuda").manual_seed(5)
    pos = torch.randn(E, H, 2, device="cuda", generator=g) * 3
    vel = torch.randn(E, H, 2, device="cuda", generator=g) * 0.2
    rob = torch.zeros(E, 1, 7, device="cuda")
    for t in range(3 * (4 * interval + 1)):
        pos = pos + vel
        rob[:, 0, :2] = 0.05 * t
        se = torch.zeros(E, H, 12, device="cuda")
        se[:, :, :2] = pos - rob[:, :, :2]
        se[:, :, 2:] = 15.0
        vis = (torch.rand(E, H, device="cuda", generator=g) > 0.25)
        obs = {"robot_node": rob.clone(), "spatial_edges": se, "visible_masks": vis}
        rew = torch.zeros(E, device="cuda")
        se_h, r_h = w_hip.process(obs, rew.clone())
        se_r, r_r = w_ref.process(obs, rew.clone())
        same = (se_h[:, :, :2] == se_r[:, :, :2]).all(-1).all(-1)
        assert float(same.float().mean()) > 0.95
        assert float((se_h[same] - se_r[same]).abs().max()) <= 1e-4, t
        assert float((r_h - r_r.reshape(E)).abs().max()) <= 1e-5, t
        if t == 2 * (4 * interval + 1) + 1:      # mid-turn: the ring is rotated
            sd_h, sd_r = w_hip.state_dict(), w_ref.state_dict()
            assert torch.equal(sd_h["traj"], sd_r["traj"]) and torch.equal(sd_h["mask"], sd_r["mask"]), "history in time order, oldest first"
            w_hip.load_state_dict(sd_h)             # un-rotated reload: the following steps must not notice


@pytest.mark.gpu
@pytest.mark.parametrize("interval", [1, 2])
def test_hip_gst_wrapper_taking_over_the_last_steps_encodings_is_bit_identical(interval):
    """Round 6: frames 1..3 of a step's observation window take their spatial encodings over from the previous step wherever the group's
    inputs and masks are the same bits (gst.hip, gst_reuse_kernel) -- the usual case with a stable visibility pattern -- and are encoded again
    wherever they are not (a human's visibility in the newest frame flipped, a history rewritten by load_state_dict).  The same stream of
    observations through a wrapper with the reuse switched off (CN_GST_REUSE=0, read when the handle is created) must give the same bits."""
    z = np.load(os.path.join(GOLDEN, "gst_e4_h20.npz"))
    pred = _model(json.loads(str(z["meta"])), "cuda")
    E, H = 97, 20
    w_on = PretextProcessor(pred, E, H, 5, 0.3, 0.3, -20.0, torch.device("cuda"), use_hip=True, pred_interval=interval)
    os.environ["CN_GST_REUSE"] = "0"
    try:
        w_off = PretextProcessor(pred, E, H, 5, 0.3, 0.3, -20.0, torch.device("cuda"), use_hip=True, pred_interval=interval)
    finally:
        del os.environ["CN_GST_REUSE"]
    g = torch.Generator(device="cuda").manual_seed(11)
    pos = torch.randn(E, H, 2, device="cuda", generator=g) * 3
    vel = torch.randn(E, H, 2, device="cuda", generator=g) * 0.2
    vel[::3] = 0.0                                          # every third env stands still: equal displacements also across a stride
    rob = torch.zeros(E, 1, 7, device="cuda")
    vis = torch.rand(E, H, device="cuda", generator=g) > 0.2
    for t in range(16):
        pos = pos + vel
        rob[:, 0, :2] = 0.05 * t
        se = torch.zeros(E, H, 12, device="cuda")
        se[:, :, :2] = pos - rob[:, :, :2]
        se[:, :, 2:] = 15.0
        flip = torch.rand(E, H, device="cuda", generator=g) < 0.01   # ~1 human in 100 enters / leaves the view per step: ~18 % of the envs change
        vis = vis ^ flip
        obs = {"robot_node": rob.clone(), "spatial_edges": se, "visible_masks": vis.clone()}
        a_se, a_r = w_on.process(obs, torch.zeros(E, device="cuda"))
        b_se, b_r = w_off.process(obs, torch.zeros(E, device="cuda"))
        assert torch.equal(a_se, b_se) and torch.equal(a_r, b_r), t
        if t == 9:                                          # a rewritten history: nothing of the previous window may be taken over blindly
            sd = w_on.state_dict()
            sd["traj"] = sd["traj"] + 0.125
            w_on.load_state_dict(sd); w_off.load_state_dict(sd)


def _check_wide(device, use_hip, interval):
    """PretextProcessor against the reference's VecPretextNormalize.process_obs_rew at 64 envs (tests/golden/gst_wrapper_e64_h20.npz, made by
    make_golden_gst.py --wide from the reference's own class): predictions / rewards <= 1e-4 absolute, identical row order wherever the
    sort key has no rounding-level tie."""
    from tests import policy_util as PU
    z = np.load(os.path.join(GOLDEN, "gst_wrapper_e64_h20.npz"))
    meta = json.loads(str(z["meta"]))
    E, H, steps = meta["E"], meta["H"], meta["steps"][str(interval)]
    m = _model(meta, device)
    w = PretextProcessor(m, E, H, 5, 0.3, 0.3, -20.0, torch.device(device), use_hip=use_hip, pred_interval=interval)
    n_same = 0
    for t, o in enumerate(PU.gst_wrapper_stream(E, H, steps, meta["seed"])):
        obs = {"robot_node": torch.from_numpy(o["robot_node"]).to(device), "spatial_edges": torch.from_numpy(o["spatial_edges"]).to(device),
               "visible_masks": torch.from_numpy(o["visible_masks"]).to(device)}
        se, rews = w.process(obs, torch.from_numpy(o["rews_in"]).to(device))
        se, rews = se.cpu().numpy(), rews.cpu().numpy().reshape(E, 1)
        want_se, want_r = z["se_i%d" % interval][t], z["rews_i%d" % interval][t].reshape(E, 1)
        np.testing.assert_allclose(rews, want_r, rtol=0, atol=1e-4, err_msg="reward t=%d" % t)
        same = (se[:, :, :2] == want_se[:, :, :2]).all(-1).all(-1)
        n_same += int(same.sum())
        np.testing.assert_allclose(se[same], want_se[same], rtol=0, atol=1e-4, err_msg="spatial_edges t=%d" % t)
    assert n_same >= 0.98 * E * steps, "row order must agree except for rounding-level ties of the distance key"


@pytest.mark.parametrize("interval", [1, 2])
def test_wrapper_torch_path_matches_reference_at_64_envs_with_and_without_a_prediction_stride(interval):
    _check_wide("cpu", False, interval)


@pytest.mark.gpu
@pytest.mark.parametrize("interval", [1, 2])
def test_hip_gst_wrapper_matches_reference_at_64_envs_with_and_without_a_prediction_stride(interval):
    _check_wide("cuda", True, interval)
