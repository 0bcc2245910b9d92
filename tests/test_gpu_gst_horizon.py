"""-m gpu: cn_gst_predict and cn_gst_wrapper_step at prediction horizons other than 5 (cn_gst_create_horizon, HipGST(pred_steps=P)): the
predictor against the float64 torch graph of GSTPredictor(5, P) on every row and the numpy oracle on sampled envs, the frame take-over against a
handle without it in bits, the wrapper's penalty / edge write-back / sort against a closed form in bits, the wrapper in the loop of
CrowdSimPredRealGST-v0 with sim.predict_steps = 3 against the oracle's wrapper; and at P = 5 the new entry point against cn_gst_create in bits.
tests/test_gst_horizon.py (no GPU) asserts what each case reaches."""
import copy
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from crowdnav_prediction_attngraph_amd.gst import PretextProcessor  # noqa: E402
from oracle import gst_oracle as GO  # noqa: E402
from tests import gst_horizon_util as HU  # noqa: E402
from tests import gst_shape_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
PCASES = list(HU.PREDICT_CASES)


def _handle(H, max_envs, sd, P, reuse=True, entry=None):
    """HipGST of horizon P with the weights set; reuse False: made under CN_GST_REUSE=0 (read when the handle is created); entry: the C entry
    point that makes it (None: the one HipGST uses)."""
    from crowdnav_prediction_attngraph_amd.hip import HipGST
    if not reuse:
        os.environ["CN_GST_REUSE"] = "0"
    try:
        if entry == "cn_gst_create":
            assert P == 5
            g = HipGST.__new__(HipGST)
            g.P, g.H, g.maxE = 5, H, max_envs
            g._open(None, H, max_envs)
        else:
            g = HipGST(H, max_envs, pred_steps=P)
    finally:
        os.environ.pop("CN_GST_REUSE", None)
    if sd is not None:
        g.set_weights(sd)
    return g


def _lib():
    from crowdnav_prediction_attngraph_amd import _abi as A
    return A.lib()


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _sampled_envs(E, H):
    p, s = U.launch_plan(E, H), U.special_envs(E)
    envs = {0, E - 1, s["present"], s["absent"], s["newest"]}
    node = (p["lstm_tiles"] - 1) * p["lstm_rows"]
    envs |= {e for e in (node // H - 1, node // H, (node - 1) // H, node // H + 1) if 0 <= e < E}
    envs |= set(np.random.RandomState(E).choice(E, min(E, 8), replace=False).tolist())
    return sorted(envs)[:16]


@functools.lru_cache(maxsize=None)
def _predict_case(case, P):
    """Model, inputs and references of a predict case, made once and never written (tests/test_gpu_gst_shapes.py's, for GSTPredictor(5, P))."""
    E, H = case
    m = HU.model(100 + H, P).cuda()
    traj, mask = (torch.from_numpy(a).cuda() for a in U.inputs(E, H, H))
    ref32, om32 = m(traj, mask)
    ref64, om64 = copy.deepcopy(m).double()(traj.double(), mask.double())
    assert torch.equal(om32.double(), om64) and tuple(ref64.shape) == (E, H, P, 5)
    valid = om64[..., 0] > 0
    d = float((ref32.double() - ref64)[valid].abs().max())
    return dict(m=m, traj=traj, mask=mask, ref64=ref64, om=om64, valid=valid, d=d, bar=max(1e-4, 4 * d))


@pytest.mark.parametrize("P", HU.HORIZONS)
@pytest.mark.parametrize("case", PCASES, ids=["x".join(map(str, c)) for c in PCASES])
def test_predict_at_a_horizon_follows_the_fp64_graph_the_oracle_and_a_handle_without_take_over(case, P):
    E, H = case
    c = _predict_case(case, P)
    sd = c["m"].state_dict()
    on, off = _handle(H, E, sd, P), _handle(H, E, sd, P, reuse=False)
    assert int(_lib().cn_gst_pred_steps(on._h)) == P
    out, om = on.predict(c["traj"], c["mask"])
    out_off, om_off = off.predict(c["traj"], c["mask"])
    valid = c["valid"]
    assert tuple(out.shape) == (E, H, P, 5) and int(valid.sum()) > 0 and int((~valid).sum()) > 0
    assert torch.equal(om.double(), c["om"])
    worst = float((out.double() - c["ref64"])[valid].abs().max())
    idx = _sampled_envs(E, H)
    want, want_m = GO.interface_forward(U.numpy_sd(c["m"]), c["traj"][idx].cpu().numpy(), c["mask"][idx].cpu().numpy(), pred_len=P)
    v = want_m[..., 0] > 0
    assert want.shape == (len(idx), H, P, 5) and np.array_equal(want_m, c["om"][idx].cpu().numpy())
    graphs = float(np.abs(want - c["ref64"][idx].cpu().numpy())[v].max())
    worst_np = float(np.abs(out[idx].cpu().numpy().astype(np.float64) - want)[v].max())
    print("predict %-9s P=%d rows %6d  |hip - fp64| %.3g  d = |fp32 - fp64| %.3g  bar %.3g  |hip - numpy| on %d envs %.3g  |fp64 - numpy| %.3g"
          % (case, P, E * H * 5, worst, c["d"], c["bar"], len(idx), worst_np, graphs))
    assert worst <= c["bar"] and worst_np <= c["bar"]
    assert graphs <= 1e-9, "the two float64 statements agree"
    assert bool((out[~valid][..., :2] == U.INVALID).all())
    assert _bits(out, out_off) and _bits(om, om_off)
    # a window shifted by one frame: the second call takes groups over and is still the handle without take-over, in bits
    t6, m6 = (torch.from_numpy(a).cuda() for a in U.inputs(E, H, H, frames=6))
    w0, w1 = (t6[:, :, :5].contiguous(), m6[:, :, :5].contiguous()), (t6[:, :, 1:].contiguous(), m6[:, :, 1:].contiguous())
    took = int(U.taken_over(U.prep(t6[:, :, :5].cpu().numpy(), m6[:, :, :5].cpu().numpy()), U.prep(t6[:, :, 1:].cpu().numpy(), m6[:, :, 1:].cpu().numpy())).sum())
    assert took > 0
    for win in (w0, w1):
        a, am = on.predict(*win)
        b, bm = off.predict(*win)
        assert _bits(a, b) and _bits(am, bm)
    ref64, om64 = copy.deepcopy(c["m"]).double()(w1[0].double(), w1[1].double())
    v1 = om64[..., 0] > 0
    shifted = float((a.double() - ref64)[v1].abs().max())
    print("predict %-9s P=%d shifted window: %d groups taken over, |hip - fp64| %.3g (bar %.3g)" % (case, P, took, shifted, c["bar"]))
    assert torch.equal(am.double(), om64) and shifted <= c["bar"]


def _obs(o, idx=None):
    sl = slice(None) if idx is None else idx
    return {k: torch.from_numpy(np.array(o[k][sl])).cuda() for k in ("robot_node", "spatial_edges", "visible_masks")}


def _processor(model, E, H, max_envs, P, reuse=True, entry=None):
    """PretextProcessor on the HIP path whose handle (of max_envs >= E envs) was made as _handle makes it."""
    w = PretextProcessor(model, E, H, P, 0.3, 0.3, U.PENALTY, torch.device("cuda"), use_hip=False)
    w.hip = _handle(H, max_envs, model.state_dict(), P, reuse, entry)
    w.hip.wrapper_set_interval(1)
    w.reset_buffers()
    return w


def test_a_five_step_handle_of_the_new_entry_is_the_handle_of_cn_gst_create_in_bits():
    """predict on a case of tests/test_gpu_gst_shapes.py's kind and 14 wrapper steps over U.wrapper_stream(97, 21, 14, seed) with the events of
    the wrapper cases (history shifted, new weights, reset)."""
    E, H, _ = HU.WRAPPER_CASE
    m1, m2 = (m.cuda() for m in U.wrapper_models(H))
    new, old = _handle(H, E, m1.state_dict(), 5), _handle(H, E, m1.state_dict(), 5, entry="cn_gst_create")
    assert int(_lib().cn_gst_pred_steps(new._h)) == int(_lib().cn_gst_pred_steps(old._h)) == 5
    t6, k6 = (torch.from_numpy(a).cuda() for a in U.inputs(E, H, H, frames=6))
    for sl in (slice(0, 5), slice(1, 6)):
        a, am = new.predict(t6[:, :, sl].contiguous(), k6[:, :, sl].contiguous())
        b, bm = old.predict(t6[:, :, sl].contiguous(), k6[:, :, sl].contiguous())
        assert _bits(a, b) and _bits(am, bm) and tuple(a.shape) == (E, H, 5, 5)
    wn, wo = _processor(m1, E, H, E, 5), _processor(m1, E, H, E, 5, entry="cn_gst_create")
    for t, o in enumerate(U.wrapper_stream(E, H, U.WRAPPER_STEPS, HU.WRAPPER_SEED)):
        obs, rin = _obs(o), torch.from_numpy(o["rews_in"].copy()).cuda()
        se_a, r_a = wn.process(obs, rin.clone())
        se_b, r_b = wo.process(obs, rin.clone())
        assert _bits(se_a, se_b) and _bits(r_a, r_b), t

        def on_history():
            sd = wn.state_dict()
            sd["traj"] = sd["traj"] + 0.125
            wn.load_state_dict(sd); wo.load_state_dict(sd)

        def on_weights():
            wn.hip.set_weights(m2.state_dict()); wo.hip.set_weights(m2.state_dict())

        def on_reset():
            wn.reset_buffers(); wo.reset_buffers()
        U.apply_event(t, on_history, on_weights, on_reset)


@pytest.mark.parametrize("P", HU.HORIZONS)
def test_wrapper_at_a_horizon_follows_the_torch_path_and_the_oracle_and_takes_frames_over(P):
    """tests/test_gpu_gst_shapes.py's wrapper test at (97, 21) and an edge width of 2 (P + 1), same bars: row order equal in every env; edges
    within 1e-4 and rewards within 1e-5 of the float32 torch path; edges within max(1e-4, 4 d) of the numpy oracle on the followed envs; the bits
    of a handle without take-over; rows that are not predicted keep their input columns."""
    E, H, max_envs = HU.WRAPPER_CASE
    m1, m2 = (HU.model(100 + H, P).cuda(), HU.model(200 + H, P).cuda())
    stream = HU.wrapper_stream(E, H, U.WRAPPER_STEPS, HU.WRAPPER_SEED, P)
    idx = U.sliced_envs(E, H)
    ow = GO.PretextWrapper(U.numpy_sd(m1), len(idx), H, P, 0.3, 0.3, U.PENALTY)
    on, off = _processor(m1, E, H, max_envs, P), _processor(m1, E, H, max_envs, P, reuse=False)
    ref = PretextProcessor(m1, E, H, P, 0.3, 0.3, U.PENALTY, torch.device("cuda"), use_hip=False)
    hist = U.History(E, H)
    worst = dict(torch=0.0, rew=0.0, oracle=0.0, d=0.0, rew_o=0.0)
    kept = 0
    for t, o in enumerate(stream):
        obs, rin = _obs(o), torch.from_numpy(o["rews_in"].copy()).cuda()
        se_a, r_a = on.process(obs, rin.clone())
        se_b, r_b = off.process(obs, rin.clone())
        assert tuple(se_a.shape) == (E, H, 2 * (P + 1)) and _bits(se_a, se_b) and _bits(r_a, r_b), t
        se_r, r_r = ref.process(obs, rin.clone())
        assert torch.equal(se_a[:, :, :2], se_r[:, :, :2]), "row order, every env (step %d)" % t
        worst["torch"] = max(worst["torch"], float((se_a - se_r).abs().max()))
        worst["rew"] = max(worst["rew"], float((r_a - r_r.reshape(E)).abs().max()))
        assert worst["torch"] <= 1e-4 and worst["rew"] <= 1e-5, (t, worst)
        want_se, want_r = ow.process(o["robot_node"][idx], o["spatial_edges"][idx], o["visible_masks"][idx], o["rews_in"][idx].reshape(-1, 1))
        a_np, r_np = se_a[idx].cpu().numpy(), se_r[idx].cpu().numpy()
        assert np.array_equal(a_np[:, :, :2], want_se[:, :, :2]), "row order against the oracle (step %d)" % t
        d, err = float(np.abs(r_np - want_se).max()), float(np.abs(a_np - want_se).max())
        worst["oracle"], worst["d"] = max(worst["oracle"], err), max(worst["d"], d)
        assert err <= max(1e-4, 4 * d), (t, err, d)
        worst["rew_o"] = max(worst["rew_o"], float(np.abs(r_a[idx].cpu().numpy() - want_r.reshape(-1)).max()))
        assert worst["rew_o"] <= 1e-5, (t, worst)
        hist.push(o)
        order = np.argsort(U.sort_keys(o["spatial_edges"])[0], axis=1, kind="stable")
        keep = np.take_along_axis(~hist.out_mask(), order, axis=1)
        rows_in = np.take_along_axis(o["spatial_edges"], order[:, :, None], axis=1)
        assert np.array_equal(se_a.cpu().numpy()[keep].view(np.uint32), rows_in[keep].view(np.uint32)), t
        kept += int(keep.sum())

        def on_history():
            sd = on.state_dict()
            assert _bits(sd["traj"], torch.from_numpy(hist.traj))
            sd["traj"] = sd["traj"] + 0.125
            hist.traj = hist.traj + np.float32(0.125)
            ow.traj = [x + np.float32(0.125) for x in ow.traj]
            for w in (on, off, ref):
                w.load_state_dict(sd)

        def on_weights():
            on.hip.set_weights(m2.state_dict()); off.hip.set_weights(m2.state_dict())
            ref.pred = m2
            ow.sd = U.numpy_sd(m2)

        def on_reset():
            for w in (on, off, ref):
                w.reset_buffers()
            hist.reset()
            ow.traj = [np.full((len(idx), H, 2), U.INVALID) for _ in range(U.T_OBS)]
            ow.mask = [np.zeros((len(idx), H, 1), dtype=bool) for _ in range(U.T_OBS)]
        U.apply_event(t, on_history, on_weights, on_reset)
    share, _ = U.reuse_share(E, H, HU.WRAPPER_SEED)
    assert 0 < kept < E * H * U.WRAPPER_STEPS and share > 0.3     # frames were taken over (the rule does not depend on P)
    print("wrapper %s P=%d |hip - torch| edges %.3g rewards %.3g   |hip - oracle| edges %.3g (d = |torch - oracle| %.3g) rewards %.3g   rows kept %d, taken over %.2f"
          % (HU.WRAPPER_CASE, P, worst["torch"], worst["rew"], worst["oracle"], worst["d"], worst["rew_o"], kept, share))


@pytest.mark.parametrize("H", HU.CV_SIZES)
@pytest.mark.parametrize("P", HU.HORIZONS)
def test_wrapper_penalty_edges_and_sort_are_exact_at_a_horizon_with_a_constant_velocity_predictor(P, H):
    """hidden2pos.weight = 0, bias = (vx, vy, 0, 0, 0): every prediction is last_pos + (k + 1) v, k < P.  Rewards are rews_in + (-20 / 2^(k+2)) of
    the earliest colliding horizon; columns 2 .. 2P+1 are last_pos + (k + 1) v - robot_xy; rows are in key order with ties in index order -- all
    E * H rows of every step, in bits."""
    E = P + 2
    m = U.const_velocity_predictor(HU.model(100 + H, P), *HU.CV_V).cuda()
    w = _processor(m, E, H, E, P)
    hist = U.History(E, H)
    seen = set()
    for t, o in enumerate(HU.cv_stream(H, P)):
        se, rews = w.process(_obs(o), torch.from_numpy(o["rews_in"].copy()).cuda())
        hist.push(o)
        want_se, want_r, first = HU.cv_expected(hist, o, P)
        seen |= set(first.tolist())
        assert np.array_equal(rews.cpu().numpy().view(np.uint32), want_r.view(np.uint32)), (t, rews.cpu().numpy(), want_r)
        assert se.shape == want_se.shape == (E, H, 2 * (P + 1)) and np.array_equal(se.cpu().numpy().view(np.uint32), want_se.view(np.uint32)), t
    assert seen == set(range(-1, P))


def test_wrapper_in_the_loop_of_the_env_with_three_predicted_steps():
    """make_vec_envs('CrowdSimPredRealGST-v0') with sim.predict_steps = 3 and a seeded random predictor of pred_len 3, 6 envs x 8 humans, reset +
    12 steps.  A second batch without the wrapper, same seed and actions, gives the raw observations and rewards the oracle's wrapper is fed."""
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd.vec_env import make_vec_envs
    E, H, P, dev = 6, 8, 3, torch.device("cuda", 0)
    cfg = C.non_randomized(**{"sim.human_num": H, "sim.predict_method": "inferred", "sim.predict_steps": P})
    pred = HU.model(33, P).to(dev)
    envs = make_vec_envs("CrowdSimPredRealGST-v0", 425, E, 0.99, None, dev, False, config=cfg, pretext_wrapper=True, predictor=pred)
    raw_envs = make_vec_envs("CrowdSimPredRealGST-v0", 425, E, 0.99, None, dev, False, config=cfg, pretext_wrapper=False)
    assert envs.edge_width == 2 * (P + 1) and envs._pretext.hip is not None and envs._pretext.hip.P == P
    ow = GO.PretextWrapper(U.numpy_sd(pred), E, H, P, float(envs.cfg.robot_radius), float(envs.cfg.human_radius), float(envs.cfg.collision_penalty))
    ref = PretextProcessor(pred, E, H, P, float(envs.cfg.robot_radius), float(envs.cfg.human_radius), float(envs.cfg.collision_penalty), dev, use_hip=False)
    obs, raw = envs.reset_device(), raw_envs.reset_device()
    rew = raw_rew = torch.zeros(E, device=dev)
    gen = torch.Generator(device="cuda").manual_seed(7)
    worst, written = dict(oracle=0.0, d=0.0, rew=0.0), 0
    for t in range(13):
        assert tuple(obs["spatial_edges"].shape) == (E, H, 2 * (P + 1))
        assert torch.equal(obs["robot_node"], raw["robot_node"]), t
        raw_np = {k: raw[k].cpu().numpy() for k in ("robot_node", "spatial_edges", "visible_masks")}
        rin = raw_rew.reshape(E).float().cpu().numpy()
        want_se, want_r = ow.process(raw_np["robot_node"], raw_np["spatial_edges"], raw_np["visible_masks"].astype(bool), rin.reshape(-1, 1))
        se_r, r_r = ref.process({k: v.clone() for k, v in raw.items()}, raw_rew.reshape(E).float().clone())
        got = obs["spatial_edges"].cpu().numpy()
        assert np.array_equal(got[:, :, :2], want_se[:, :, :2]), "row order against the oracle (step %d)" % t
        d, err = float(np.abs(se_r.cpu().numpy() - want_se).max()), float(np.abs(got - want_se).max())
        worst["oracle"], worst["d"] = max(worst["oracle"], err), max(worst["d"], d)
        assert err <= max(1e-4, 4 * d), (t, err, d)
        worst["rew"] = max(worst["rew"], float(np.abs(rew.reshape(E).cpu().numpy() - want_r.reshape(-1)).max()))
        assert worst["rew"] <= 1e-5, (t, worst)
        written += int((got[:, :, 2:] != np.take_along_axis(raw_np["spatial_edges"], np.argsort(U.sort_keys(raw_np["spatial_edges"])[0], axis=1, kind="stable")[:, :, None],
                                                            axis=1)[:, :, 2:]).any())
        action = torch.empty(E, 2, device=dev).uniform_(-1.0, 1.0, generator=gen)
        obs, rew = envs.step_device(action)[:2]
        raw, raw_rew = raw_envs.step_device(action)[:2]
        obs, rew, raw, raw_rew = dict(obs), rew.clone(), {k: v.clone() for k, v in raw.items()}, raw_rew.clone()
    assert written >= 8                                      # predictions were written into the edges
    print("env loop P=3: |hip - oracle| edges %.3g (d = |torch - oracle| %.3g), rewards %.3g" % (worst["oracle"], worst["d"], worst["rew"]))
    envs.close()
    raw_envs.close()
