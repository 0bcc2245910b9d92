"""cn_gst_predict and cn_gst_wrapper_step away from 20 humans and past one turn of their workgroups (csrc/gst.hip): both LSTM templates with
ragged last tiles and more tiles than workgroups, encoder-layer tiles with padding rows over several turns, the attention core on both sides of
H = 20, the frame take-over with listed tiles of every kind, the wrapper's push / penalty / sort kernels at H = 1, 21, 50, 64.  Held to the
float64 torch graph on every row and to the numpy oracle on sampled envs; the take-over to the bits of a handle made with it switched off; the
penalty and the edge write-back to a closed form through a constant-velocity predictor.  tests/test_gst_shapes.py (no GPU) asserts what each
case reaches and the conditions under which no env has to be left out for row order or penalty."""
import copy
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from crowdnav_prediction_attngraph_amd import _abi as A  # noqa: E402
from crowdnav_prediction_attngraph_amd.gst import PretextProcessor  # noqa: E402
from oracle import gst_oracle as GO  # noqa: E402
from tests import gst_shape_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
PCASES, WCASES = list(U.PREDICT_CASES), list(U.WRAPPER_CASES)


def _ids(cases):
    return ["x".join(str(v) for v in c) for c in cases]


def _handle(H, max_envs, sd, reuse=True):
    """HipGST with the weights set; reuse False: made under CN_GST_REUSE=0 (read when the handle is created)."""
    from crowdnav_prediction_attngraph_amd.hip import HipGST
    if not reuse:
        os.environ["CN_GST_REUSE"] = "0"
    try:
        g = HipGST(H, max_envs)
    finally:
        os.environ.pop("CN_GST_REUSE", None)
    if sd is not None:
        g.set_weights(sd)
    return g


def _bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _sampled_envs(E, H):
    """At most 32 envs for the numpy oracle: first, last, those around LSTM tiles 255 / 256 and around the last LSTM tile, the special ones."""
    p, s = U.launch_plan(E, H), U.special_envs(E)
    envs = {0, E - 1, s["present"], s["absent"], s["newest"]}
    for node in (256 * p["lstm_rows"], (p["lstm_tiles"] - 1) * p["lstm_rows"]):
        envs |= {e for e in (node // H - 1, node // H, (node - 1) // H, node // H + 1) if 0 <= e < E}
    rs = np.random.RandomState(E)
    envs |= set(rs.choice(E, 12, replace=False).tolist())
    return sorted(envs)[:32]


@functools.lru_cache(maxsize=None)
def _predict_case(case):
    """Model, inputs and references of a predict case, made once and never written: the float64 and the float32 torch graph on the device over
    all rows, d = their largest difference on valid rows, the bar max(1e-4, 4 d), and the result of a handle without take-over."""
    E, H = case
    m = U.model(100 + H).cuda()
    traj, mask = (torch.from_numpy(a).cuda() for a in U.inputs(E, H, H))
    ref32, om32 = m(traj, mask)
    ref64, om64 = copy.deepcopy(m).double()(traj.double(), mask.double())
    assert torch.equal(om32.double(), om64)
    valid = om64[..., 0] > 0
    d = float((ref32.double() - ref64)[valid].abs().max())
    off = _handle(H, E, m.state_dict(), reuse=False)
    out_off, om_off = off.predict(traj, mask)
    return dict(m=m, traj=traj, mask=mask, ref64=ref64, om=om64, valid=valid, d=d, bar=max(1e-4, 4 * d), off=off, out_off=out_off.clone(), om_off=om_off.clone())


@pytest.mark.parametrize("case", PCASES, ids=_ids(PCASES))
def test_predict_follows_the_fp64_graph_on_every_row_and_the_numpy_oracle(case):
    E, H = case
    c = _predict_case(case)
    g = _handle(H, E, c["m"].state_dict())
    out, om = g.predict(c["traj"], c["mask"])
    valid = c["valid"]
    assert int(valid.sum()) > 0 and int((~valid).sum()) > 0
    assert torch.equal(om.double(), c["om"])
    worst = float((out.double() - c["ref64"])[valid].abs().max())
    idx = _sampled_envs(E, H)
    want, want_m = GO.interface_forward(U.numpy_sd(c["m"]), c["traj"][idx].cpu().numpy(), c["mask"][idx].cpu().numpy())
    v = want_m[..., 0] > 0
    assert np.array_equal(want_m, c["om"][idx].cpu().numpy())
    graphs = float(np.abs(want - c["ref64"][idx].cpu().numpy())[v].max())
    worst_np = float(np.abs(out[idx].cpu().numpy().astype(np.float64) - want)[v].max())
    print("predict %-10s rows %6d  |hip - fp64| %.3g  d = |fp32 - fp64| %.3g  bar %.3g  |hip - numpy| on %d envs %.3g  |fp64 - numpy| %.3g"
          % (case, E * H * 5, worst, c["d"], c["bar"], len(idx), worst_np, graphs))
    assert worst <= c["bar"] and worst_np <= c["bar"]
    assert graphs <= 1e-9, "the two float64 statements agree"
    assert bool((out[~valid][..., :2] == U.INVALID).all())
    # the first call of a handle lists every group: tiles of listed groups against tiles of consecutive rows
    assert _bits(out, c["out_off"]) and _bits(om, c["om_off"])


@pytest.mark.parametrize("case", PCASES, ids=_ids(PCASES))
def test_predict_takes_a_shifted_window_over_and_forgets_it_when_it_must(case):
    """Frames 0..4, then frames 1..5 of the same six: the second call takes over what it may.  Then E, E - 1, E envs and new weights: every
    result is the bits of a handle that never takes anything over."""
    E, H = case
    c = _predict_case(case)
    m2 = U.model(200 + H).cuda()
    t6, m6 = (torch.from_numpy(a).cuda() for a in U.inputs(E, H, H, frames=6))
    w0, w1 = (t6[:, :, :5].contiguous(), m6[:, :, :5].contiguous()), (t6[:, :, 1:].contiguous(), m6[:, :, 1:].contiguous())
    on, off = _handle(H, E, c["m"].state_dict()), c["off"]

    def both(win, n=E):
        a, am = on.predict(win[0][:n], win[1][:n])
        b, bm = off.predict(win[0][:n], win[1][:n])
        assert _bits(a, b) and _bits(am, bm)
        return a, am
    both(w0)
    out, om = both(w1)                                     # take-over inside cn_gst_predict
    ref64, om64 = copy.deepcopy(c["m"]).double()(w1[0].double(), w1[1].double())
    valid = om64[..., 0] > 0
    worst = float((out.double() - ref64)[valid].abs().max())
    print("predict %-10s shifted window |hip - fp64| %.3g (bar %.3g)" % (case, worst, c["bar"]))
    assert torch.equal(om.double(), om64) and worst <= c["bar"]
    both(w0, E - 1)                                        # another E: the window of the call before is not this batch's
    both(w1)
    both(w0)
    try:
        on.set_weights(m2.state_dict())                    # new weights: the encodings held are not this model's
        off.set_weights(m2.state_dict())
        out2, _ = both(w1)
        assert not _bits(out2, out)
    finally:
        off.set_weights(c["m"].state_dict())               # the cached handle goes back as it was


def _obs(o, idx=None):
    sl = slice(None) if idx is None else idx
    return {k: torch.from_numpy(np.array(o[k][sl])).cuda() for k in ("robot_node", "spatial_edges", "visible_masks")}


def _processor(model, E, H, max_envs, reuse=True):
    """PretextProcessor on the HIP path whose handle holds max_envs >= E envs."""
    w = PretextProcessor(model, E, H, 5, 0.3, 0.3, U.PENALTY, torch.device("cuda"), use_hip=False)
    w.hip = _handle(H, max_envs, model.state_dict(), reuse)
    w.hip.wrapper_set_interval(1)
    w.reset_buffers()
    return w


@pytest.mark.parametrize("case", WCASES, ids=_ids(WCASES))
def test_wrapper_follows_the_torch_path_and_the_oracle_in_every_env(case):
    E, H, max_envs = case
    m1, m2 = (m.cuda() for m in U.wrapper_models(H))
    stream = U.wrapper_stream(E, H, U.WRAPPER_STEPS, U.WRAPPER_SEEDS[case])
    idx = U.sliced_envs(E, H)
    oracle = U.oracle_run(E, H, U.WRAPPER_SEEDS[case], idx)
    on, off = _processor(m1, E, H, max_envs), _processor(m1, E, H, max_envs, reuse=False)
    ref = PretextProcessor(m1, E, H, 5, 0.3, 0.3, U.PENALTY, torch.device("cuda"), use_hip=False)
    hist = U.History(E, H)
    worst = dict(torch=0.0, rew=0.0, oracle=0.0, d=0.0, rew_o=0.0)
    kept = 0
    for t, (o, want) in enumerate(zip(stream, oracle)):
        obs, rin = _obs(o), torch.from_numpy(o["rews_in"].copy()).cuda()
        se_a, r_a = on.process(obs, rin.clone())
        se_b, r_b = off.process(obs, rin.clone())
        assert _bits(se_a, se_b) and _bits(r_a, r_b), t
        se_r, r_r = ref.process(obs, rin.clone())
        assert torch.equal(se_a[:, :, :2], se_r[:, :, :2]), "row order, every env (step %d)" % t
        worst["torch"] = max(worst["torch"], float((se_a - se_r).abs().max()))
        worst["rew"] = max(worst["rew"], float((r_a - r_r.reshape(E)).abs().max()))
        assert worst["torch"] <= 1e-4 and worst["rew"] <= 1e-5, (t, worst)
        # the numpy oracle on the followed envs: bar from the float32 torch path's own distance to it
        a_np, r_np = se_a[idx].cpu().numpy(), se_r[idx].cpu().numpy()
        assert np.array_equal(a_np[:, :, :2], want["se"][:, :, :2]), "row order against the oracle (step %d)" % t
        d = float(np.abs(r_np - want["se"]).max())
        err = float(np.abs(a_np - want["se"]).max())
        worst["oracle"], worst["d"] = max(worst["oracle"], err), max(worst["d"], d)
        assert err <= max(1e-4, 4 * d), (t, err, d)
        worst["rew_o"] = max(worst["rew_o"], float(np.abs(r_a[idx].cpu().numpy() - want["rews"]).max()))
        assert worst["rew_o"] <= 1e-5, (t, worst)
        # rows of humans that are not predicted keep their input columns 2..11
        hist.push(o)
        order = np.argsort(U.sort_keys(o["spatial_edges"])[0], axis=1, kind="stable")
        keep = np.take_along_axis(~hist.out_mask(), order, axis=1)
        rows_in = np.take_along_axis(o["spatial_edges"], order[:, :, None], axis=1)
        assert np.array_equal(se_a.cpu().numpy()[keep].view(np.uint32), rows_in[keep].view(np.uint32)), t
        kept += int(keep.sum())

        def on_history():
            sd = on.state_dict()
            assert _bits(sd["traj"], torch.from_numpy(hist.traj)) and torch.equal(sd["mask"].bool(), torch.from_numpy(hist.mask))
            sd["traj"] = sd["traj"] + 0.125
            hist.traj = hist.traj + np.float32(0.125)
            for w in (on, off, ref):
                w.load_state_dict(sd)

        def on_weights():
            on.hip.set_weights(m2.state_dict())
            off.hip.set_weights(m2.state_dict())
            ref.pred = m2

        def on_reset():
            for w in (on, off, ref, hist):
                (w.reset if w is hist else w.reset_buffers)()
        U.apply_event(t, on_history, on_weights, on_reset)
    assert 0 < kept < E * H * U.WRAPPER_STEPS
    print("wrapper %-14s |hip - torch| edges %.3g rewards %.3g   |hip - oracle| edges %.3g (d = |torch - oracle| %.3g) rewards %.3g   rows kept %d"
          % (case, worst["torch"], worst["rew"], worst["oracle"], worst["d"], worst["rew_o"], kept))


@pytest.mark.parametrize("H", U.CV_SIZES)
def test_wrapper_penalty_edges_and_sort_are_exact_with_a_constant_velocity_predictor(H):
    """hidden2pos.weight = 0, bias = (vx, vy, 0, 0, 0): every prediction is last_pos + (k + 1) v.  Rewards are rews_in + (-20 / 2^(k+2)) of the
    earliest colliding horizon, rews_in where nobody collides; columns 2..11 are last_pos + (k + 1) v - robot_xy; rows are in key order with
    ties in index order -- all in bits."""
    E = 7
    m = U.const_velocity_predictor(U.model(100 + H), *U.CV_V).cuda()
    w = _processor(m, E, H, E)
    hist = U.History(E, H)
    seen = set()
    for t, o in enumerate(U.cv_stream(H)):
        se, rews = w.process(_obs(o), torch.from_numpy(o["rews_in"].copy()).cuda())
        hist.push(o)
        want_se, want_r, first = U.cv_expected(hist, o)
        seen |= set(first.tolist())
        assert np.array_equal(rews.cpu().numpy().view(np.uint32), want_r.view(np.uint32)), (t, rews.cpu().numpy(), want_r)
        assert np.array_equal(se.cpu().numpy().view(np.uint32), want_se.view(np.uint32)), t
    assert seen == {-1, 0, 1, 2, 3, 4}


def test_refusals_launch_nothing():
    g = _handle(21, 8, None)
    x, m = torch.zeros(4, 21, 5, 2, device="cuda"), torch.ones(4, 21, 5, 1, device="cuda")
    with pytest.raises(A.CnError, match="call cn_gst_set_weights first"):
        g.predict(x, m)
    g.set_weights(U.model(121).state_dict())
    g.wrapper_reset(4)
    o = U.wrapper_stream(5, 21, 1, 1)[0]
    with pytest.raises(A.CnError, match=r"call cn_gst_wrapper_reset\(E=5\) first"):
        g.wrapper_step(_obs(o), torch.zeros(5, device="cuda"), U.DIST, U.PENALTY)
    se = g.wrapper_step(_obs(o, slice(0, 4)), torch.zeros(4, device="cuda"), U.DIST, U.PENALTY)   # the handle is as usable as before
    assert bool(torch.isfinite(se).all())
