"""-m gpu: the four network-size flags (human_node_rnn_size R, human_node_embedding_size M, attention_size A, human_node_output_size O) through the HIP
path -- cn_policy_create_sized, the robot-node kernel with run-time sizes (csrc/rn_sized.hip) in fused mode, the separate launches of modes
'bf16x3' / 'fp32' -- on the reference-generated vectors of tests/golden/polsize_*.npz / rollsize_*.npz and against the fp64 host mirror on synthetic
observations.  See tests/test_policy_sizes.py for the CPU side.

Bars.  Project bars of tests/test_gpu_policy_variants.py: 1e-4 for 'fused' and 'bf16x3', 3e-5 for 'fp32'.  They were set at the default widths; for
the five golden tuples the fp32 CPU mirror is within
    (64,64,32,64) 7.2e-7   (256,128,128,512) 1.0e-6   (192,64,48,320) 1.1e-6   (128,128,64,256) 1.1e-6   (128,64,16,256) 7.5e-7
of the fp64 mirror (largest of value / action / logp / hidden state), so 4 x that distance stays two orders below the project bars and every case
keeps them."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from crowdnav_prediction_attngraph_amd import _abi as A  # noqa: E402
from crowdnav_prediction_attngraph_amd.policy import Policy, make_spaces  # noqa: E402
from tests import policy_util as PU  # noqa: E402
from tests.test_policy_sizes import PATHS, ROLL, build, filled_rollouts, inputs, load_formula_weights, size_kwargs, update_policy  # noqa: E402
from tests.test_policy_variants import check_update_against_the_reference  # noqa: E402

MODES = ("fused", "bf16x3", "fp32")
BAR = {"fused": 1e-4, "bf16x3": 1e-4, "fp32": 3e-5}
SMALL, LARGE, RAGGED = (64, 64, 32, 64), (256, 128, 128, 512), (192, 64, 48, 320)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", PATHS, ids=lambda p: os.path.basename(p)[8:-4])
def test_sized_rollout_forward_matches_the_reference(path, mode):
    z = np.load(path)
    meta = json.loads(str(z["meta"]))
    N = meta["N"]
    pol = load_formula_weights(build(meta), meta).cuda()
    pol.rollout_gemm_mode = mode
    obs, hxs = inputs(z, meta, "cuda", n=N)
    masks = torch.from_numpy(z["masks"][:N]).cuda()
    value, action, logp, hx = pol.act(obs, hxs, masks, deterministic=True)
    gv = pol.get_value(obs, hxs, masks)
    for got, want, what in ((value, z["value"], "value"), (action, z["action"], "action"), (logp, z["logp"], "logp"), (hx["human_node_rnn"], z["hx_out"], "hx"),
                            (gv, z["get_value"], "get_value")):
        err = float(np.abs(got.cpu().numpy().reshape(want.shape) - want).max())
        print("%s %s %s: max |device - reference| = %.3e (bar %.0e)" % (os.path.basename(path), mode, what, err, BAR[mode]))
        assert err <= BAR[mode], what
    hip = pol._hip_policy(N, torch.device("cuda", torch.cuda.current_device()))
    assert hip.dims.astuple() == tuple(meta["dims"]) and hip.state_shapes(N) == {"human_node_rnn": (N, 1, meta["dims"][0])}
    hip.set_taps(True)
    pol.act(obs, hxs, masks, deterministic=True)
    feat = hip.taps(N)["actor_feat"]
    assert feat.shape == (N, meta["dims"][3])
    np.testing.assert_allclose(feat.cpu().numpy(), z["actor_feat"], atol=BAR[mode])


# ---- synthetic shapes against the fp64 mirror ----
def sized_policy(dims, H, D=2, **kw):
    ob_space, act_space = make_spaces(H, D)
    torch.manual_seed(0)
    pol = Policy(ob_space.spaces, act_space, base="selfAttn_merge_srnn", base_kwargs=dict(size_kwargs(dims), **kw))
    shapes = {k: tuple(v.shape) for k, v in pol.state_dict().items()}
    pol.load_state_dict({k: torch.from_numpy(v) for k, v in PU.formula_state_dict(shapes).items()})
    return pol


def mirror64(pol64, ob, h, masks, eps):
    """One step of the host mirror in fp64 with its taps: value, action (mean + std * eps, or the mode), logp, h', robot_emb, hr_attn, hr_out, actor_feat."""
    base = pol64.base
    E = masks.shape[0]
    d = lambda x: torch.from_numpy(np.asarray(x)).double()
    inp = {k: (d(v) if k != "visible_masks" else torch.from_numpy(v)) for k, v in ob.items()}
    with torch.no_grad():
        value, feat, hx = base.forward_rnn(inp, {"human_node_rnn": d(h)}, d(masks), 1, E)
        mean = pol64.dist.fc_mean(feat)
        std = pol64.dist.logstd(torch.zeros_like(mean)).exp()
        action = mean if eps is None else mean + std * d(eps)
        logp = pol64._log_prob(mean, std, action)
        c = base.counted_inputs(inp)
        rs = base.robot_linear(torch.cat((c["temporal_edges"].reshape(E, 2), c["robot_node"].reshape(E, 7)), -1))
        det = c["detected_human_num"].reshape(E).to(torch.int64).clamp(min=1)
        out_sp, valid = base._hh_block(c["spatial_edges"].reshape(E, base.human_num, base.edge_width), det)
        hr, attn = base._hr_attention(rs, out_sp, valid)
    return dict(value=value.numpy(), action=action.numpy(), logp=logp.numpy(), hxs=hx["human_node_rnn"].numpy().reshape(E, -1), robot_emb=rs.numpy(),
                hr_attn=attn.numpy(), hr_out=hr.numpy(), actor_feat=feat.numpy())


GUARD = 96


def guarded(n, dev):
    """n floats of NaN with GUARD floats of NaN behind them: (view of the n, the whole buffer)."""
    buf = torch.full((n + GUARD,), float("nan"), device=dev)
    return buf[:n], buf


def device_step(hip, ob_dev, h_in, masks, eps, E, H, dims):
    """cn_policy_act into NaN-filled outputs with guard tails, then the taps the same way.  Returns the outputs, and checks the tails."""
    dev = hip.device
    R, O = dims[0], dims[3]
    sizes = dict(value=E, action=2 * E, logp=E, hxs=E * R)
    bufs = {k: guarded(n, dev) for k, n in sizes.items()}
    out = {k: v[0] for k, v in bufs.items()}
    hip.act(ob_dev, h_in, masks, eps=eps, out=dict(value=out["value"].view(E, 1), action=out["action"].view(E, 2), logp=out["logp"].view(E, 1),
                                                    hxs=out["hxs"].view(E, 1, R)))
    tsizes = dict(spatial_lin=E * H * 256, hr_attn=E * H, hr_out=E * 256, robot_emb=E * 256, actor_feat=E * O)
    tb = {k: guarded(n, dev) for k, n in tsizes.items()}
    A.call("cn_policy_get_taps", hip._h, E, A.ptr(tb["spatial_lin"][0]), A.ptr(tb["hr_attn"][0]), A.ptr(tb["hr_out"][0]), A.ptr(tb["robot_emb"][0]),
           A.ptr(tb["actor_feat"][0]), A.stream_ptr(), device=dev)
    torch.cuda.synchronize()
    res = {}
    for k, (view, whole) in list(bufs.items()) + list(tb.items()):
        assert torch.isnan(whole[view.numel():]).all(), "guard tail behind %s was written" % k
        assert not torch.isnan(view).any(), "%s has entries the forward did not write" % k
        res[k] = view.clone()
    return res


@pytest.mark.parametrize("H", [1, 5, 20])
@pytest.mark.parametrize("dims", [SMALL, LARGE, RAGGED], ids=["small", "large", "ragged"])
def test_sized_forward_past_one_workgroup_against_the_fp64_mirror(dims, H):
    """E = 1, 9, 17, 33: one and several workgroups at both envs-per-workgroup choices (16 at the small corner, 8 at the other two) with a ragged
    last group; detected counts 1 and H, masks 0 and 1, noise given and NULL, the hidden state ping-ponged over three steps; all three modes
    against the fp64 mirror at the project bars, fused against bf16x3 at twice the bar, and two runs of a mode bit for bit."""
    from crowdnav_prediction_attngraph_amd.hip import HipPolicy
    D, R, O = 2, dims[0], dims[3]
    pol = sized_policy(dims, H)
    pol64 = sized_policy(dims, H).double()
    sd = {k: v.cuda() for k, v in pol.state_dict().items()}
    hips = {}
    for mode in MODES:
        hips[mode] = HipPolicy(H, D, 33, dims=dims)
        hips[mode].set_gemm_mode(mode)
        hips[mode].set_weights(sd)
    for E in (1, 9, 17, 33):
        rs = np.random.RandomState(100 * E + H)
        h = rs.uniform(-1, 1, (E, R)).astype(np.float32)
        h_dev = {mode: torch.from_numpy(h).cuda() for mode in MODES}
        h64 = h.astype(np.float64)
        for step in range(3):
            ob = PU.synth_obs(E, H, D, seed=7000 + 10 * E + step)
            det = ob["detected_human_num"].reshape(-1)
            assert det[0] == 1 or E == 1
            assert det[-1] == H
            masks = (rs.uniform(size=(E, 1)) > 0.3).astype(np.float32)
            masks[0] = 1.0
            if E > 1:
                masks[-1] = 0.0
            eps = None if step == 1 else rs.standard_normal((E, 2)).astype(np.float32)
            want = mirror64(pol64, ob, h64, masks, eps)
            ob_dev = {k: torch.from_numpy(v).cuda() for k, v in ob.items()}
            m_dev = torch.from_numpy(masks).cuda()
            e_dev = None if eps is None else torch.from_numpy(eps).cuda()
            got = {}
            for mode in MODES:
                got[mode] = device_step(hips[mode], ob_dev, h_dev[mode].view(E, 1, R), m_dev, e_dev, E, H, dims)
                again = device_step(hips[mode], ob_dev, h_dev[mode].view(E, 1, R), m_dev, e_dev, E, H, dims)
                for k in got[mode]:
                    assert torch.equal(got[mode][k], again[k]), ("two runs differ", mode, k, E, step)
                for k in ("value", "action", "logp", "hxs", "robot_emb", "hr_out", "actor_feat"):
                    g = got[mode][k].cpu().numpy().astype(np.float64).reshape(want[k].shape)
                    err = float(np.abs(g - want[k]).max())
                    assert err <= BAR[mode], (mode, k, "E=%d step=%d" % (E, step), err)
                attn = got[mode]["hr_attn"].cpu().numpy().reshape(E, H)
                assert float(np.abs(attn - want["hr_attn"]).max()) <= BAR[mode] and all((attn[e, int(det[e]):] == 0).all() for e in range(E))
            for k in ("value", "action", "logp", "hxs", "actor_feat"):     # two independent implementations of the same arithmetic
                diff = float((got["fused"][k] - got["bf16x3"][k]).abs().max())
                assert diff <= 2 * BAR["fused"], (k, E, step, diff)
            h64 = want["hxs"]
            h_dev = {mode: got[mode]["hxs"].view(E, R).clone() for mode in MODES}
    for hip in hips.values():
        hip.close()


def sized_handle_at_default(H, D, E, dims_ptr):
    """A HipPolicy whose handle comes from cn_policy_create_sized (the wrapper itself takes cn_policy_create at the default dims)."""
    from crowdnav_prediction_attngraph_amd.hip import HipPolicy
    hip = HipPolicy.__new__(HipPolicy)
    hip.H, hip.D, hip.maxE = H, D, E
    hip.dims = A.policy_dims(None)
    hip.R, hip.O = 128, 256
    hip._open(None, H, D, E, dims_ptr, create="cn_policy_create_sized")
    return hip


@pytest.mark.parametrize("mode", MODES)
def test_the_default_dims_change_no_bit(mode):
    """cn_policy_create_sized with the default tuple, and with dims = NULL, against cn_policy_create at E = 33, H = 20: act, get_value and every tap."""
    from crowdnav_prediction_attngraph_amd.hip import HipPolicy
    E, H, D = 33, 20, 2
    pol = sized_policy(A.DEFAULT_DIMS, H)
    sd = {k: v.cuda() for k, v in pol.state_dict().items()}
    d = A.PolicyDims(128, 64, 64, 256)
    handles = [HipPolicy(H, D, E), sized_handle_at_default(H, D, E, C.byref(d)), sized_handle_at_default(H, D, E, None)]
    ob = {k: torch.from_numpy(v).cuda() for k, v in PU.synth_obs(E, H, D, seed=77).items()}
    g = torch.Generator().manual_seed(5)
    h = (torch.rand(E, 1, 128, generator=g) * 2 - 1).cuda()
    masks = (torch.rand(E, 1, generator=g) > 0.2).float().cuda()
    eps = torch.randn(E, 2, generator=g).cuda()
    res = []
    for hip in handles:
        hip.set_gemm_mode(mode)
        hip.set_weights(sd)
        out = hip.act(ob, h, masks, eps=eps)
        taps = hip.taps(E)
        value = hip.get_value(ob, h, masks)
        res.append(dict(out, get_value=value, **{"tap_" + k: v for k, v in taps.items()}))
    torch.cuda.synchronize()
    for other in res[1:]:
        for k, v in res[0].items():
            assert torch.equal(v, other[k]), k
    for hip in handles:
        hip.close()


def test_create_sized_refuses_sizes_outside_the_box_in_the_library_too():
    h = C.c_void_p()
    for bad in ((96, 64, 64, 256), (128, 64, 64, 576), (128, 96, 64, 256), (128, 64, 0, 256)):
        d = A.PolicyDims(*bad)
        with pytest.raises(A.CnError, match="outside the device box"):
            A.call("cn_policy_create_sized", 5, 2, 4, C.byref(d), C.byref(h), device=torch.device("cuda", 0))


@pytest.mark.parametrize("use_self_attn,sort_humans", [(False, True), (True, False)])
def test_sized_variants_against_the_fp64_mirror(use_self_attn, sort_humans):
    """use_self_attn = False / sort_humans = False at (192, 64, 48, 320): the sized half must not care what produced out_sp."""
    E, H, D = 9, 10, 2
    kw = dict(use_self_attn=use_self_attn, sort_humans=sort_humans)
    pol = sized_policy(RAGGED, H, **kw).cuda()
    pol64 = sized_policy(RAGGED, H, **kw).double()
    ob = PU.synth_obs(E, H, D, seed=41)
    rs = np.random.RandomState(8)
    det = ob["detected_human_num"].reshape(E).astype(int)
    vm = np.arange(H)[None, :] < det[:, None]
    if not sort_humans:
        for e in range(E):
            perm = rs.permutation(H)
            ob["spatial_edges"][e], vm[e] = ob["spatial_edges"][e][perm], vm[e][perm]
        vm[E // 2] = False
        ob["detected_human_num"] = np.maximum(vm.sum(1), 1).astype(np.float32).reshape(E, 1)
    ob["visible_masks"] = vm
    h = rs.uniform(-1, 1, (E, 192)).astype(np.float32)
    masks = np.ones((E, 1), np.float32)
    masks[2] = 0.0
    want = mirror64(pol64, ob, h.astype(np.float64), masks, None)
    ob_dev = {k: torch.from_numpy(v).cuda() for k, v in ob.items()}
    hxs = {"human_node_rnn": torch.from_numpy(h).cuda().view(E, 1, 192), "human_human_edge_rnn": torch.zeros(E, H + 1, 256, device="cuda")}
    for mode in MODES:
        pol.rollout_gemm_mode = mode
        value, action, logp, hx = pol.act(ob_dev, hxs, torch.from_numpy(masks).cuda(), deterministic=True)
        for got, k in ((value, "value"), (action, "action"), (logp, "logp"), (hx["human_node_rnn"], "hxs")):
            err = float(np.abs(got.cpu().numpy().astype(np.float64).reshape(want[k].shape) - want[k]).max())
            assert err <= BAR[mode], (mode, k, err)


def test_sized_training_forward_and_gradients():
    """evaluate_actions on the GPU at (192, 64, 48, 320) -- the fused human-human block in front of the torch-op robot-node part -- against the
    reference's outputs, and every gradient against the CPU graph of the same module."""
    import copy
    path = [p for p in PATHS if "r192" in p][0]
    z = np.load(path)
    meta = json.loads(str(z["meta"]))
    N = meta["N"]
    pol_c = load_formula_weights(build(meta), meta)
    pol_g = copy.deepcopy(pol_c).cuda()
    res = {}
    for name, pol, dev in (("cpu", pol_c, "cpu"), ("gpu", pol_g, "cuda")):
        obs, hxs = inputs(z, meta, dev)
        v, lp, ent, hx = pol.evaluate_actions(obs, hxs, torch.from_numpy(z["masks"]).to(dev), torch.from_numpy(z["actions"]).to(dev))
        pol.zero_grad()
        (v.mean() + 0.3 * lp.mean()).backward()
        res[name] = (v.detach().cpu().numpy(), lp.detach().cpu().numpy(), hx["human_node_rnn"].detach().cpu().numpy().reshape(N, -1),
                     {k: p.grad.detach().cpu().double() for k, p in pol.named_parameters() if p.grad is not None})
    np.testing.assert_allclose(res["gpu"][0], z["ev_value"], atol=1e-4)
    np.testing.assert_allclose(res["gpu"][1], z["ev_logp"], atol=1e-4)
    np.testing.assert_allclose(res["gpu"][2], z["ev_hx"].reshape(N, -1), atol=1e-4)
    assert set(res["cpu"][3]) == set(res["gpu"][3])
    for k, gc in res["cpu"][3].items():
        scale = max(float(gc.abs().max()), 1e-6)
        err = float((gc - res["gpu"][3][k]).abs().max())
        assert err <= 3e-4 * scale + 1e-7, (k, err, scale)


def test_sized_ppo_update_reference_golden_through_the_hip_path():
    """The reference's PPO.update at (192, 64, 48, 320) replayed on the GPU, with tests/test_gpu_policy_variants.py's arguments."""
    from crowdnav_prediction_attngraph_amd import hip_train
    z = np.load(ROLL[0])
    meta = json.loads(str(z["meta"]))
    pol = update_policy(meta).cuda()
    ro = filled_rollouts(z, meta, pol, "cuda")
    assert not hip_train.MinibatchStepper.supported(pol, ro)      # the one-call minibatch step knows the default sizes only
    check_update_against_the_reference(z, meta, pol, ro, atol=2e-6, rtol=1e-5)


NETWORK = dict(human_node_rnn_size=192, human_node_embedding_size=64, attention_size=48, human_node_output_size=320)


def test_sized_training_checkpoints_and_resumes_bit_exact(tmp_path):
    from crowdnav_prediction_attngraph_amd import config as Cfg
    from crowdnav_prediction_attngraph_amd.trainer import train
    cfg = Cfg.Config(**{"sim.human_num": 5})
    kw = dict(env_name="CrowdSimVarNum-v0", num_processes=8, num_steps=4, seed=3, config=cfg, log=None, lr=1e-3, network=NETWORK)
    full, pol_full = train(num_updates=3, save_dir=str(tmp_path / "full"), **kw)
    assert pol_full.base.dims == (192, 64, 48, 320) and tuple(pol_full.base.humanNodeRNN.gru.weight_hh_l0.shape) == (576, 192)
    assert all(np.isfinite([r["value_loss"], r["action_loss"], r["entropy"]]).all() for r in full)
    part, _ = train(num_updates=2, save_dir=str(tmp_path / "a"), **kw)
    ck = os.path.join(str(tmp_path / "a"), "checkpoints", "00001.pt")
    assert os.path.isfile(ck) and os.path.isfile(ck[:-3] + ".resume.pt")
    rest, pol_res = train(num_updates=3, resume=ck, **kw)
    assert [r["update"] for r in rest] == [2]
    for k in ("value_loss", "action_loss", "entropy", "episodes", "eprewmean"):
        assert full[2][k] == rest[0][k], (k, full[2][k], rest[0][k])
    for (k, x), (_, y) in zip(pol_full.state_dict().items(), pol_res.state_dict().items()):
        assert torch.equal(x, y), k
    sd = torch.load(os.path.join(str(tmp_path / "full"), "checkpoints", "00002.pt"))
    assert list(sd) == list(pol_full.state_dict()) and tuple(sd["base.humanNodeRNN.output_linear.weight"].shape) == (320, 192)


def test_sized_batched_evaluation_and_its_batch_invariant_form():
    """evaluate_batched of 4 cases at (192, 64, 48, 320): the batch-invariant run (separate launches, 'bf16x3') equals the same four cases one at a
    time; the fused run reports the same protocol."""
    from crowdnav_prediction_attngraph_amd import config as Cfg
    from crowdnav_prediction_attngraph_amd.evaluation import evaluate_batched
    dev = torch.device("cuda", 0)
    cfg = Cfg.Config(**{"sim.human_num": 5})
    ob_space, act_space = make_spaces(5, 2)
    torch.manual_seed(11)
    pol = Policy(ob_space.spaces, act_space, base="selfAttn_merge_srnn",
                 base_kwargs=dict(env_name="CrowdSimVarNum-v0", num_processes=1, num_mini_batch=1, seq_length=30, **NETWORK)).to(dev)
    with torch.no_grad():
        pol.dist.fc_mean.bias.copy_(torch.tensor([0.3, -0.2]))
    cases = [0, 2, 4, 6]
    per_env = {}
    from crowdnav_prediction_attngraph_amd.evaluation import _batch_invariant, _evaluate_batched
    with _batch_invariant(pol, True):
        bat = _evaluate_batched(pol, "CrowdSimVarNum-v0", cfg, 7, cases, dev, None, per_env=per_env)
        singles = []
        for c in cases:
            pe = {}
            _evaluate_batched(pol, "CrowdSimVarNum-v0", cfg, 7, [c], dev, None, per_env=pe)
            singles.append(pe)
    assert bat["episodes"] == 4
    assert list(per_env["cases"]) == cases
    for i, pe in enumerate(singles):
        for k in ("outcome", "steps", "danger_steps", "danger_sum", "path_length", "ep_return"):       # per-env host lists, compared bit for bit
            assert pe[k][0] == per_env[k][i], (k, cases[i], pe[k][0], per_env[k][i])
    fused = evaluate_batched(pol, "CrowdSimVarNum-v0", cfg, 7, 4, device=dev)
    inv = evaluate_batched(pol, "CrowdSimVarNum-v0", cfg, 7, 4, device=dev, batch_invariant=True)
    assert pol.rollout_gemm_mode == "fused" and fused["episodes"] == inv["episodes"] == 4
    assert inv["success_rate"] + inv["collision_rate"] + inv["timeout_rate"] == pytest.approx(1.0)
