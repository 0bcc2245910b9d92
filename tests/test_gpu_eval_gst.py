"""-m gpu: the GST-predictor policy on the fast path -- evaluate_batched for CrowdSimPredRealGST-v0 behind the VecPretextNormalize
processing, the evaluation bookkeeping as one launch (cn_eval_accumulate), train() with the wrapper in the loop writing the rollout
storage in place, and evaluation inside train()."""
import json
import logging
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GST = "CrowdSimPredRealGST-v0"
LOG = logging.getLogger("eval-gst-test")


def _predictor(seed=0):
    from crowdnav_prediction_attngraph_amd.gst import GSTPredictor
    torch.manual_seed(seed)
    return GSTPredictor().to("cuda")


def _gst_config(**over):
    from crowdnav_prediction_attngraph_amd import config as C
    return C.non_randomized(**dict({"sim.human_num": 10, "sim.predict_method": "inferred", "env.test_size": 16}, **over))


def _policy(env_name, cfg, pred=None, seed=3):
    """The biased untrained policy of tests/test_gpu_eval.py:21-25 for `env_name`."""
    from crowdnav_prediction_attngraph_amd.policy import Policy
    from crowdnav_prediction_attngraph_amd.vec_env import make_vec_envs
    dev = torch.device("cuda", 0)
    envs = make_vec_envs(env_name, 7, 1, 0.99, None, dev, True, config=cfg, pretext_wrapper=pred is not None, predictor=pred)
    assert envs.cfg.phase == 2
    torch.manual_seed(seed)
    pol = Policy(envs.observation_space.spaces, envs.action_space, base="selfAttn_merge_srnn",
                 base_kwargs=dict(env_name=env_name, num_processes=1, num_mini_batch=1, seq_length=30)).to(dev)
    with torch.no_grad():
        pol.dist.fc_mean.bias.copy_(torch.tensor([0.3, -0.2]))
    return pol, envs


def test_wrapper_step_of_one_env_does_not_depend_on_the_batch():
    """cn_gst_wrapper_step of one env alone against the same env as one of 64: the wrapped spatial edges and the penalised reward are equal
    bit for bit over 40 steps, during which neighbours (and the env itself) end episodes and auto-reset."""
    from crowdnav_prediction_attngraph_amd.config import to_env_config
    from crowdnav_prediction_attngraph_amd.gst import PretextProcessor
    from crowdnav_prediction_attngraph_amd.hip import HipEnvBatch
    cfg_py = _gst_config(**{"env.time_limit": 5})                 # 20 steps: every env runs into its time limit, some collide before
    cfg = to_env_config(cfg_py, GST, 64, "train")
    E, dev = 64, torch.device("cuda", 0)
    env = HipEnvBatch(cfg, E, 11, device=dev)
    pred = _predictor()
    mk = lambda n: PretextProcessor(pred, n, env.H, int(cfg.predict_steps), float(cfg.robot_radius), float(cfg.human_radius),  # noqa: E731
                                    float(cfg.collision_penalty), dev)
    full, picks = mk(E), (0, 37, 63)
    alone = {k: mk(1) for k in picks}
    gen = torch.Generator(device="cuda").manual_seed(5)
    obs, rew = env.reset(), torch.zeros(E, device=dev)
    resets = torch.zeros(E, dtype=torch.int64, device=dev)
    valid = 0
    for t in range(40):
        raw = {k: v.clone() for k, v in obs.items()}
        rew_in = rew.clone()
        se, r = full.process(raw, rew_in.clone())
        for k in picks:
            se1, r1 = alone[k].process({n: v[k:k + 1].contiguous() for n, v in raw.items()}, rew_in[k:k + 1].clone())
            assert torch.equal(se1[0], se[k]), (t, k, float((se1[0] - se[k]).abs().max()))
            assert torch.equal(r1, r[k:k + 1]), (t, k)
        valid += int((se[:, :, 2:] != raw["spatial_edges"][:, :, 2:]).any())
        action = torch.empty(E, 2, device=dev).uniform_(-1.0, 1.0, generator=gen)
        obs, rew, done, info, _, _ = env.step(action)
        resets += done.long()
    assert valid >= 30                                            # predictions were written
    h = resets.cpu()
    assert int(h.sum()) - int(h[37]) > 0, "no neighbour ended an episode: the run does not cover a neighbour's reset"
    env.close()


def test_sequential_and_batched_evaluation_agree_with_the_gst_wrapper():
    from crowdnav_prediction_attngraph_amd.evaluation import evaluate, evaluate_batched
    cfg, pred, dev = _gst_config(), _predictor(), torch.device("cuda", 0)
    pol, envs = _policy(GST, cfg, pred)
    assert envs.edge_width == 12
    n = 20
    seq = evaluate(pol, envs, 1, dev, n, LOG, cfg, None, batch_invariant=True)
    bat = evaluate_batched(pol, GST, cfg, 7, n, device=dev, logging=LOG, batch_invariant=True, predictor=pred)
    print("sequential", seq)
    print("batched   ", bat)
    assert seq["episodes"] == bat["episodes"] == n
    for k in ("success_rate", "collision_rate", "timeout_rate", "collision_cases", "timeout_cases"):
        assert seq[k] == bat[k], (k, seq[k], bat[k])
    for k in ("nav_time", "path_length", "intrusion_ratio", "mean_reward"):
        assert seq[k] == pytest.approx(bat[k], rel=1e-6, abs=1e-6), (k, seq[k], bat[k])
    if seq["min_intrusion_dist"] == seq["min_intrusion_dist"]:
        assert seq["min_intrusion_dist"] == pytest.approx(bat["min_intrusion_dist"], rel=1e-9)
    assert seq["collision_rate"] + seq["timeout_rate"] + seq["success_rate"] == pytest.approx(1.0)
    fused = evaluate_batched(pol, GST, cfg, 7, n, device=dev, logging=LOG, predictor=pred)
    print("fused     ", fused)
    assert pol.rollout_gemm_mode == "fused" and fused["episodes"] == n
    for k in ("success_rate", "collision_rate", "timeout_rate"):
        assert abs(fused[k] - bat[k]) <= 2.0 / n + 1e-9, (k, fused[k], bat[k])


@pytest.mark.parametrize("env_name,over", [("CrowdSimVarNum-v0", {}), ("CrowdSimPred-v0", {"sim.predict_method": "const_vel"}), (GST, {})])
def test_bookkeeping_kernel_equals_the_torch_expression(env_name, over):
    """cn_eval_accumulate against the torch-op form on the same episodes; the polling stride does not matter; a rerun gives the same bits."""
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd.evaluation import _batch_invariant, _evaluate_batched
    cfg = C.non_randomized(**dict({"sim.human_num": 10, "env.test_size": 16}, **over))
    pred = _predictor() if env_name == GST else None
    pol, envs = _policy(env_name, cfg, pred)
    envs.close()
    dev = torch.device("cuda", 0)

    def run(**kw):
        per_env = {}
        with _batch_invariant(pol, True):
            m = _evaluate_batched(pol, env_name, cfg, 7, 20, dev, None, predictor=pred, per_env=per_env, **kw)
        return m, per_env
    m_k, k16 = run()
    m_t, tor = run(use_kernel=False)
    assert k16["cases"] == tor["cases"] == [0, 2, 4, 6, 8, 10, 12, 14]
    for key in ("outcome", "steps", "danger_steps"):
        assert k16[key] == tor[key], key
    assert all(o in (1, 2, 3) for o in k16["outcome"]) and sum(k16["danger_steps"]) > 0
    assert k16["ep_return"] == tor["ep_return"]
    for a, b in zip(k16["path_length"], tor["path_length"]):
        assert a == pytest.approx(b, rel=1e-6)
    for a, b in zip(k16["danger_sum"], tor["danger_sum"]):
        assert a == pytest.approx(b, rel=1e-12, abs=0.0)
    for k in ("success_rate", "collision_rate", "timeout_rate", "collision_cases", "timeout_cases", "nav_time", "intrusion_ratio", "mean_reward"):
        assert m_k[k] == m_t[k], k
    for poll in (1, 64, 16):                                # 16 again: a rerun
        m_p, per = run(poll_every=poll)
        assert per == k16, poll
        assert repr(m_p) == repr(m_k), poll


def _storage_tensors(r):
    out = {"obs/" + k: v for k, v in r.obs.items()}
    out.update(rewards=r.rewards, masks=r.masks, actions=r.actions, value_preds=r.value_preds, action_log_probs=r.action_log_probs,
               hxs=r.recurrent_hidden_states["human_node_rnn"])
    return out


def test_rollout_with_the_wrapper_writes_the_storage_in_place_with_the_same_bits(tmp_path):
    from crowdnav_prediction_attngraph_amd.policy import Policy
    from crowdnav_prediction_attngraph_amd.storage import RolloutStorage
    from crowdnav_prediction_attngraph_amd.trainer import EpisodeStats, collect_rollout, train
    from crowdnav_prediction_attngraph_amd.vec_env import make_vec_envs
    cfg, pred, dev = _gst_config(), _predictor(), torch.device("cuda", 0)
    E, T = 16, 6

    def setup():
        torch.manual_seed(425)
        envs = make_vec_envs(GST, 425, E, 0.99, None, dev, False, config=cfg, phase="train", pretext_wrapper=True, predictor=pred)
        pol = Policy(envs.observation_space.spaces, envs.action_space, base="selfAttn_merge_srnn",
                     base_kwargs=dict(env_name=GST, num_processes=E, num_mini_batch=2, seq_length=T, use_self_attn=True, sort_humans=True)).to(dev)
        r = RolloutStorage(T, E, envs.observation_space.spaces, envs.action_space, 128, 256)
        r.to(dev)
        obs = envs.reset_device()
        for k in r.obs:
            r.obs[k][0].copy_(obs[k].view_as(r.obs[k][0]) if k != "visible_masks" else obs[k].to(torch.bool))
        torch.cuda.manual_seed(99)
        return envs, pol, r, EpisodeStats(dev)

    envs, pol, r_new, st_new = setup()
    for _ in range(2):                                         # two rollouts: the second starts from the first one's last row
        collect_rollout(envs, pol, r_new, st_new)
        new = {k: v.clone() for k, v in _storage_tensors(r_new).items()}
        r_new.after_update()
    envs.close()

    envs, pol, r_old, st_old = setup()
    keys = ("robot_node", "temporal_edges", "spatial_edges", "detected_human_num")
    hx = r_old.recurrent_hidden_states["human_node_rnn"]
    hp = pol._hip_policy(E, dev)
    for _ in range(2):
        eps = torch.empty(T, E, 2, device=dev).normal_()
        for t in range(T):                                     # the copying loop collect_rollout ran before it wrote in place
            out = dict(value=r_old.value_preds[t], action=r_old.actions[t], logp=r_old.action_log_probs[t], hxs=hx[t + 1])
            hp.act({k: r_old.obs[k][t] for k in keys}, hx[t], r_old.masks[t], eps=eps[t], out=out)
            o, reward, done, info, ep_ret, ep_len = envs.step_device(r_old.actions[t])
            for k in keys:
                r_old.obs[k][t + 1].copy_(o[k].view_as(r_old.obs[k][t + 1]))
            r_old.obs["visible_masks"][t + 1].copy_(o["visible_masks"].to(torch.bool))
            r_old.rewards[t].copy_(reward.view(E, 1))
            r_old.masks[t + 1].copy_((done == 0).view(E, 1))
            st_old.update(done, info, ep_ret, ep_len)
        old = {k: v.clone() for k, v in _storage_tensors(r_old).items()}
        r_old.after_update()
    envs.close()
    assert set(new) == set(old) and "obs/visible_masks" in new
    for k in new:
        assert torch.equal(new[k], old[k]), k
    assert torch.equal(st_new.acc, st_old.acc)
    se = new["obs/spatial_edges"]
    assert bool((se[1:, :, :, 2:].abs() > 0).any()) and float(new["rewards"].abs().sum()) > 0

    # the public entry: train() with the wrapper, and a bit-exact resume (the checkpoint carries the wrapper's history)
    kw = dict(env_name=GST, pretext_wrapper=True, predictor=pred, num_processes=16, num_steps=6, config=cfg, log=None)
    d = str(tmp_path / "run")
    full, pol_full = train(num_updates=2, save_dir=d, save_interval=1, **kw)
    ck = os.path.join(d, "checkpoints", "00000.pt")
    assert os.path.isfile(ck) and "pretext" in torch.load(ck[:-3] + ".resume.pt", map_location="cpu")["env"]
    rest, pol_res = train(num_updates=2, resume=ck, **kw)
    assert [x["update"] for x in rest] == [1]
    for k in ("value_loss", "action_loss", "entropy", "episodes", "eprewmean"):
        assert full[1][k] == rest[0][k] and np.isfinite(full[1][k]), k
    for (k, x), (_, y) in zip(pol_full.state_dict().items(), pol_res.state_dict().items()):
        assert torch.equal(x, y), k
    with pytest.raises(ValueError):
        train(env_name="CrowdSimVarNum-v0", pretext_wrapper=True, num_processes=16, num_steps=6, num_updates=1, log=None)


def test_train_follows_config_use_wrapper():
    from crowdnav_prediction_attngraph_amd.trainer import train
    cfg, pred = _gst_config(**{"env.use_wrapper": True}), _predictor()
    kw = dict(env_name=GST, predictor=pred, num_processes=16, num_steps=6, num_updates=1, log=None)
    on, _ = train(config=cfg, **kw)
    explicit, _ = train(config=_gst_config(), pretext_wrapper=True, **kw)
    off, _ = train(config=_gst_config(), **kw)
    assert on[0]["value_loss"] == explicit[0]["value_loss"] != off[0]["value_loss"]


@pytest.mark.parametrize("env_name,wrapper", [("CrowdSimVarNum-v0", False), (GST, True)])
def test_evaluation_inside_train_leaves_the_run_alone(env_name, wrapper):
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd.evaluation import evaluate_batched
    from crowdnav_prediction_attngraph_amd.trainer import train
    pred = _predictor() if wrapper else None
    cfg = _gst_config() if wrapper else C.non_randomized(**{"sim.human_num": 10, "env.test_size": 16})
    kw = dict(env_name=env_name, num_processes=32, num_steps=8, num_updates=4, seed=5, config=cfg, log=None, lr=1e-3, pretext_wrapper=wrapper, predictor=pred)
    plain, pol_plain = train(**kw)
    with_eval, pol_eval = train(eval_interval=2, eval_cases=12, **kw)
    assert ["eval" in r for r in with_eval] == [False, True, False, True] and not any("eval" in r for r in plain)
    for a, b in zip(plain, with_eval):
        for k in a:
            if not k.endswith("_s") and k != "allreduce_ms":   # wall times differ
                assert a[k] == b[k], (a["update"], k, a[k], b[k])
    for (k, x), (_, y) in zip(pol_plain.state_dict().items(), pol_eval.state_dict().items()):
        assert torch.equal(x, y), k
    after = evaluate_batched(pol_eval, env_name, cfg, 5, 12, predictor=pred)
    last = with_eval[-1]["eval"]
    assert last["episodes"] == 12 and set(last) == set(after)
    for k in after:
        assert last[k] == after[k] or (last[k] != last[k] and after[k] != after[k]), (k, last[k], after[k])


class _ReplayPolicy(object):
    """Stands where the policy stands in evaluate(): returns the recorded actions one by one and notes the observation it is shown."""

    class base:
        human_num, human_node_rnn_size, human_human_edge_rnn_size = 8, 128, 256

    def __init__(self, actions):
        self.actions, self.edges = actions, []

    def act(self, obs, hxs, masks, deterministic=False):
        self.edges.append(obs["spatial_edges"][0].cpu().numpy().copy())
        return None, torch.from_numpy(self.actions[len(self.edges) - 1]).view(1, 2).cuda(), None, hxs


@pytest.mark.parametrize("tag", ["fast", "still"])
def test_replay_of_the_reference_evaluation_with_the_gst_wrapper(tag):
    """tests/golden/ref_eval_predgst_h8.npz: the reference's rl.evaluation.evaluate on CrowdSimPredRealGST-v0 + VecPretextNormalize (shipped
    predictor weights, wrapper reset() included), 8 episodes over test cases 0 2 4 6 8 0 2 4, a rule policy whose actions were recorded.
    Replaying the actions, evaluate() on the one-env wrapped vec-env and evaluate_batched() must give the reference's episodes."""
    from crowdnav_prediction_attngraph_amd.evaluation import _evaluate_batched, evaluate
    from crowdnav_prediction_attngraph_amd.gst import GSTPredictor
    from crowdnav_prediction_attngraph_amd.vec_env import make_vec_envs
    z = np.load(os.path.join(GOLDEN, "ref_eval_predgst_h8.npz"))
    meta = json.loads(str(z["meta"]))
    w = np.load(os.path.join(GOLDEN, "gst_real_e4_h20.npz"))
    pred = GSTPredictor()
    pred.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("w/")})
    pred = pred.to("cuda")
    H, n, seed, dev = meta["human_num"], meta["episodes"], meta["seed"], torch.device("cuda", 0)
    cfg = _gst_config(**{"sim.human_num": H, "env.test_size": meta["test_size"], "env.use_wrapper": True})
    ref = {k: z["%s_%s" % (tag, k)] for k in ("actions", "edges", "masks", "outcome", "steps", "path_length", "danger_steps", "danger_dists", "reward")}
    logged = meta["runs"][tag]["logged"]
    first = np.concatenate([[0], np.cumsum(ref["steps"])])
    assert set(ref["outcome"].tolist() + z["fast_outcome"].tolist() + z["still_outcome"].tolist()) == {1, 2, 3} and ref["danger_steps"].sum() > 0

    def check_edges(got, want, mask, what):
        # current positions and the env's own placeholder futures: float32 values below 16 of the same float64 trajectory, i.e. equal up to
        # a rounding flip of 1e-6 (bound 1e-5); predictions where the wrapper wrote them: SURVEY 8c's 1e-4
        np.testing.assert_allclose(got[:, :2], want[:, :2], rtol=0, atol=1e-5, err_msg=str(what))
        m = np.repeat(mask[:, None], got.shape[1] - 2, axis=1)
        np.testing.assert_allclose(got[:, 2:][m], want[:, 2:][m], rtol=0, atol=1e-4, err_msg=str(what))
        np.testing.assert_allclose(got[:, 2:][~m], want[:, 2:][~m], rtol=0, atol=1e-5, err_msg=str(what))

    def check_metrics(m):
        print(tag, m)
        assert m["collision_cases"] == logged["collision_cases"] and m["timeout_cases"] == logged["timeout_cases"]
        for k in ("success_rate", "collision_rate", "timeout_rate", "nav_time", "path_length", "intrusion_ratio", "min_intrusion_dist"):
            assert "%.2f" % m[k] == logged[k], (k, m[k], logged[k])
        assert m["mean_reward"] == pytest.approx(float(np.mean(ref["reward"])), abs=1e-4)

    # ---- sequential: the reference-shaped loop over ONE env behind the wrapper ----
    envs = make_vec_envs(GST, seed, 1, 0.99, None, dev, True, config=cfg, pretext_wrapper=True, predictor=pred)
    pol = _ReplayPolicy(ref["actions"])
    m_seq = evaluate(pol, envs, 1, dev, n, LOG, cfg, None)
    assert len(pol.edges) == len(ref["actions"]), "the episodes did not take the reference's number of steps"
    check_metrics(m_seq)
    for i, got in enumerate(pol.edges):
        check_edges(got, ref["edges"][i], ref["masks"][i], ("sequential", i))

    # ---- batched: the five distinct cases as one batch ----
    cases = sorted(set(meta["cases"]))
    ep_of = [meta["cases"].index(c) for c in cases]              # env e replays the first recorded episode of its case
    seen = []

    def act_fn(t, obs):
        a = np.zeros((len(cases), 2), np.float32)
        for e, k in enumerate(ep_of):
            if t < ref["steps"][k]:
                a[e] = ref["actions"][first[k] + t]
        seen.append(obs["spatial_edges"].cpu().numpy().copy())
        return torch.from_numpy(a).cuda()
    per_env = {}
    m_bat = _evaluate_batched(None, GST, cfg, seed, n, dev, LOG, predictor=pred, act_fn=act_fn, per_env=per_env)
    check_metrics(m_bat)
    assert per_env["cases"] == cases
    for e, k in enumerate(ep_of):
        assert per_env["outcome"][e] == ref["outcome"][k] and per_env["steps"][e] == ref["steps"][k] and per_env["danger_steps"][e] == ref["danger_steps"][k]
        assert per_env["path_length"][e] == pytest.approx(ref["path_length"][k], rel=1e-6)
        for t in range(ref["steps"][k]):
            check_edges(seen[t][e], ref["edges"][first[k] + t], ref["masks"][first[k] + t], ("batched", e, t))
    # the Danger distances, episode by episode in step order
    d0 = np.concatenate([[0], np.cumsum(ref["danger_steps"])])
    for e, k in enumerate(ep_of):
        assert per_env["danger_sum"][e] == pytest.approx(float(ref["danger_dists"][d0[k]:d0[k + 1]].sum()), rel=1e-6, abs=1e-9)
