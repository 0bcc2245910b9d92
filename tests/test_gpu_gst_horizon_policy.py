"""-m gpu: the GST-predictor policy at sim.predict_steps = 3 -- train() with the wrapper in the loop, checkpoint and bit-exact resume (the
wrapper's history included), sequential against batched evaluation, and the two refusals: eight steps with the attention policy (edge width 18),
and a predictor whose pred_len is not the env's predict_steps."""
import logging
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import gst_horizon_util as HU  # noqa: E402

GST = "CrowdSimPredRealGST-v0"
LOG = logging.getLogger("gst-horizon-test")


def _config(P, **over):
    from crowdnav_prediction_attngraph_amd import config as C
    return C.non_randomized(**dict({"sim.human_num": 10, "sim.predict_method": "inferred", "sim.predict_steps": P, "env.test_size": 16}, **over))


def test_train_checkpoint_and_resume_with_three_predicted_steps(tmp_path):
    from crowdnav_prediction_attngraph_amd.trainer import train
    cfg, pred = _config(3), HU.model(5, 3).cuda()
    kw = dict(env_name=GST, pretext_wrapper=True, predictor=pred, num_processes=8, num_steps=6, config=cfg, log=None)
    d = str(tmp_path / "run")
    full, pol_full = train(num_updates=2, save_dir=d, save_interval=1, **kw)
    ck = os.path.join(d, "checkpoints", "00000.pt")
    side = torch.load(ck[:-3] + ".resume.pt", map_location="cpu")
    assert "pretext" in side["env"] and tuple(side["env"]["pretext"]["traj"].shape) == (5, 8, 10, 2)
    assert tuple(side["rollout0"]["obs"]["spatial_edges"].shape) == (8, 10, 8)
    rest, pol_res = train(num_updates=2, resume=ck, **kw)
    assert [x["update"] for x in rest] == [1]
    for k in ("value_loss", "action_loss", "entropy", "episodes", "eprewmean"):
        assert full[1][k] == rest[0][k] and np.isfinite(full[1][k]), k
    for (k, x), (_, y) in zip(pol_full.state_dict().items(), pol_res.state_dict().items()):
        assert torch.equal(x, y), k


def test_sequential_and_batched_evaluation_agree_with_three_predicted_steps():
    from crowdnav_prediction_attngraph_amd.evaluation import evaluate, evaluate_batched
    from crowdnav_prediction_attngraph_amd.policy import Policy
    from crowdnav_prediction_attngraph_amd.vec_env import make_vec_envs
    cfg, pred, dev = _config(3), HU.model(5, 3).cuda(), torch.device("cuda", 0)
    envs = make_vec_envs(GST, 7, 1, 0.99, None, dev, True, config=cfg, pretext_wrapper=True, predictor=pred)
    assert envs.edge_width == 8
    torch.manual_seed(3)
    pol = Policy(envs.observation_space.spaces, envs.action_space, base="selfAttn_merge_srnn",
                 base_kwargs=dict(env_name=GST, num_processes=1, num_mini_batch=1, seq_length=30, predict_steps=3)).to(dev)
    with torch.no_grad():
        pol.dist.fc_mean.bias.copy_(torch.tensor([0.3, -0.2]))
    n = 8
    seq = evaluate(pol, envs, 1, dev, n, LOG, cfg, None, batch_invariant=True)
    bat = evaluate_batched(pol, GST, cfg, 7, n, device=dev, logging=LOG, batch_invariant=True, predictor=pred)
    print("sequential", seq)
    print("batched   ", bat)
    assert seq["episodes"] == bat["episodes"] == n
    for k in ("success_rate", "collision_rate", "timeout_rate", "collision_cases", "timeout_cases"):
        assert seq[k] == bat[k], (k, seq[k], bat[k])
    for k in ("nav_time", "path_length", "intrusion_ratio", "mean_reward"):
        assert seq[k] == pytest.approx(bat[k], rel=1e-6, abs=1e-6), (k, seq[k], bat[k])


def test_the_two_refusals_of_the_policy_path():
    from crowdnav_prediction_attngraph_amd.trainer import train
    from crowdnav_prediction_attngraph_amd.vec_env import make_vec_envs
    kw = dict(env_name=GST, pretext_wrapper=True, num_processes=8, num_steps=6, num_updates=1, log=None)
    with pytest.raises(NotImplementedError, match=r"predict_steps = 8 .* width 18, .* at most 16"):
        train(config=_config(8), predictor=HU.model(5, 8).cuda(), **kw)
    with pytest.raises(ValueError, match=r"pred_len = 5 .*predict_steps is 3"):
        train(config=_config(3), predictor=HU.model(5, 5).cuda(), **kw)
    # the wrapper itself takes eight steps: it is the attention policy's edge width that stops at 16
    envs = make_vec_envs(GST, 425, 4, 0.99, None, torch.device("cuda", 0), False, config=_config(8), pretext_wrapper=True, predictor=HU.model(5, 8).cuda())
    obs = envs.reset_device()
    assert tuple(obs["spatial_edges"].shape) == (4, 10, 18) and bool(torch.isfinite(obs["spatial_edges"]).all())
    envs.close()
