"""The reference's own train.py / test.py / collect_data.py against dropin/, through the interface they expect of it
(tests/golden/dropin_surface.json, names read off the scripts' syntax trees by tests/golden/make_golden_dropin_surface.py):

1. every `from ... import name` of the three scripts resolves with dropin/ first on sys.path;
2. every attribute train.py reads off the objects the shims hand out exists on the mirrors."""
import importlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "dropin")
with open(os.path.join(ROOT, "tests", "golden", "dropin_surface.json")) as _f:
    SURFACE = json.load(_f)

THIRD_PARTY = {"os", "shutil", "time", "collections", "numpy", "torch", "pandas", "matplotlib", "logging", "argparse", "sys", "importlib", "copy", "tqdm"}


@pytest.fixture()
def dropin_path():
    saved, mods = list(sys.path), set(sys.modules)
    sys.path.insert(0, DROPIN)
    yield
    sys.path[:] = saved
    for m in set(sys.modules) - mods:
        if m.split(".")[0] in ("rl", "crowd_sim", "crowd_nav", "arguments"):
            del sys.modules[m]


@pytest.mark.parametrize("script", ["train.py", "test.py", "collect_data.py"])
def test_every_import_of_the_reference_scripts_resolves_against_dropin(script, dropin_path):
    checked = 0
    for module, names in SURFACE["import_from"][script]:
        if module.split(".")[0] not in THIRD_PARTY:
            mod = importlib.import_module(module)
            assert os.path.abspath(mod.__file__).startswith(DROPIN), "%s resolved outside dropin/: %s" % (module, mod.__file__)
            for name in names:
                if name == "*":
                    assert getattr(mod, "__all__", None), "%s: `import *` needs __all__" % module
                    for n in mod.__all__:
                        assert hasattr(mod, n)
                else:
                    assert hasattr(mod, name) or importlib.import_module(module + "." + name), (module, name)
                checked += 1
    assert checked >= (3 if script == "collect_data.py" else 6)


def test_attribute_surface_of_train_py_exists_on_the_mirrors(dropin_path):
    """envs.* / actor_critic.* / rollouts.* / agent.* / algo_args.* / config.* as train.py reads them (:85-135,148,162-210)."""
    from arguments import get_args
    from crowdnav_prediction_attngraph_amd.policy import Policy, make_spaces
    from crowdnav_prediction_attngraph_amd.ppo import PPO
    from crowdnav_prediction_attngraph_amd.storage import RolloutStorage
    from tests.oracle_vec_env import OracleVecEnv
    from crowdnav_prediction_attngraph_amd.vec_env import BatchedCrowdSim
    old = sys.argv
    sys.argv = ["train.py", "--no-cuda", "--env-name", "CrowdSimVarNum-v0"]
    try:
        args = get_args()
        from crowd_nav.configs.config import Config
        config = Config()
    finally:
        sys.argv = old
    ob_space, act_space = make_spaces(20, 2)
    pol = Policy(ob_space.spaces, act_space, base_kwargs=args, base=config.robot.policy)
    ro = RolloutStorage(args.num_steps, args.num_processes, ob_space.spaces, act_space, args.human_node_rnn_size, args.human_human_edge_rnn_size)
    agent = PPO(pol, args.clip_param, args.ppo_epoch, args.num_mini_batch, args.value_loss_coef, args.entropy_coef, lr=args.lr, eps=args.eps,
                max_grad_norm=args.max_grad_norm)
    objs = {"actor_critic": pol, "rollouts": ro, "agent": agent, "algo_args": args, "config": config, "env_config": config}
    chains = {tuple(c) for c in SURFACE["train_py_attr_chains"] if c[0] in set(objs) | {"envs"}}
    assert len(chains) > 40
    for chain in sorted(chains):
        if chain[0] == "envs":
            for cls in (BatchedCrowdSim, OracleVecEnv):      # the product's vec-env and the test stand-in expose the same surface
                assert hasattr(cls, chain[1]) or chain[1] in ("observation_space", "action_space"), chain
            continue
        if chain[:2] == ("agent", "optimizer") and chain[2:] == ("lr",):
            continue                                           # only read when algo == 'acktr' (train.py:150)
        cur = objs[chain[0]]
        for a in chain[1:]:
            assert hasattr(cur, a), "train.py reads %s but %r has no attribute %r" % (".".join(chain), type(cur).__name__, a)
            cur = getattr(cur, a)
            if callable(cur) and not isinstance(cur, torch.nn.Module):
                break
