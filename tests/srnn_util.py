"""Shared helpers of the DS-RNN (base='srnn') tests: fixtures of tests/golden/make_golden_srnn.py -> policies, observations, storages."""
import glob
import json
import os

import numpy as np
import torch

from crowdnav_prediction_attngraph_amd.policy import Policy, make_spaces
from crowdnav_prediction_attngraph_amd.storage import RolloutStorage
from tests import policy_util as PU
from tests.golden_util import GOLDEN

OBS_KEYS = ("robot_node", "temporal_edges", "spatial_edges", "detected_human_num")
ACT_CASES = sorted(glob.glob(os.path.join(GOLDEN, "srnn_act_*.npz")))
SEQ_CASES = sorted(glob.glob(os.path.join(GOLDEN, "srnn_seq_*.npz")))
ROLLOUT_CASES = sorted(glob.glob(os.path.join(GOLDEN, "srnn_rollout_*.npz")))
DEAD = ("base.humanNodeRNN.edge_embed.", "base.human_node_final_linear.", "base.spatial_linear.")


def case_id(path):
    return os.path.basename(path)[5:-4]


def load(path):
    z = np.load(path)
    return z, json.loads(str(z["meta"]))


def policy(meta, E, nmb=1, T=1, formula=True):
    ob_space, act_space = make_spaces(meta["H"], meta["D"])
    pol = Policy(ob_space.spaces, act_space, base="srnn", base_kwargs=dict(env_name=meta["env_name"], num_processes=E, num_mini_batch=nmb, seq_length=T))
    if formula:
        sd = PU.formula_state_dict({k: tuple(v) for k, v in meta["shapes"].items()})
        pol.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return pol, ob_space, act_space


def fill_rollouts(z, meta, ob_space, act_space):
    """The fixture's rollout in a RolloutStorage: observations, recorded actions / values / log-probs, the node state of every row and the
    edge state of rows 0 and T (the rows the update and the next rollout read)."""
    T, E, H = meta["T"], meta["E"], meta["H"]
    ro = RolloutStorage(T, E, ob_space.spaces, act_space, 128, 256)
    for k in OBS_KEYS:
        ro.obs[k][0].copy_(torch.from_numpy(z["obs0_" + k]))
    ro.recurrent_hidden_states["human_node_rnn"][0].copy_(torch.from_numpy(z["hxs_node"][0]))
    ro.materialize_edge_rnn()[0].copy_(torch.from_numpy(z["hxs_edge0"]))
    for s in range(T):
        nxt = {k: torch.from_numpy(z["obs%d_%s" % (s + 1, k)]) for k in OBS_KEYS}
        nxt["visible_masks"] = torch.zeros(E, H, dtype=torch.bool)
        edge = torch.from_numpy(z["hxs_edge_last"]) if s == T - 1 else torch.full((E, H + 1, 256), float(s + 1))
        hx = {"human_node_rnn": torch.from_numpy(z["hxs_node"][s + 1]), "human_human_edge_rnn": edge}
        masks = torch.from_numpy(np.where(z["dones"][s], 0.0, 1.0).astype(np.float32).reshape(E, 1))
        ro.insert(nxt, hx, torch.from_numpy(z["actions"][s]), torch.from_numpy(z["logp"][s]), torch.from_numpy(z["values"][s]),
                  torch.from_numpy(z["rewards"][s]), masks, torch.ones(E, 1))
    return ro
