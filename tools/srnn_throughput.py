#!/usr/bin/env python3
"""Throughput of the DS-RNN baseline (Policy(base='srnn')) on the GPU at the bench shape.

    python tools/srnn_throughput.py --out profiles/srnn_throughput.json

Protocol of tools/gst_throughput.py: every variant is warmed up first; a window is wall clock around repeated work that ends in
torch.cuda.synchronize() and lasts at least --window seconds; the variants of a group alternate inside this one process, --repeats windows
each; median, minimum and maximum are reported.
  (a) forward:  one rollout forward of --envs x --humans through cn_srnn_act, arithmetic modes 'bf16x3' and 'fp32', and the same forward through
                the mirror's torch ops (SRNNBase.forward_sequence, no autograd) on the same device;
  (b) rollout:  env-steps per second of (forward -> simulator step), trainer.collect_rollout over --steps steps;
  (c) update:   seconds of one PPO.update at T = --steps with envs / 2 envs per minibatch (autograd producer, --ppo-epoch epochs).
Beside them the two floors of the edge-GRU kernel at that shape, from its own FLOP and byte counts (see `floors` in the output).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--humans", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--ppo-epoch", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0)
    a = ap.parse_args()
    import torch

    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd.policy import Policy
    from crowdnav_prediction_attngraph_amd.ppo import PPO
    from crowdnav_prediction_attngraph_amd.storage import RolloutStorage
    from crowdnav_prediction_attngraph_amd.trainer import bootstrap_value, collect_rollout
    from crowdnav_prediction_attngraph_amd.vec_env import make_vec_envs

    assert torch.cuda.is_available(), "srnn_throughput.py measures the GPU paths"
    dev = torch.device("cuda", torch.cuda.current_device())
    E, H, T = a.envs, a.humans, a.steps
    env_name = "CrowdSimVarNum-v0"
    cfg = C.Config(**{"sim.human_num": H})
    torch.manual_seed(425)
    envs = make_vec_envs(env_name, 425, E, 0.99, None, dev, False, config=cfg, phase="train")
    pol = Policy(envs.observation_space.spaces, envs.action_space, base="srnn",
                 base_kwargs=dict(env_name=env_name, num_processes=E, num_mini_batch=2, seq_length=T)).to(dev)
    ro = RolloutStorage(T, E, envs.observation_space.spaces, envs.action_space, 128, 256)
    ro.to(dev)
    ro.materialize_edge_rnn()
    obs = envs.reset_device()
    for k in ro.obs:
        ro.obs[k][0].copy_(obs[k].view_as(ro.obs[k][0]) if k != "visible_masks" else obs[k].to(torch.bool))

    def window(fn):
        """calls of fn until the window is full -> seconds per call"""
        torch.cuda.synchronize()
        t0, n = time.perf_counter(), 0
        while True:
            fn()
            n += 1
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= a.window:
                return dt / n

    def measure(variants, warm=2):
        for fn in variants.values():
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
        secs = {k: [] for k in variants}
        for _ in range(a.repeats):
            for k, fn in variants.items():
                secs[k].append(window(fn))
        return {k: {"s_median": statistics.median(v), "s_min": min(v), "s_max": max(v), "windows": v} for k, v in secs.items()}

    out = {"device": torch.cuda.get_device_name(0), "envs": E, "humans": H, "steps": T, "edge_width": 2, "window_s": a.window, "repeats": a.repeats}

    # a few rollouts first: the forwards below run on a recurrent state and observations that training would see
    for _ in range(2):
        collect_rollout(envs, pol, ro)
        ro.after_update()
    f_obs = {k: ro.obs[k][0] for k in ("robot_node", "temporal_edges", "spatial_edges", "detected_human_num")}
    node, edge, masks = ro.recurrent_hidden_states["human_node_rnn"][0], ro.recurrent_hidden_states["human_human_edge_rnn"][0], ro.masks[0]
    eps = torch.randn(E, 2, device=dev)
    h = pol._hip_srnn(E, dev)
    bufs = dict(value=torch.empty(E, 1, device=dev), action=torch.empty(E, 2, device=dev), logp=torch.empty(E, 1, device=dev),
                hxs=torch.empty(E, 1, 128, device=dev), edge_hxs=torch.empty(E, H + 1, 256, device=dev))

    def fwd_hip(mode, reps=20):
        def fn():
            h.set_gemm_mode(mode)
            for _ in range(reps):
                h.act(f_obs, node, edge, masks, eps=eps, out=bufs)
        return fn, reps

    def fwd_torch():
        with torch.no_grad():
            v, feat, _, _ = pol.base.forward_sequence(f_obs, node, edge, masks, 1, E)
            mean = pol.dist.fc_mean(feat)
            pol._log_prob(mean, pol.dist.logstd(torch.zeros_like(mean)).exp(), mean)

    (f3, reps), (f0, _) = fwd_hip("bf16x3"), fwd_hip("fp32")
    m = measure({"hip_bf16x3": f3, "hip_fp32": f0, "torch_ops": fwd_torch})
    for k in ("hip_bf16x3", "hip_fp32"):
        for q in ("s_median", "s_min", "s_max"):
            m[k][q] /= reps
        m[k]["windows"] = [x / reps for x in m[k]["windows"]]
    h.set_gemm_mode("bf16x3")
    out["forward"] = m

    r = measure({"collect_rollout": lambda: (collect_rollout(envs, pol, ro), ro.after_update())}, warm=1)["collect_rollout"]
    out["rollout"] = dict(r, env_steps_per_s_median=T * E / r["s_median"], env_steps_per_s_min=T * E / r["s_max"], env_steps_per_s_max=T * E / r["s_min"])

    agent = PPO(pol, 0.2, a.ppo_epoch, 2, 0.5, 0.0, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
    collect_rollout(envs, pol, ro)
    ro.compute_returns(bootstrap_value(pol, ro), True, 0.99, 0.95, False)
    u = measure({"update": lambda: agent.update(ro)}, warm=1)["update"]
    out["update"] = dict(update_s_median=u["s_median"], update_s_min=u["s_min"], update_s_max=u["s_max"], windows=u["windows"], ppo_epoch=a.ppo_epoch,
                         envs_per_minibatch=E // 2, optimiser_steps=2 * a.ppo_epoch, peak_memory_gb=torch.cuda.max_memory_allocated() / 2 ** 30)

    # floors of the edge-GRU kernel at this shape, from its own counts
    rows = E * (H + 1)
    flop_hh, flop_ih = 2.0 * rows * 256 * 768, 2.0 * rows * 64 * 768
    state_bytes = 2.0 * rows * 256 * 4                      # hidden state read + write
    tiles = -(-E // 64) + -(-E * H // 64)
    out["floors"] = {
        "edge_rows": rows, "algorithmic_gflop": (flop_hh + flop_ih) / 1e9,
        "mfma_floor_us_all_bf16x3_at_833_tflops": (flop_hh + flop_ih) / 833e12 * 1e6,
        "mfma_floor_us_as_built": (flop_hh / 833e12 + flop_ih / 157.3e12) * 1e6,   # W_hh split at the three-pass ceiling, W_ih on the fp32 MFMA
        "state_bytes_mb": state_bytes / 1e6, "state_floor_us_at_8_tb_s": state_bytes / 8.0e12 * 1e6,
        "state_bytes_with_epilogue_reread_mb": 1.5 * state_bytes / 1e6,
        "weight_stream_l2_gb": tiles * (2 * 768 * 256 * 2 + 768 * 64 * 4) / 1e9, "tiles": tiles,
    }
    envs.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
