#!/usr/bin/env python3
"""Throughput of the DS-RNN baseline (Policy(base='srnn')) on the GPU at the bench shape.

    python tools/srnn_throughput.py --out profiles/srnn_throughput.json [--parent-dir DIR] [--legs forward,rollout,update,edge_seq]

Protocol of tools/gst_throughput.py: every variant is warmed up first; a window is wall clock around repeated work that ends in
torch.cuda.synchronize() and lasts at least --window seconds; the variants of a group alternate inside this one process, --repeats windows
each; median, minimum and maximum are reported.
  (a) forward:  one rollout forward of --envs x --humans through cn_srnn_act, arithmetic modes 'bf16x3' and 'fp32', and the same forward through
                the mirror's torch ops (SRNNBase.forward_sequence, no autograd) on the same device;
  (b) rollout:  env-steps per second of (forward -> simulator step), trainer.collect_rollout over --steps steps;
  (c) update:   seconds of one PPO.update at T = --steps with envs / 2 envs per minibatch (autograd producer, --ppo-epoch epochs).  With
                --parent-dir (a checkout of the parent commit with its library built) the leg follows tools/eval_throughput.py instead: the
                parent's tree and this one run as child processes of this one, alternating, --rounds times; each child warms up once and
                times --update-repeats updates (host clock around an update that ends in synchronize) and reports its peak memory.
                "Faster" = the two [min..max] intervals do not overlap;
  (d) edge_seq: the edge-GRU sequence of one minibatch (T = --steps, N = envs / 2) through cn_srnn_seq_fwd and cn_srnn_seq_bwd (BPTT + weight
                gradients), event-bracketed medians in both arithmetic modes, beside their MFMA and byte floors from the kernels' own counts.
Beside them the two floors of the edge-GRU kernel at that shape, from its own FLOP and byte counts (see `floors` in the output).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--worker" not in sys.argv:           # a worker imports the package of the tree it was started in (PYTHONPATH)
    sys.path.insert(0, ROOT)


def update_worker(a):
    """One child of the update leg, in whichever tree PYTHONPATH names: a rollout at the bench shape, one warm-up update, then timed ones."""
    import torch

    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd.policy import Policy, SRNNBase
    from crowdnav_prediction_attngraph_amd.ppo import PPO
    from crowdnav_prediction_attngraph_amd.storage import RolloutStorage
    from crowdnav_prediction_attngraph_amd.trainer import bootstrap_value, collect_rollout
    from crowdnav_prediction_attngraph_amd.vec_env import make_vec_envs
    dev = torch.device("cuda", 0)
    E, H, T = a.envs, a.humans, a.steps
    env_name = "CrowdSimVarNum-v0"
    torch.manual_seed(425)
    envs = make_vec_envs(env_name, 425, E, 0.99, None, dev, False, config=C.Config(**{"sim.human_num": H}), phase="train")
    pol = Policy(envs.observation_space.spaces, envs.action_space, base="srnn",
                 base_kwargs=dict(env_name=env_name, num_processes=E, num_mini_batch=2, seq_length=T)).to(dev)
    ro = RolloutStorage(T, E, envs.observation_space.spaces, envs.action_space, 128, 256)
    ro.to(dev)
    ro.materialize_edge_rnn()
    obs = envs.reset_device()
    for k in ro.obs:
        ro.obs[k][0].copy_(obs[k].view_as(ro.obs[k][0]) if k != "visible_masks" else obs[k].to(torch.bool))
    for _ in range(2):
        collect_rollout(envs, pol, ro)
        ro.after_update()
    agent = PPO(pol, 0.2, a.ppo_epoch, 2, 0.5, 0.0, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
    collect_rollout(envs, pol, ro)
    ro.compute_returns(bootstrap_value(pol, ro), True, 0.99, 0.95, False)
    losses = agent.update(ro)           # warm-up: code objects, allocator
    times = []
    for _ in range(a.update_repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = agent.update(ro)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    envs.close()
    print("RESULT " + json.dumps(dict(times_s=times, peak_memory_gb=torch.cuda.max_memory_allocated() / 2 ** 30, last_losses=list(losses),
                                      train_edge_kernels=getattr(SRNNBase, "train_edge_kernels", None))))


def update_child(tree, a):
    env = dict(os.environ, PYTHONPATH=tree)
    env.pop("CN_HIP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "update", "--envs", str(a.envs), "--humans", str(a.humans), "--steps", str(a.steps),
           "--ppo-epoch", str(a.ppo_epoch), "--update-repeats", str(a.update_repeats)]
    p = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError("update worker in %s failed (%d):\n%s" % (tree, p.returncode, p.stderr[-3000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def update_ab(a):
    sides = [("parent", os.path.abspath(a.parent_dir)), ("tree", ROOT)]
    got = {name: dict(times=[], peak=[], flag=None) for name, _ in sides}
    for _ in range(a.rounds):
        for name, tree in sides:         # alternating: both sides see the same box in the same minutes
            r = update_child(tree, a)
            got[name]["times"] += r["times_s"]
            got[name]["peak"].append(r["peak_memory_gb"])
            got[name]["flag"] = r["train_edge_kernels"]
    rec = {}
    for name, g in got.items():
        t = g["times"]
        rec[name] = dict(update_s_median=statistics.median(t), update_s_min=min(t), update_s_max=max(t), n=len(t), all_s=t,
                         peak_memory_gb=max(g["peak"]), train_edge_kernels=g["flag"])
    rec["faster"] = dict(rule="the [min..max] intervals of the two sides do not overlap", met=rec["tree"]["update_s_max"] < rec["parent"]["update_s_min"])
    rec["peak_memory"] = dict(rule="this tree's peak does not exceed the parent's", met=rec["tree"]["peak_memory_gb"] <= rec["parent"]["peak_memory_gb"])
    return rec


def edge_seq_leg(torch, pol, dev, E, H, D, T, repeats=7):
    """The edge-GRU sequence of one minibatch through the two calls, on synthetic inputs in the simulator's ranges (timing does not read them)."""
    N = E // 2
    g = torch.Generator(device=dev).manual_seed(3)
    te = torch.rand(T * N, 2, device=dev, generator=g) * 2 - 1
    se = torch.rand(T * N, H, D, device=dev, generator=g) * 8 - 4
    se[:, H // 2:] = 15.0
    e0 = torch.rand(N, H + 1, 256, device=dev, generator=g) - 0.5
    m = (torch.rand(T * N, 1, device=dev, generator=g) > 0.02).float()
    hip = pol._hip_handle(E, dev)
    grads = [torch.empty_like(p) for p in pol.base._edge_parameters()]
    d_e0 = torch.empty_like(e0)
    ws = torch.empty(hip.seq_workspace_bytes(T, N) // 4, device=dev)
    rows = T * N * (H + 1)
    out = {"T": T, "N": N, "row_steps": rows, "workspace_gb": ws.numel() * 4 / 2 ** 30}
    for mode in ("bf16x3", "fp32"):
        hip.set_gemm_mode(mode)
        tf, tb = [], []
        for i in range(repeats + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            h_all, _ = hip.seq_fwd(te, se, e0, m, T, N, workspace=ws)
            ev[1].record()
            d_h = h_all             # any gradient: the kernels' time does not depend on the values
            hip.seq_bwd(te, se, e0, m, h_all, d_h, ws, T, N, grads, d_e0)
            ev[2].record()
            torch.cuda.synchronize()
            if i:                   # the first pass is the warm-up
                tf.append(ev[0].elapsed_time(ev[1]))
                tb.append(ev[1].elapsed_time(ev[2]))
        out[mode] = dict(fwd_ms_median=statistics.median(tf), fwd_ms_min=min(tf), fwd_ms_max=max(tf), bwd_wgrad_ms_median=statistics.median(tb),
                         bwd_wgrad_ms_min=min(tb), bwd_wgrad_ms_max=max(tb))
    hip.set_gemm_mode("bf16x3")
    # floors from the kernels' own counts, per row and step; 833 TFLOPS = the three-pass ceiling of bf16x3, 157.3 TFLOPS = fp32 MFMA, 8 TB/s HBM
    hh, ih = 2.0 * 768 * 256, 2.0 * 768 * 64
    wgrad = 2.0 * 768 * 256 + 2.0 * 1024 * 80 + 2.0 * 64 * 16           # as issued: the [e | 1] operand padded to 80, [x | 1] to 16 columns
    fwd_bytes = (1 + 1 + 1 + 4) * 1024 + 256 + 4 * D                     # h read, epilogue re-read, h written, gates written, embedding, x
    bpt_bytes = (1 + 1 + 1 + 4 + 4 + 1 + 4 + 2) * 1024 + 2 * 256         # d_h, carry, h_prev, gates read / written, g z, gates staged, carry r / w
    wg_bytes = (3 + 6) * 1024 + (4 * 1024 + 8 * 256) + 256 + 4 * D       # D once per product, the shared operand once per 128-column slice
    out["floors_ms"] = {
        "fwd_mfma_bf16x3": rows * (hh / 833e12 + ih / 157.3e12) * 1e3, "fwd_mfma_fp32": rows * (hh + ih) / 157.3e12 * 1e3,
        "fwd_bytes_at_8_tb_s": rows * fwd_bytes / 8e12 * 1e3,
        "bwd_mfma_bf16x3": rows * (hh / 833e12 + (ih + wgrad) / 157.3e12) * 1e3, "bwd_mfma_fp32": rows * (hh + ih + wgrad) / 157.3e12 * 1e3,
        "bwd_bytes_at_8_tb_s": rows * (bpt_bytes + wg_bytes) / 8e12 * 1e3,
        "bytes_per_row_step": {"fwd": fwd_bytes, "bptt": bpt_bytes, "wgrad": wg_bytes},
    }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="forward,rollout,update,edge_seq")
    ap.add_argument("--parent-dir", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--update-repeats", type=int, default=2)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--humans", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--ppo-epoch", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0)
    a = ap.parse_args()
    if a.worker:
        return update_worker(a)
    legs = set(a.legs.split(","))
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
    h = pol._hip_handle(E, dev)
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

    if "forward" in legs:
        (f3, reps), (f0, _) = fwd_hip("bf16x3"), fwd_hip("fp32")
        m = measure({"hip_bf16x3": f3, "hip_fp32": f0, "torch_ops": fwd_torch})
        for k in ("hip_bf16x3", "hip_fp32"):
            for q in ("s_median", "s_min", "s_max"):
                m[k][q] /= reps
            m[k]["windows"] = [x / reps for x in m[k]["windows"]]
        h.set_gemm_mode("bf16x3")
        out["forward"] = m

    if "rollout" in legs:
        r = measure({"collect_rollout": lambda: (collect_rollout(envs, pol, ro), ro.after_update())}, warm=1)["collect_rollout"]
        out["rollout"] = dict(r, env_steps_per_s_median=T * E / r["s_median"], env_steps_per_s_min=T * E / r["s_max"], env_steps_per_s_max=T * E / r["s_min"])

    if "edge_seq" in legs:
        out["edge_seq"] = edge_seq_leg(torch, pol, dev, E, H, 2, T)

    if "update" in legs and a.parent_dir:
        envs.close()
        envs = None
        del ro
        torch.cuda.empty_cache()
        out["update"] = dict(update_ab(a), ppo_epoch=a.ppo_epoch, envs_per_minibatch=E // 2, optimiser_steps=2 * a.ppo_epoch, rounds=a.rounds,
                             update_repeats=a.update_repeats)
    elif "update" in legs:
        agent = PPO(pol, 0.2, a.ppo_epoch, 2, 0.5, 0.0, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
        collect_rollout(envs, pol, ro)
        ro.compute_returns(bootstrap_value(pol, ro), True, 0.99, 0.95, False)
        torch.cuda.reset_peak_memory_stats()
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
    if envs is not None:
        envs.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
