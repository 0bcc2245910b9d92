#!/usr/bin/env python3
"""Where the GPU time of a DS-RNN (Policy(base='srnn')) PPO.update goes, from one kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/srnn_update_breakdown.py --run
    python tools/srnn_update_breakdown.py --summarize DIR/.../*_kernel_trace.csv --out profiles/srnn_update_breakdown.txt

--run is the traced workload: one rollout at the bench shape of tools/srnn_throughput.py (4096 envs x 20 humans, T = 30, 2 minibatches), one
warm-up PPO.update and one update between two triple sentinels.  The package is imported from PYTHONPATH / the working directory, so the same
file traces the parent commit's tree.  The framework kernels of the torch-op path carry no name that says which part of the network they
belong to, so the run drops a sentinel launch (torch.cuda._sleep: `spin_kernel`) at the seams of every minibatch, in this order:
    S0 evaluate_actions starts | S1 attention forward starts | S2 attention forward ends | S3 the gradient of `weighted` is ready |
    S4, S5 the gradients of h_t and h_s (attention's inputs) are ready | S6 the optimiser step starts
--summarize sums kernel durations between consecutive sentinels and prints the share of four groups:
    (a) edge GRUs: S0..S1 (forward: _edge_gi and the two _gru_cell loops, or the sequence kernels) and S5..S6 (their backward)
    (b) attention: S1..S2 and S3..S5
    (c) node GRU, trunks, heads, losses: S2..S3 (forward and backward)
    (d) gather and optimiser: S6..the next S0, and what precedes the first S0 (advantages, the first minibatch's gather)
With SRNNBase.train_node_kernels the attention is hip_train.SrnnAttention on h_all itself; the same sentinels go around that call.
A kernel belongs to the interval its start falls into; the sentinels themselves are left out.
"""
import argparse
import csv
import glob
import os
import sys

SENTINEL = "spin_kernel"
PER_MINIBATCH = 7


def run(a):
    import torch

    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd.policy import Policy
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
    if a.ops and hasattr(pol.base, "train_edge_kernels"):
        pol.base.train_edge_kernels = False
        pol.base.train_node_kernels = False
    ro = RolloutStorage(T, E, envs.observation_space.spaces, envs.action_space, 128, 256)
    ro.to(dev)
    ro.materialize_edge_rnn()
    obs = envs.reset_device()
    for k in ro.obs:
        ro.obs[k][0].copy_(obs[k].view_as(ro.obs[k][0]) if k != "visible_masks" else obs[k].to(torch.bool))
    collect_rollout(envs, pol, ro)
    ro.compute_returns(bootstrap_value(pol, ro), True, 0.99, 0.95, False)
    agent = PPO(pol, 0.2, a.ppo_epoch, 2, 0.5, 0.0, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
    agent.update(ro)                            # warm-up, unmarked

    mark = lambda: torch.cuda._sleep(200)       # noqa: E731
    ev, attn, step = pol.evaluate_actions, pol.base.attention, agent._optimizer_step

    def evaluate_actions(*args, **kw):
        mark()                                  # S0
        return ev(*args, **kw)

    def attention(h_t, h_s):
        mark()                                  # S1
        if h_t.requires_grad:
            h_t.register_hook(lambda g: mark())         # S4 / S5
            h_s.register_hook(lambda g: mark())
        weighted, w = attn(h_t, h_s)
        if weighted.requires_grad:
            weighted.register_hook(lambda g: mark())    # S3
        mark()                                  # S2
        return weighted, w

    def optimizer_step(*args, **kw):
        mark()                                  # S6
        return step(*args, **kw)

    pol.evaluate_actions, pol.base.attention, agent._optimizer_step = evaluate_actions, attention, optimizer_step
    from crowdnav_prediction_attngraph_amd import hip_train
    fused = getattr(hip_train, "SrnnAttention", None)
    if fused is not None and getattr(pol.base, "train_node_kernels", False) and not a.ops:
        # the kernel route never calls SRNNBase.attention: the same seams around hip_train.SrnnAttention, whose input is h_all itself (its
        # gradient is the two of h_t and h_s at once: S4 and S5 are neighbours)
        def both(g):
            mark()
            mark()

        class MarkedAttention:
            @staticmethod
            def apply(h_all, *rest):
                mark()                                  # S1
                if h_all.requires_grad:
                    h_all.register_hook(both)           # S4, S5
                out = fused.apply(h_all, *rest)
                if out[0].requires_grad:
                    out[0].register_hook(lambda g: mark())      # S3
                mark()                                  # S2
                return out
        hip_train.SrnnAttention = MarkedAttention
    torch.cuda.synchronize()
    mark(); mark(); mark()                      # the marked update lies between two triple sentinels
    agent.update(ro)
    mark(); mark(); mark()
    torch.cuda.synchronize()
    envs.close()
    print("traced one PPO.update: %d envs x %d humans, T = %d, 2 minibatches, %d epoch(s), peak memory %.2f GB"
          % (E, H, T, a.ppo_epoch, torch.cuda.max_memory_allocated() / 2 ** 30))


def summarize(a):
    paths = sorted(p for pat in a.summarize for p in glob.glob(pat))
    rows = []
    for p in paths:
        with open(p, newline="") as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    sent = [i for i, r in enumerate(rows) if SENTINEL in r[2]]
    # the triple sentinels: three sentinels with no kernel between them (S4 and S5 may be neighbours, never three)
    triples = [k for k in range(len(sent) - 2) if sent[k + 2] == sent[k] + 2]
    assert len(triples) == 2, "expected two triple sentinels around the marked update, found %d" % len(triples)
    inner = sent[triples[0] + 3:triples[1]]
    assert inner and len(inner) % PER_MINIBATCH == 0, "%d sentinels inside the update: not a multiple of %d" % (len(inner), PER_MINIBATCH)
    group_of = ["a", "b", "c", "b", "b", "a", "d"]     # the interval that FOLLOWS sentinel S0 .. S6
    total = {"a": 0, "b": 0, "c": 0, "d": 0}
    count = dict(total)
    names = {g: {} for g in total}
    bounds = [sent[triples[0] + 2]] + inner + [sent[triples[1]]]
    for j in range(len(bounds) - 1):
        g = "d" if j == 0 else group_of[(j - 1) % PER_MINIBATCH]
        for s, e, n in rows[bounds[j] + 1:bounds[j + 1]]:
            total[g] += e - s
            count[g] += 1
            names[g][n] = names[g].get(n, 0) + e - s
    wall = rows[bounds[-1]][0] - rows[bounds[0]][1]
    busy = sum(total.values())
    label = {"a": "(a) edge GRUs: _edge_gi + the two _gru_cell loops, forward and backward", "b": "(b) attention, forward and backward",
             "c": "(c) node GRU, trunks, heads, losses, forward and backward", "d": "(d) gather and optimiser"}
    out = ["%s" % a.title, "minibatches traced: %d; kernels: %d; GPU busy %.1f ms of %.1f ms between the sentinels"
           % (len(inner) // PER_MINIBATCH, sum(count.values()), busy / 1e6, wall / 1e6), ""]
    for g in "abcd":
        out.append("%-78s %9.1f ms  %5.1f %%  %7d kernels" % (label[g], total[g] / 1e6, 100.0 * total[g] / busy, count[g]))
    for g in "abcd":
        out += ["", "top kernels of %s" % label[g][:3]]
        for n, t in sorted(names[g].items(), key=lambda kv: -kv[1])[:a.top]:
            out.append("  %9.1f ms  %s" % (t / 1e6, n[:150]))
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--ops", action="store_true", help="--run: force the torch-op loop (train_edge_kernels = False) where the tree has the switch")
    ap.add_argument("--summarize", nargs="+", default=None, help="kernel-trace CSV files (globs)")
    ap.add_argument("--title", default="DS-RNN PPO.update, 4096 envs x 20 humans, T = 30, 2 minibatches: GPU time by part of the network")
    ap.add_argument("--out", default=None)
    ap.add_argument("--top", type=int, default=6)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--humans", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--ppo-epoch", type=int, default=1)
    a = ap.parse_args()
    if a.run:
        if not os.environ.get("PYTHONPATH"):
            sys.path.insert(0, os.getcwd())
        return run(a)
    if a.summarize:
        return summarize(a)
    ap.error("--run or --summarize")


if __name__ == "__main__":
    main()
