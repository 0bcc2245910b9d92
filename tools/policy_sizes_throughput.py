#!/usr/bin/env python3
"""The policy at network sizes other than the default, timed on the MI355X -> profiles/policy_sizes_throughput.json

    python tools/policy_sizes_throughput.py --out profiles/policy_sizes_throughput.json [--parent-dir DIR] [--rounds 3]

  forward   one rollout forward (cn_policy_act, taps off, noise given) at 4096 envs x 20 humans for five (R, M, A, O) tuples in the three gemm
            modes: device events around a window of `--iters` forwards, three windows after a warm-up window, median with [min..max].  Beside each
            fused figure the sized kernel's own floor: its baked weight image (4 bytes per weight: bf16 hi + lo) times the workgroups that each
            stream it once, over the ~34 TB/s aggregate L2 -> CU rate DESIGN.md section 4 quotes for the fused kernels' weight streams.
  update    PPO.update at T = 30, 4096 envs in two minibatches of 2048, for (192, 64, 48, 320), (256, 128, 128, 512) and for the default: update_s of
            trainer.train's updates 1..3 (update 0 is the warm-up).  Off the default sizes the robot-node part of the update runs on the sized
            sequence (cn_rn_seq_fwd_sized / cn_rn_seq_bwd_sized): inside the autograd-joined producer when the recorded figures were taken, inside
            cn_ppo_minibatch_step_sized since (tools/minibatch_sized_throughput.py records that step).
  update_ab the same update in the tree under --parent-dir and in this tree as alternating child processes (`--rounds` children of three timed
            updates per side and tuple): this tree's sized figures must lie below the parent's with intervals that do not overlap, the default
            tuple's median inside the parent's own range.
  gru       one cn_gru_seq_fwd_sized and one cn_gru_seq_bwd_sized launch per R at N = 2048, T = 30: device events, median of 21 after 5 warm-ups
            (the fragment-image kernel of R = 192 / 256 is inside the bracket), beside the kernel's own floor: the W_hh image (12 R^2 bytes) x 128
            workgroups x 30 steps over the 34 TB/s L2 rate for the streamed form, a wavefront's serial MFMA count x 16 cycles for the resident forms.
  bench_ab  `python bench.py --gpus 1 --steps 20 --warmup 5` of the tree under --parent-dir (a checkout of the parent commit with its library
            built) and of this tree as alternating child processes, `--rounds` each (the side that goes first alternates as well): ms_per_step of every run.
            This tree's median must lie inside the parent's own [min..max].
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUPLES = [(64, 64, 32, 64), (256, 128, 128, 512), (192, 64, 48, 320), (128, 128, 64, 256), (128, 64, 16, 256)]
FLAGS = ("human_node_rnn_size", "human_node_embedding_size", "attention_size", "human_node_output_size")
L2_STREAM_BYTES_PER_S = 34e12


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": list(xs)}


def weight_image_bytes(dims):
    R, M, _, O = dims
    return 4 * ((256 + M) * 256 + 3 * R * R + M * 256 + 3 * R * 2 * M + 2 * O * R + 2 * O * O)


def envs_per_group(dims):
    """rn_sized.hip's rule: 16 envs per workgroup where sixteen activation images and the table fit into 160 KB of LDS, else 8."""
    R, M, _, O = dims
    per_env = max(256, 2 * O) + 4 + max(256 + 2 * M, 2 * O) + 4 + 2 * (3 * R + 4) + 2 * (R + 4)
    table = 256 + 2 * M + 6 * R + 7 * O + 64
    return 16 if 4 * (16 * per_env + table) <= 160 * 1024 else 8


def forward_times(E, H, iters, windows):
    import numpy as np
    import torch
    from crowdnav_prediction_attngraph_amd import _abi as A
    from crowdnav_prediction_attngraph_amd.hip import HipPolicy
    from crowdnav_prediction_attngraph_amd.policy import Policy, make_spaces
    sys.path.insert(0, ROOT)
    from tests import policy_util as PU
    out = []
    ob = {k: torch.from_numpy(v).cuda() for k, v in PU.synth_obs(E, H, 2, seed=1).items()}
    ob_space, act_space = make_spaces(H, 2)
    for dims in TUPLES + [A.DEFAULT_DIMS]:
        torch.manual_seed(425)
        pol = Policy(ob_space.spaces, act_space, base="selfAttn_merge_srnn", base_kwargs=dict(zip(FLAGS, dims)))
        sd = {k: v.cuda() for k, v in pol.state_dict().items()}
        hip = HipPolicy(H, 2, E, dims=dims)
        hip.set_weights(sd)
        hip.set_taps(False)
        R = dims[0]
        g = torch.Generator().manual_seed(1)
        hx = [(torch.rand(E, 1, R, generator=g) * 2 - 1).cuda(), torch.empty(E, 1, R, device="cuda")]
        masks = torch.ones(E, 1, device="cuda")
        eps = torch.randn(E, 2, generator=g).cuda()
        res = dict(value=torch.empty(E, 1, device="cuda"), action=torch.empty(E, 2, device="cuda"), logp=torch.empty(E, 1, device="cuda"))
        rec = {"dims": list(dims), "envs": E, "humans": H, "live_rows": int(np.clip(ob["detected_human_num"].cpu().numpy(), 1, H).sum())}
        for mode in ("fused", "bf16x3", "fp32"):
            hip.set_gemm_mode(mode)
            ms = []
            for w in range(windows + 1):                 # window 0 is the warm-up
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for i in range(iters):
                    hip.act(ob, hx[i & 1], masks, eps=eps, out=dict(res, hxs=hx[(i + 1) & 1]))
                stop.record()
                stop.synchronize()
                if w:
                    ms.append(start.elapsed_time(stop) / iters)
            rec[mode + "_ms_per_forward"] = summary(ms)
        if tuple(dims) != A.DEFAULT_DIMS:
            te = envs_per_group(dims)
            groups = (E + te - 1) // te
            rec["sized_kernel"] = {"envs_per_workgroup": te, "workgroups": groups, "weight_image_bytes": weight_image_bytes(dims),
                                   "floor_us": weight_image_bytes(dims) * groups / L2_STREAM_BYTES_PER_S * 1e6,
                                   "floor_is": "weight image bytes x workgroups / 34 TB/s aggregate L2 -> CU stream (the robot-node kernel alone; the fused "
                                               "figure beside it is the whole forward, human-human kernel included)"}
        hip.close()
        out.append(rec)
    return out


def update_times(E, T, updates):
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd.trainer import train
    out = []
    for dims in UPDATE_DIMS:
        cfg = C.non_randomized(**{"sim.human_num": 20})
        hist, _ = train("CrowdSimVarNum-v0", num_processes=E, num_steps=T, num_updates=updates + 1, seed=425, config=cfg, log=None, network=dict(zip(FLAGS, dims)))
        out.append({"dims": list(dims), "envs": E, "steps": T, "minibatches": 2, "ppo_epoch": 5, "update_s": summary([r["update_s"] for r in hist[1:]]),
                    "rollout_s": summary([r["rollout_s"] for r in hist[1:]]), "warmup_update_s": hist[0]["update_s"]})
    return out


UPDATE_DIMS = ((192, 64, 48, 320), (256, 128, 128, 512), (128, 64, 64, 256))
UPDATE_CHILD = """
import json, sys
sys.path.insert(0, '.')
from crowdnav_prediction_attngraph_amd import config as C
from crowdnav_prediction_attngraph_amd.trainer import train
dims = json.loads(sys.argv[1])
flags = ("human_node_rnn_size", "human_node_embedding_size", "attention_size", "human_node_output_size")
cfg = C.non_randomized(**{"sim.human_num": 20})
hist, _ = train("CrowdSimVarNum-v0", num_processes=int(sys.argv[2]), num_steps=30, num_updates=4, seed=425, config=cfg, log=None, network=dict(zip(flags, dims)))
print("UPDATE_S " + json.dumps([r["update_s"] for r in hist[1:]]))
"""


def update_child(tree, dims, E):
    p = subprocess.run([sys.executable, "-c", UPDATE_CHILD, json.dumps(list(dims)), str(E)], cwd=tree, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError("update child in %s failed (%d): %s" % (tree, p.returncode, p.stderr[-2000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("UPDATE_S ")][-1][9:])


def update_ab(parent_dir, rounds, E):
    out = []
    for dims in UPDATE_DIMS:
        runs = {"parent": [], "this": []}
        for r in range(rounds):
            pair = (("parent", parent_dir), ("this", ROOT))
            for name, tree in (pair if r % 2 == 0 else pair[::-1]):
                runs[name] += update_child(tree, dims, E)
                print(dims, name, runs[name][-3:], flush=True)
        p, t = summary(runs["parent"]), summary(runs["this"])
        out.append({"dims": list(dims), "envs": E, "steps": 30, "parent_update_s": p, "this_update_s": t, "this_below_parent_without_overlap": bool(t["max"] < p["min"]),
                    "this_median_inside_parent_range": bool(p["min"] <= t["median"] <= p["max"])})
    return out


def gru_times(N, T):
    import torch
    from crowdnav_prediction_attngraph_amd import _abi as A
    out = []
    g = torch.Generator().manual_seed(3)
    for R in (64, 128, 192, 256):
        u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).cuda()   # noqa: E731
        gi, h0, m, whh, bhh, dhs = u(T, N, 3 * R), u(N, R), torch.ones(T, N, device="cuda"), u(3 * R, R) * (1.6 / R ** 0.5), u(3 * R) * 0.1, u(T, N, R)
        e = lambda *s: torch.empty(*s, device="cuda")   # noqa: E731
        hs, hms, gates, dgi, dgh, dh0, ws = e(T, N, R), e(T, N, R), e(T, N, 4 * R), e(T, N, 3 * R), e(T, N, 3 * R), e(N, R), e(3 * R * R)
        fwd = lambda: A.call("cn_gru_seq_fwd_sized", T, N, R, A.ptr(gi), A.ptr(h0), A.ptr(m), A.ptr(whh), A.ptr(bhh), A.ptr(hs), A.ptr(hms), A.ptr(gates),  # noqa: E731
                             A.ptr(ws), A.stream_ptr())
        bwd = lambda: A.call("cn_gru_seq_bwd_sized", T, N, R, A.ptr(gates), A.ptr(hms), A.ptr(m), A.ptr(whh), A.ptr(dhs), A.ptr(dgi), A.ptr(dgh), A.ptr(dh0),  # noqa: E731
                             A.ptr(ws), A.stream_ptr())
        rec = {"R": R, "N": N, "T": T, "scheme": "resident128" if R == 128 else ("resident" if R == 64 else "streamed")}
        for name, fn in (("fwd", fwd), ("bwd", bwd)):
            us = []
            for i in range(26):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                fn()
                stop.record()
                stop.synchronize()
                if i >= 5:
                    us.append(start.elapsed_time(stop) * 1e3)
            rec[name + "_us"] = summary(us)
        groups = (N + 15) // 16
        if R > 128:
            rec["floor_us"] = 12 * R * R * groups * T / L2_STREAM_BYTES_PER_S * 1e6
            rec["floor_is"] = "W_hh image (12 R^2 bytes) x %d workgroups x %d steps / 34 TB/s aggregate L2 -> CU stream, per direction" % (groups, T)
        else:
            mfma = 3 * (R // 64) * 3 * (R // 32) * T                    # per wavefront and direction: 3 terms x blocks x gates (or 3 R / 32 k-steps) x k-steps x T
            rec["floor_us"] = mfma * 16 / 2.4e9 * 1e6                     # a wavefront is alone on its SIMD and its steps are serial: 16 cycles per MFMA at 2.4 GHz
            rec["floor_is"] = "%d v_mfma_f32_16x16x32_bf16 per wavefront (one per SIMD, the steps are serial) x 16 cycles at 2.4 GHz, per direction" % mfma
        out.append(rec)
    return out


def bench_child(tree):
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError("bench.py in %s failed (%d): %s" % (tree, p.returncode, p.stderr[-2000:]))
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    return {"ms_per_step": line["ms_per_step"], "value": line["value"], "unit": line["unit"]}


def bench_ab(parent_dir, rounds):
    runs = {"parent": [], "this": []}
    for r in range(rounds):
        pair = (("parent", parent_dir), ("this", ROOT))
        for name, tree in (pair if r % 2 == 0 else pair[::-1]):      # the side that goes first alternates too
            runs[name].append(bench_child(tree))
            print(name, runs[name][-1], flush=True)
    res = {name: {"ms_per_step": summary([r["ms_per_step"] for r in rs]), "runs": rs} for name, rs in runs.items()}
    p, t = res["parent"]["ms_per_step"], res["this"]["ms_per_step"]
    res["this_median_inside_parent_range"] = bool(p["min"] <= t["median"] <= p["max"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parent-dir", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--update-rounds", type=int, default=2, help="update_ab: child processes per side and tuple, three timed updates each")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--humans", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--skip", default="", help="comma-separated: forward, update, bench_ab, update_ab, gru")
    a = ap.parse_args()
    skip = set(filter(None, a.skip.split(",")))
    sys.path.insert(0, ROOT)
    res = {"cmd": " ".join(sys.argv)}

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    if "bench_ab" not in skip and a.parent_dir:      # first: child processes only, before this process opens the GPU
        res["bench_ab"] = bench_ab(os.path.abspath(a.parent_dir), a.rounds)
        flush()
    if "update_ab" not in skip and a.parent_dir:
        res["update_ab"] = update_ab(os.path.abspath(a.parent_dir), a.update_rounds, a.envs)
        flush()
    if "gru" not in skip:
        res["gru"] = gru_times(2048, 30)
        flush()
    if "forward" not in skip:
        res["forward"] = forward_times(a.envs, a.humans, a.iters, 3)
        flush()
    if "update" not in skip:
        res["update"] = update_times(a.envs, 30, 3)
        flush()
    print(json.dumps(res)[:3000])


if __name__ == "__main__":
    main()
