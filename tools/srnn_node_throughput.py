#!/usr/bin/env python3
"""The DS-RNN baseline's PPO.update with the node half on HIP kernels (SRNNBase.train_node_kernels) against the parent commit, and the two
attention kernels alone.

    python tools/srnn_node_throughput.py --parent-dir DIR --out profiles/srnn_node_throughput.json

  update:  the method of tools/srnn_throughput.py (its update leg, reused from there): the parent's tree (--parent-dir, a checkout of the parent
           commit with its library built) and this one run as alternating child processes in one box, --rounds x --update-repeats PPO.updates
           each after one warm-up, at --envs x --humans, T = --steps, envs / 2 per minibatch; median [min..max] and the peak memory of both
           sides.  The bar: this tree's interval lies below the parent's and the two do not overlap.
  kernels: one event-bracketed cn_srnn_attn_fwd and cn_srnn_attn_bwd at B = T * envs / 2 samples of H humans, median of 21 after 5 warm-ups,
           beside their stream floors: h_all read once (forward), read once and its gradient written once (backward), at the 8.0 TB/s spec rate.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def kernel_leg(B, H, warm=5, reps=21):
    import torch

    from crowdnav_prediction_attngraph_amd import _abi as A
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(3)
    h_all = torch.rand(B, H + 1, 256, device=dev, generator=g) * 2 - 1
    wt, ws = (torch.rand(64, 256, device=dev, generator=g) - 0.5) / 8, (torch.rand(64, 256, device=dev, generator=g) - 0.5) / 8
    bt = torch.rand(64, device=dev, generator=g) - 0.5
    d_w, d_t = torch.rand(B, 256, device=dev, generator=g) - 0.5, torch.rand(B, 256, device=dev, generator=g) - 0.5
    weighted, attn, te, u = (torch.empty(B, n, device=dev) for n in (256, H, 64, 256))
    d_h_all, d_u, d_te = torch.empty_like(h_all), torch.empty(B, 256, device=dev), torch.empty(B, 64, device=dev)
    tf, tb = [], []
    for i in range(warm + reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        A.call("cn_srnn_attn_fwd", B, H, A.ptr(h_all), A.ptr(wt), A.ptr(bt), A.ptr(ws), A.ptr(weighted), A.ptr(attn), A.ptr(te), A.ptr(u), A.stream_ptr())
        ev[1].record()
        A.call("cn_srnn_attn_bwd", B, H, A.ptr(h_all), A.ptr(wt), A.ptr(ws), A.ptr(attn), A.ptr(u), A.ptr(d_w), A.ptr(d_t), A.ptr(d_h_all), A.ptr(d_u),
               A.ptr(d_te), A.stream_ptr())
        ev[2].record()
        torch.cuda.synchronize()
        if i >= warm:
            tf.append(ev[0].elapsed_time(ev[1]))
            tb.append(ev[1].elapsed_time(ev[2]))
    h_bytes = B * (H + 1) * 256 * 4
    small = B * (256 + H + 64 + 256) * 4                               # weighted, attn, te, u written by the forward; read or mirrored by the backward
    return dict(B=B, H=H, h_all_gb=h_bytes / 1e9, warmups=warm, samples=reps,
                fwd_ms_median=statistics.median(tf), fwd_ms_min=min(tf), fwd_ms_max=max(tf),
                bwd_ms_median=statistics.median(tb), bwd_ms_min=min(tb), bwd_ms_max=max(tb),
                floors_ms=dict(fwd_h_all_once_at_8_tb_s=h_bytes / 8e12 * 1e3, bwd_h_all_read_and_written_at_8_tb_s=2 * h_bytes / 8e12 * 1e3,
                               fwd_all_operands_at_8_tb_s=(h_bytes + small) / 8e12 * 1e3),
                achieved_tb_s=dict(fwd=h_bytes / (statistics.median(tf) * 1e-3) / 1e12, bwd=2 * h_bytes / (statistics.median(tb) * 1e-3) / 1e12))


def main():
    import srnn_throughput as S
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-dir", default=None)
    ap.add_argument("--legs", default="kernels,update")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--update-repeats", type=int, default=2)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--humans", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--ppo-epoch", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    legs = set(a.legs.split(","))
    import torch
    assert torch.cuda.is_available(), "srnn_node_throughput.py measures the GPU paths"
    out = {"device": torch.cuda.get_device_name(0), "envs": a.envs, "humans": a.humans, "steps": a.steps, "envs_per_minibatch": a.envs // 2}
    if "kernels" in legs:
        out["attention_kernels"] = kernel_leg(a.steps * (a.envs // 2), a.humans)
        torch.cuda.empty_cache()
    if "update" in legs:
        if not a.parent_dir:
            raise SystemExit("the update leg needs --parent-dir: a checkout of the parent commit with its library built")
        out["update"] = dict(S.update_ab(a), ppo_epoch=a.ppo_epoch, optimiser_steps=2 * a.ppo_epoch, rounds=a.rounds, update_repeats=a.update_repeats)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
