#!/usr/bin/env python3
"""Bit pin of the GRU sequence pair (cn_gru_seq_fwd_sized / cn_gru_seq_bwd_sized) -> tests/golden/gru_seq_bits.json

    python tests/golden/make_golden_gru_bits.py --commit <hash of the build that ran>      (needs the MI355X)

Inputs come from np.random.RandomState seeds (uniform doubles cast to float32, as tests/test_gpu_rn_seq_sizes.py's fp64 comparison draws them), so
the file holds no arrays: per case the sha256 of the raw float32 bytes of hs, hms, gates, dgi, dgh, dh0 (the arrays themselves would be over
1 MB), and the commit whose build produced them.  Consumer: tests/test_gpu_gru_seq_bits.py, which imports CASES, inputs, run and digests from here.

Cases (R, T, N):
  (3, 17) at every R   two workgroups, the second with one live row: the min(row, N-1) clamps and the row < N guards
  (1, 1) at 128, 192   t + 1 < T is never true, the min(t+1, T-1) clamps apply, the streamed form's wrap requests a step that does not exist
  (2, 16) at 128       an exactly full workgroup
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "gru_seq_bits.json")
CASES = [(R, 3, 17) for R in (64, 128, 192, 256)] + [(128, 1, 1), (192, 1, 1), (128, 2, 16)]
ARRAYS = ("hs", "hms", "gates", "dgi", "dgh", "dh0")
GUARD = 96


def case_id(case):
    return "R%d_T%d_N%d" % case


def inputs(R, T, N):
    """float32 inputs of one case.  Done masks on the diagonal (m[0,0] = m[1,1] = m[2,2] = 0) wherever the sequence has more than one step; a
    single step keeps its mask at 1, since the one zero it could hold would wipe h0 and with it the z * h term and d(h0)."""
    rs = np.random.RandomState([R, T, N])
    d = dict(gi=rs.uniform(-1, 1, (T, N, 3 * R)), h0=rs.uniform(-1, 1, (N, R)), whh=rs.uniform(-1, 1, (3 * R, R)) * (1.6 / np.sqrt(R)),
             bhh=rs.uniform(-0.1, 0.1, 3 * R), d_hs=rs.uniform(-1, 1, (T, N, R)))
    m = np.ones((T, N))
    if T > 1:
        for i in range(min(T, N, 3)):
            m[i, i] = 0.0
    d["m"] = m
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in d.items()}


def run(R, T, N, inp, null_workspace=False):
    """One forward and one backward into NaN-filled buffers with NaN guard tails; returns the six arrays as device tensors."""
    import torch
    from crowdnav_prediction_attngraph_amd import _abi as A
    dev = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
    shapes = dict(hs=(T, N, R), hms=(T, N, R), gates=(T, N, 4 * R), dgi=(T, N, 3 * R), dgh=(T, N, 3 * R), dh0=(N, R), ws_f=(3 * R * R,), ws_b=(3 * R * R,))
    bufs = {k: torch.full((int(np.prod(s)) + GUARD,), float("nan"), device="cuda") for k, s in shapes.items()}
    v = {k: b[:int(np.prod(shapes[k]))].view(*shapes[k]) for k, b in bufs.items()}
    ws_f, ws_b = (None, None) if null_workspace else (A.ptr(v["ws_f"]), A.ptr(v["ws_b"]))
    A.call("cn_gru_seq_fwd_sized", T, N, R, A.ptr(dev["gi"]), A.ptr(dev["h0"]), A.ptr(dev["m"]), A.ptr(dev["whh"]), A.ptr(dev["bhh"]), A.ptr(v["hs"]),
           A.ptr(v["hms"]), A.ptr(v["gates"]), ws_f, A.stream_ptr())
    A.call("cn_gru_seq_bwd_sized", T, N, R, A.ptr(v["gates"]), A.ptr(v["hms"]), A.ptr(dev["m"]), A.ptr(dev["whh"]), A.ptr(dev["d_hs"]), A.ptr(v["dgi"]),
           A.ptr(v["dgh"]), A.ptr(v["dh0"]), ws_b, A.stream_ptr())
    torch.cuda.synchronize()
    for k, whole in bufs.items():
        assert torch.isnan(whole[v[k].numel():]).all(), "guard tail behind %s was written" % k
        assert k.startswith("ws_") or not torch.isnan(v[k]).any(), "%s has entries the call did not write" % k
    return {k: v[k].clone() for k in ARRAYS}


def digests(out):
    return {k: hashlib.sha256(out[k].contiguous().cpu().numpy().astype(np.float32, copy=False).tobytes()).hexdigest() for k in ARRAYS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose build is loaded")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--only", default="", help="comma-separated R: regenerate these, keep the other cases of the existing file")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    only = {int(x) for x in a.only.split(",") if x}
    res = {"commit": a.commit, "arrays": list(ARRAYS), "cases": {}}
    if only:
        with open(a.out) as f:
            res = json.load(f)
        res.setdefault("regenerated", {})
    for case in CASES:
        if only and case[0] not in only:
            continue
        res["cases"][case_id(case)] = digests(run(*case, inputs(*case)))
        if only:
            res["regenerated"][case_id(case)] = a.commit
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases" % (a.out, len(res["cases"])))


if __name__ == "__main__":
    main()
