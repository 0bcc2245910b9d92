#!/usr/bin/env python
"""How many wave-steps orca_lp3_kernel needs per pair of programs: the nested lock-step loops against one flat loop, and pairs
formed at random against pairs formed inside bins of a predictor.  CPU only.

orca_lp3_kernel (csrc/orca.h) solves two linearProgram3 programs per wavefront.  A program is a walk over its violated lines
("open line i: project the lines j < i on it"), each followed by a walk over the violated projected lines ("clip": one
linearProgram1).  The study replays recorded hand-overs (header + lines, as orca_lane_kernel writes them) with a float32
restatement of lp3_wave that counts, per opened line, the clips it took, and checks the result of every program against the
oracle's.  From the counts:

  (a) nested, random pairs   the loop nest of lp3_pair: per outer turn one open and max(clips of a, clips of b) clips
  (b) flat, random pairs     one loop, a turn gives each half its next unit: a program takes sum max(c_k, 1) turns, a pair the maximum
  (c) flat, binned pairs     as (b), pairs formed between neighbours of a list ordered by the bin of a predictor (longest bin
                             first, a bin's odd program pairs with the first of the next bin)

Predictors (all known to the lane kernel at hand-over): nn - line_fail; the number of lines >= line_fail the result at hand-over
violates at distance 0; the two combined.  Bins: at most 8, edges at the quantiles of the predictor over the recorded list.

A wave-step is one execution of a block by the wavefront.  Open blocks, clip blocks and the turns that do neither (the loop
heads that find a walk finished) are counted apart and summed with the instructions of those blocks in the gfx950 assembly of
each form (WEIGHTS: counted per basic block of orca_lp3_kernel, s_nop included).

  python tools/lp3_pairing_study.py --record tests/golden/lp3_handovers_h20.npz     # oracle run -> fixture (a few hundred programs)
  python tools/lp3_pairing_study.py tests/golden/lp3_handovers_h20.npz > profiles/lp3_pairing_study.txt
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F = np.float32
EPS = F(1e-5)
# form -> instructions of (an open, a clip, a turn's fixed part).  nested: the fixed part is the head of the inner loop, paid by the turns that
# do not clip; flat: the head of the single loop, paid by every turn on top of the blocks it enters.
WEIGHTS = {
    "nested": (130, 190, 25),          # the loop nest with a float DPP tree and the chord of the disc worked out in every clip
    "nested, chords": (170, 130, 25),  # the chords of all projected lines once per open, the trees on integer keys
    "flat": (95, 195, 56),
}


def record(path, envs, steps, keep, seed):
    """Step `envs` oracle envs of the flagship's class (20 humans, fixed attributes) and keep every `keep`-th hand-over."""
    from oracle import oracle as O
    from tests.lp3_util import handovers, oracle_env_head
    from tests.test_gpu_env import _actions
    head = oracle_env_head()
    cfg = O.default_config(human_num=20, nenv=envs)
    oenvs = [O.OracleEnv(cfg, seed + i) for i in range(envs)]
    keys = ("robot_node", "temporal_edges", "spatial_edges", "detected_human_num", "visible_masks")
    obs = [oe.reset() for oe in oenvs]
    host = {k: np.stack([ob[k] for ob in obs]) for k in keys}
    progs, n_agents = [], 0
    for t in range(steps):
        for oe in oenvs:
            n_agents += oe.human_count
            progs += handovers(oe, head, want_lines=True)
        act = _actions(host, t, envs)
        obs = [oe.step(act[i], autoreset=True)[0] for i, oe in enumerate(oenvs)]
        host = {k: np.stack([ob[k] for ob in obs]) for k in keys}
    frac = len(progs) / n_agents
    progs = progs[::keep]
    lines = np.zeros((len(progs), 32, 4), F)
    for k, p in enumerate(progs):
        lines[k, :p["nn"]] = p["lines"]
    np.savez_compressed(path, lines=lines, nn=np.array([p["nn"] for p in progs], np.int32), line_fail=np.array([p["line_fail"] for p in progs], np.int32),
                        radius=np.array([p["radius"] for p in progs], F), pref=np.array([p["pref"] for p in progs], F),
                        out=np.array([p["out"] for p in progs], F), infeasible_fraction=np.float64(frac))
    print("%d programs kept of %d agent-steps (%.1f %% infeasible) -> %s" % (len(progs), n_agents, 100 * frac, path))


def det(ax, ay, bx, by):
    return F(F(ax * by) - F(ay * bx))


def lp1(P, D, valid, i, radius, optx, opty, dir_opt, r):
    """RVO2 linearProgram1 on line i against the valid lines before it (bounds by min / max: the same decision as the sequential loop)."""
    ipx, ipy, idx, idy = P[i, 0], P[i, 1], D[i, 0], D[i, 1]
    dot = F(F(ipx * idx) + F(ipy * idy))
    disc = F(F(F(dot * dot) + F(radius * radius)) - F(F(ipx * ipx) + F(ipy * ipy)))
    if disc < 0:
        return False
    sq = np.sqrt(disc)
    tl, tr = F(-dot - sq), F(-dot + sq)
    for j in range(i):
        if not valid[j]:
            continue
        den = det(idx, idy, D[j, 0], D[j, 1])
        num = det(D[j, 0], D[j, 1], F(ipx - P[j, 0]), F(ipy - P[j, 1]))
        if abs(den) <= EPS:
            if num < 0:
                return False
            continue
        t = F(num / den)
        if den >= 0:
            tr = min(tr, t)
        else:
            tl = max(tl, t)
    if tl > tr:
        return False
    if dir_opt:
        t = tr if F(F(optx * idx) + F(opty * idy)) > 0 else tl
    else:
        t = F(F(idx * F(optx - ipx)) + F(idy * F(opty - ipy)))
        t = tl if t < tl else (tr if t > tr else t)
    r[0] = F(ipx + F(t * idx)); r[1] = F(ipy + F(t * idy))
    return True


def viol(P, D, k, r, dist):
    return det(D[k, 0], D[k, 1], F(P[k, 0] - r[0]), F(P[k, 1] - r[1])) > dist


def lp2_head(P, D, nn, radius, pref):
    """linearProgram2 with the preferred velocity up to the line it fails on: (line_fail, result there)."""
    ox, oy = pref
    if F(F(ox * ox) + F(oy * oy)) > F(radius * radius):
        inv = F(F(1) / np.sqrt(F(F(ox * ox) + F(oy * oy))))
        r = [F(radius * F(ox * inv)), F(radius * F(oy * inv))]
    else:
        r = [ox, oy]
    valid = np.ones(nn, bool)
    for i in range(nn):
        if viol(P, D, i, r, F(0)):
            if not lp1(P, D, valid, i, radius, ox, oy, False, r):
                return i, r
    return nn, r


def lp3_counts(P, D, nn, begin, radius, r):
    """lp3_wave with counters: the clips of every opened line.  r is updated in place."""
    dist = F(0)
    clips = []
    for i in range(begin, nn):
        if not viol(P, D, i, r, dist):
            continue
        Q, QD, valid = np.zeros((i, 2), F), np.zeros((i, 2), F), np.zeros(i, bool)
        for j in range(i):
            d = det(D[i, 0], D[i, 1], D[j, 0], D[j, 1])
            if abs(d) <= EPS:
                if F(F(D[i, 0] * D[j, 0]) + F(D[i, 1] * D[j, 1])) > 0:
                    continue
                Q[j] = (F(F(0.5) * F(P[i, 0] + P[j, 0])), F(F(0.5) * F(P[i, 1] + P[j, 1])))
            else:
                s = F(det(D[j, 0], D[j, 1], F(P[i, 0] - P[j, 0]), F(P[i, 1] - P[j, 1])) / d)
                Q[j] = (F(P[i, 0] + F(s * D[i, 0])), F(P[i, 1] + F(s * D[i, 1])))
            ddx, ddy = F(D[j, 0] - D[i, 0]), F(D[j, 1] - D[i, 1])
            inv = F(F(1) / np.sqrt(F(F(ddx * ddx) + F(ddy * ddy))))
            QD[j] = (F(ddx * inv), F(ddy * inv))
            valid[j] = True
        ox, oy = F(-D[i, 1]), D[i, 0]
        t = list(r)
        r[0], r[1] = F(radius * ox), F(radius * oy)
        c = 0
        for j in range(i):
            if valid[j] and viol(Q, QD, j, r, F(0)):
                c += 1
                if not lp1(Q, QD, valid, j, radius, ox, oy, True, r):
                    r[0], r[1] = t
                    break
        clips.append(c)
        dist = det(D[i, 0], D[i, 1], F(P[i, 0] - r[0]), F(P[i, 1] - r[1]))
    return clips


def half_units(clips):
    """The flat loop's turns of one program: (opens this turn, clips this turn) flags."""
    op, cl = [], []
    for c in clips:
        op += [1] + [0] * (max(c, 1) - 1)
        cl += [1] * c if c else [0]
    return np.array(op, bool), np.array(cl, bool)


def cost_nested(a, b):
    """parent lp3_pair: outer turn k opens line k of both halves and clips until both inner walks are through (+ the turn that finds that out)"""
    n = max(len(a), len(b))
    aa, bb = a + [0] * (n - len(a)), b + [0] * (n - len(b))
    opens = n
    clips = sum(max(x, y) for x, y in zip(aa, bb))
    turns = sum(max(x, y) + 1 for x, y in zip(aa, bb)) + 1
    return opens, clips, turns


def cost_flat(a, b):
    (ao, ac), (bo, bc) = half_units(a), half_units(b)
    n = max(len(ao), len(bo))
    pad = lambda v: np.concatenate([v, np.zeros(n - len(v), bool)])
    return int((pad(ao) | pad(bo)).sum()), int((pad(ac) | pad(bc)).sum()), n + 1


def weigh(c, form):
    w = WEIGHTS[form]
    return w[0] * c[0] + w[1] * c[1] + w[2] * (c[2] if form == "flat" else c[2] - c[1])


def pair_up(order):
    return [(order[k], order[k + 1] if k + 1 < len(order) else None) for k in range(0, len(order), 2)]


def total(pairs, clips, cost):
    tot = np.zeros(3, np.int64)
    for a, b in pairs:
        tot += cost(clips[a], clips[b] if b is not None else [])
    return tot


def binned_order(pred, arrival, bins):
    """bins by the quantiles of the predictor, longest first; inside a bin the order slots were handed out in"""
    edges = np.unique(np.quantile(pred, np.linspace(0, 1, bins + 1)[1:-1]))
    b = np.searchsorted(edges, pred, side="right")
    pos = {k: n for n, k in enumerate(arrival)}
    return sorted(arrival, key=lambda k: (-b[k], pos[k])), len(edges) + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("fixture", nargs="?")
    ap.add_argument("--record", metavar="NPZ")
    ap.add_argument("--envs", type=int, default=24)
    ap.add_argument("--steps", type=int, default=160)
    ap.add_argument("--keep", type=int, default=37, help="keep every n-th hand-over of the run")
    ap.add_argument("--seed", type=int, default=425)
    ap.add_argument("--shuffles", type=int, default=20)
    a = ap.parse_args()
    if a.record:
        return record(a.record, a.envs, a.steps, a.keep, a.seed)
    z = np.load(a.fixture)
    N = len(z["nn"])
    clips, p_rest, p_viol = [], [], []
    for k in range(N):
        nn, lf, radius = int(z["nn"][k]), int(z["line_fail"][k]), z["radius"][k]
        P, D = z["lines"][k, :nn, 0:2].copy(), z["lines"][k, :nn, 2:4].copy()
        lf2, r = lp2_head(P, D, nn, radius, z["pref"][k])
        assert lf2 == lf, (k, lf2, lf)   # the restatement takes the oracle's path
        p_rest.append(nn - lf)
        p_viol.append(sum(bool(viol(P, D, i, r, F(0))) for i in range(lf, nn)))
        clips.append(lp3_counts(P, D, nn, lf, radius, r))
        assert r[0] == z["out"][k, 0] and r[1] == z["out"][k, 1], (k, r, z["out"][k])   # ... and ends on the oracle's bits
    p_rest, p_viol = np.array(p_rest), np.array(p_viol)
    turns = np.array([sum(max(c, 1) for c in cl) for cl in clips])
    inner = np.array([sum(cl) for cl in clips])
    print("programs: %d (20 humans, fixed attributes; %.1f %% of the run's agent-steps were infeasible)" % (N, 100 * float(z["infeasible_fraction"])))
    pc = lambda v: "%s / mean %.1f" % (" / ".join("%d" % np.percentile(v, q) for q in (10, 50, 90, 99, 100)), v.mean())
    print("opened lines per program      (10 / 50 / 90 / 99 / 100th percentile): " + pc(np.array([len(c) for c in clips])))
    print("clips per program                                                    : " + pc(inner))
    print("turns of the flat loop per program, sum max(c_k, 1)                  : " + pc(turns))
    for form, w in WEIGHTS.items():
        print("weights, %-15s: open %d, clip %d, fixed part of a turn %d instructions" % (form, w[0], w[1], w[2]))
    print()
    rng = np.random.RandomState(a.seed)
    rows = {}

    def add(name, cost, order_fn, form="flat"):
        acc = []
        for _ in range(a.shuffles):
            arrival = rng.permutation(N)
            acc.append(total(pair_up(order_fn(arrival)), clips, cost))
        rows[name] = (np.mean(acc, axis=0), form)

    add("(a) nested, random pairs", cost_nested, lambda arr: list(arr), "nested")
    add("(a') nested with chords and key trees, random pairs", cost_nested, lambda arr: list(arr), "nested, chords")
    add("(b) flat, random pairs", cost_flat, lambda arr: list(arr))
    preds = {"nn - line_fail": p_rest, "violated at hand-over": p_viol, "combined: violated * 32 + (nn - line_fail)": p_viol * 32 + p_rest,
             "[bound] the true turn count": turns}
    for pname, pred in preds.items():
        for bins in (2, 4, 8):
            nb = binned_order(pred, np.arange(N), bins)[1]
            add("(c) flat, %s, %d bins%s" % (pname, bins, "" if nb == bins else " (%d distinct)" % nb), cost_flat,
                lambda arr, pred=pred, bins=bins: binned_order(pred, arr, bins)[0])
    add("[bound] flat, sorted by the true turn count", cost_flat, lambda arr: sorted(arr, key=lambda k: -turns[k]))
    base_a, base_b = weigh(*rows["(a) nested, random pairs"]), weigh(*rows["(b) flat, random pairs"])
    print("%-72s %9s %9s %9s %12s %8s %8s" % ("per %d programs, mean of %d arrival orders" % (N, a.shuffles), "opens", "clips", "turns", "weighted", "vs (a)", "vs (b)"))
    for name, (r, form) in rows.items():
        w = weigh(r, form)
        print("%-72s %9.0f %9.0f %9.0f %12.0f %7.1f%% %7.1f%%" % (name, r[0], r[1], r[2], w, 100 * (w / base_a - 1), 100 * (w / base_b - 1)))
    print()
    print("corr(predictor, turns): nn - line_fail %.2f, violated at hand-over %.2f, combined %.2f" % tuple(
        np.corrcoef(p, turns)[0, 1] for p in (p_rest, p_viol, p_viol * 32 + p_rest)))
    best = min((weigh(*r), n) for n, r in rows.items() if n.startswith("(c)") and "[bound]" not in n)
    print("gate for the binned hand-over: best (c) must be >= 15 %% under (b): best is %.1f %% under (%s): %s" % (
        100 * (1 - best[0] / base_b), best[1], "PASSED" if best[0] <= 0.85 * base_b else "NOT PASSED"))


if __name__ == "__main__":
    main()
