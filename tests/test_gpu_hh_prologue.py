"""-m gpu: the head of the fused human-human kernel (csrc/hh_fused.hip) -- the launch prologue that takes a row plan in one batch of
loads, and the input phase (e0) of every tile -- at the smallest shapes where its paths differ: batch sizes around the unrolled
verification (512 threads x 8 envs), one / several / no tile per workgroup, four-row-block tiles, the input widths, a stale plan.

The forward is compared with oracle/policy_oracle.py at the 1e-4 of tests/test_gpu_policy.py (same weights, same helpers).  Plans are
written by _make_plan below in the documented layout of csrc/row_plan.h (any packing of whole envs into tiles of <= 63 rows is a plan the
kernel accepts), so that detected_human_num can be chosen freely -- 0 included, which the library counts as one (dummy) row -- and one
case takes the plan the simulator itself built."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import policy_util as PU  # noqa: E402
from tests.golden_util import GOLDEN  # noqa: E402
from tests.test_gpu_policy import TOL, _dev, _sd_dev  # noqa: E402

MAGIC, TMAX, HDR = 0x52504C4E, 1024, 8
KEYS = ("value", "action", "logp", "hxs")


def _workgroups(E, H):
    return max(1, min(256, (E * H + 15) // 16))


def _make_plan(det, E, H, pack="even"):
    """int32 plan of csrc/row_plan.h for the counts `det`: header | row_off[E + 1] (padded to 4) | tile_cnt[1024] | items[1024][64]; item =
    env | rows << 16, a list ends with a zero item; tile t belongs to workgroup t % NW.  Envs go largest first to the emptiest tile
    ("even") or to the first tile with room ("first": full tiles in front, empty lists behind them)."""
    rows = np.clip(det.astype(np.int64), 1, H)
    NW = _workgroups(E, H)
    total = int(rows.sum())
    n = max(1, -(-total // (62 * NW)))
    T = n * NW
    assert T <= TMAX
    off_t = HDR + ((E + 1 + 3) & ~3)
    off_i = off_t + TMAX
    plan = np.zeros(off_i + TMAX * 64, dtype=np.int32)
    plan[HDR + 1:HDR + E + 1] = np.cumsum(rows)
    load, cnt = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
    for e in np.argsort(-rows, kind="stable"):
        ok = np.where((load + rows[e] <= 63) & (cnt < 63))[0]
        t = ok[np.argmin(load[ok])] if pack == "even" else ok[0]
        plan[off_i + t * 64 + cnt[t]] = int(e) | (int(rows[e]) << 16)
        cnt[t] += 1
        load[t] += rows[e]
    plan[off_t:off_t + T] = cnt
    plan[:HDR] = [MAGIC, NW, n, total, E, H, T, 0]
    return plan, load.reshape(n, NW)


def _policy(E, H, D):
    from crowdnav_prediction_attngraph_amd.hip import HipPolicy
    shapes = json.loads(str(np.load(os.path.join(GOLDEN, "policy_varnum_e4_h20.npz"))["meta"]))["shapes"]
    shapes["base.spatial_attn.embedding_layer.0.weight"] = [128, D]
    sd, sdd = _sd_dev(shapes)
    pol = HipPolicy(H, D, E)     # default mode: fused
    pol.set_weights(sdd)
    return sd, pol


def _inputs(E, H, D, det, seed):
    """PU.synth_obs with the counts `det`: the rows the library looks at (clamp(det, 1, H) per env) hold positions like synth_obs's own,
    the rest the padding value 15."""
    obs = PU.synth_obs(E, H, D, seed=seed)
    rs = np.random.RandomState(seed + 1)
    spatial = np.full((E, H, D), 15.0, dtype=np.float32)
    for e, n in enumerate(np.clip(det, 1, H)):
        p = rs.uniform(-4, 4, (n, 2))
        p = p[np.argsort(np.linalg.norm(p, axis=1))]
        v = rs.uniform(-1, 1, (n, 2))
        for k in range(D // 2):
            spatial[e, :n, 2 * k:2 * k + 2] = p + 0.25 * k * v
        if D & 1:
            spatial[e, :n, D - 1] = p[:, 0] + 0.25 * (D // 2) * v[:, 0]
    obs["spatial_edges"] = spatial
    obs["detected_human_num"] = det.astype(np.float32).reshape(E, 1)
    hxs = rs.uniform(-1, 1, (E, 1, 128)).astype(np.float32)
    masks = (rs.uniform(size=(E, 1)) > 0.2).astype(np.float32)
    eps = rs.standard_normal((E, 2)).astype(np.float32)
    return obs, hxs, masks, eps


def _reference(sd, obs, hxs, masks, eps, H):
    from oracle import policy_oracle as P
    E = hxs.shape[0]
    o = dict(obs)
    o["detected_human_num"] = np.clip(obs["detected_human_num"], 1, H)   # no detected human = one dummy row (crowd_sim_var_num.py:290-292)
    value, mean, _, h_new, _ = P.act(sd, o, hxs.reshape(E, 128), masks)
    std = np.exp(sd["dist.logstd._bias"].astype(np.float64).reshape(1, 2))
    action = mean + std * eps
    return dict(value=value, action=action, logp=P.log_prob(mean, np.log(std), action), hxs=h_new)


def _act(pol, obs, hxs, masks, eps, plan):
    out = pol.act(_dev(obs), torch.from_numpy(hxs).cuda(), torch.from_numpy(masks).cuda(), eps=torch.from_numpy(eps).cuda(),
                  row_plan=None if plan is None else torch.from_numpy(plan).cuda())
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy().reshape(out[k].shape[0], -1) for k in KEYS}


def _check(got, ref, what):
    for k in KEYS:
        err = float(np.abs(got[k] - ref[k]).max())
        print("%s %s: max abs error %.2e" % (what, k, err))
        assert err <= TOL, (what, k, err)


def _both_paths_match_the_oracle(E, H, D, det, seed, pack="even"):
    sd, pol = _policy(E, H, D)
    obs, hxs, masks, eps = _inputs(E, H, D, det, seed)
    ref = _reference(sd, obs, hxs, masks, eps, H)
    plan, load = _make_plan(det, E, H, pack)
    _check(_act(pol, obs, hxs, masks, eps, plan), ref, "planned")
    _check(_act(pol, obs, hxs, masks, eps, None), ref, "no plan")
    pol.close()
    return load


@pytest.mark.parametrize("E", [4, 260, 516])
def test_ragged_verification_batches(E):
    """Every thread of a workgroup checks envs tid, tid + 512, ... of the plan against detected_human_num: 4 envs use a few lanes of one
    wavefront, 260 end inside the first round, 516 four envs into the second.  Counts 0..H."""
    H = 20
    det = np.random.RandomState(E).randint(0, H + 1, size=E)
    _both_paths_match_the_oracle(E, H, 2, det, seed=E)


def test_simulator_plan_small_batch():
    """The plan the simulator wrote beside its own observation (one builder group at 260 envs)."""
    from crowdnav_prediction_attngraph_amd import _abi as A
    from crowdnav_prediction_attngraph_amd.hip import HipEnvBatch
    E, H = 260, 20
    env = HipEnvBatch(A.default_env_config(human_num=H, nenv=E), E, 425)
    obs = env.reset()
    for t in range(8):
        obs = env.step(torch.full((E, 2), 0.3, device="cuda"))[0]
    assert int(env.row_plan[0]) == MAGIC
    sd, pol = _policy(E, H, 2)
    keys = ("robot_node", "temporal_edges", "spatial_edges", "detected_human_num")
    ob_np = {k: obs[k].cpu().numpy() for k in keys}
    _, hxs, masks, eps = _inputs(E, H, 2, np.ones(E, dtype=np.int64), seed=3)
    ref = _reference(sd, ob_np, hxs, masks, eps, H)
    _check(_act(pol, ob_np, hxs, masks, eps, env.row_plan.cpu().numpy()), ref, "simulator plan")
    env.close()
    pol.close()


@pytest.mark.parametrize("case", ["e512_random", "e1024_all", "e512_mostly_empty"])
def test_tile_sequences(case):
    """Workgroups with one tile and with none (512 random envs packed into full tiles: fewer tiles than workgroups), with several tiles
    (1024 x 20 rows = 2 tiles each, so a tile's successor is requested inside it and the last tile has none), and tiles of one-row envs
    (most counts 0: up to 63 envs per list, and lists that are empty -- the "fewer envs than tiles" branch)."""
    H = 20
    if case == "e512_random":
        E = 512
        det = np.random.RandomState(7).randint(0, H + 1, size=E)
    elif case == "e1024_all":
        E = 1024
        det = np.full(E, H)
    else:
        E = 512
        det = np.where(np.random.RandomState(8).uniform(size=E) < 0.9, 0, H)
    load = _both_paths_match_the_oracle(E, H, 2, det, seed=11, pack="even" if case == "e1024_all" else "first")
    if case == "e1024_all":
        assert load.shape[0] >= 2 and (load[1] > 0).all()
    else:
        assert (load == 0).any() and (load > 0).any()


@pytest.mark.parametrize("H", [57, 63])
def test_four_row_block_tiles(H):
    """Crowds of 49..63 humans: a tile is one env of four row blocks, the LDS holds nothing but X and the shared scratch region.  (No plan
    exists beyond 32 rows per env: the scan path, with the direct loads of e0.)"""
    E = 8
    sd, pol = _policy(E, H, 2)
    obs, hxs, masks, eps = _inputs(E, H, 2, np.full(E, H), seed=H)
    ref = _reference(sd, obs, hxs, masks, eps, H)
    _check(_act(pol, obs, hxs, masks, eps, None), ref, "H = %d" % H)
    pol.close()


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 7, 12, 14, 16])
def test_input_widths(D):
    """e0 takes its inputs four features at a time: one batch of loads for D = 2 and 4, three for 12, three and a half-filled fourth for
    14, four for 16; an odd width (the entries take every width from 1) ends on a single feature: 1 alone, 3 = a pair + 1, 5 = a full
    batch + 1, 7 = a batch, a pair + 1.  (The library takes edge widths up to 16 -- cn_policy_create and cn_hh_block_fwd refuse more -- so the 18 of the widest
    prediction env never reaches this kernel; 14 and 16 stand in for what it would exercise.)"""
    E, H = 64, 20
    det = np.random.RandomState(D).randint(0, H + 1, size=E)
    _both_paths_match_the_oracle(E, H, D, det, seed=D)


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 7, 12, 14, 16])
def test_input_widths_training_entry(D):
    """The same e0 code in the training instantiation (cn_hh_block_fwd), which writes e0 and X out: both against float64 numpy on the
    compacted rows."""
    from crowdnav_prediction_attngraph_amd import _abi as A
    B, H = 64, 20
    g = torch.Generator(device="cuda").manual_seed(D)
    se = torch.randn(B, H, D, device="cuda", generator=g)
    det = torch.randint(1, H + 1, (B,), device="cuda", generator=g)
    det[0], det[-1] = 1, H
    nd = det.to(torch.int32)
    row_off = torch.cat([nd.new_zeros(1), nd.cumsum(0, dtype=torch.int32)])
    R = int(row_off[-1])
    w = [torch.randn(128, D, device="cuda", generator=g) / D ** 0.5, torch.randn(128, device="cuda", generator=g) * 0.1,
         torch.randn(512, 128, device="cuda", generator=g) / 128 ** 0.5, torch.randn(512, device="cuda", generator=g) * 0.1,
         torch.randn(1536, 512, device="cuda", generator=g) * 0.05, torch.randn(1536, device="cuda", generator=g) * 0.1,
         torch.randn(256, 512, device="cuda", generator=g) * 0.05, torch.randn(256, device="cuda", generator=g) * 0.1]
    L = A.lib()
    ws = torch.empty(int(L.cn_hh_block_workspace_bytes()), dtype=torch.uint8, device="cuda")
    outs = [torch.zeros(R, n, device="cuda") for n in (128, 512, 1536, 512, 256)]
    A.check(L.cn_hh_block_fwd(B, H, D, A.ptr(se), A.ptr(row_off), *[A.ptr(t) for t in w], 0.125, A.ptr(ws), *[A.ptr(t) for t in outs], A.stream_ptr()),
            "cn_hh_block_fwd")
    torch.cuda.synchronize()
    live = (torch.arange(H, device="cuda").view(1, H) < det.view(B, 1)).cpu().numpy()
    x = se.cpu().numpy().astype(np.float64)[live]                      # [R, D], env-major = the compacted order
    wn = [t.cpu().numpy().astype(np.float64) for t in w[:4]]
    e0 = np.maximum(x @ wn[0].T + wn[1], 0.0)
    xx = np.maximum(e0 @ wn[2].T + wn[3], 0.0)
    for name, got, ref in (("e0", outs[0], e0), ("x", outs[1], xx)):
        err = float(np.abs(got.cpu().numpy() - ref).max())
        print("D = %d %s: max abs error %.2e" % (D, name, err))
        assert err <= TOL, (name, err)


def test_well_formed_stale_plan_equals_no_plan():
    """The plan of observation A with observation B of the same shape: every item is a valid env, only the counts differ.  The kernel must
    refuse it and compute exactly what it computes without a plan."""
    E, H, D = 516, 20, 2
    rs = np.random.RandomState(5)
    det_a, det_b = rs.randint(0, H + 1, size=E), rs.randint(0, H + 1, size=E)
    assert (np.clip(det_a, 1, H) != np.clip(det_b, 1, H)).any()
    sd, pol = _policy(E, H, D)
    plan_a, _ = _make_plan(det_a, E, H)
    obs, hxs, masks, eps = _inputs(E, H, D, det_b, seed=6)
    stale = _act(pol, obs, hxs, masks, eps, plan_a)
    sl_stale = pol.taps(E)["spatial_lin"].clone()
    none = _act(pol, obs, hxs, masks, eps, None)
    sl_none = pol.taps(E)["spatial_lin"]
    live = torch.arange(H, device="cuda").view(1, H) < torch.from_numpy(np.clip(det_b, 1, H)).cuda().view(E, 1)
    assert torch.equal(sl_stale[live], sl_none[live])      # out_sp (padded rows are not materialised)
    for k in KEYS:
        assert np.array_equal(stale[k], none[k]), k
    # (An ACCEPTED plan is visible in the bits: the order in which a row's heads are summed follows from the index of the workgroup that
    # holds the row, and the plan deals the envs to other workgroups than the scan does.  Equal bits above therefore mean "refused", and
    # the plan of observation B itself must show a difference -- or the hand-written plans of this file are not being taken at all.)
    plan_b, _ = _make_plan(det_b, E, H)
    _act(pol, obs, hxs, masks, eps, plan_b)
    sl_fresh = pol.taps(E)["spatial_lin"]
    assert float((sl_fresh[live] - sl_none[live]).abs().max()) <= TOL and not torch.equal(sl_fresh[live], sl_none[live])
    # ... and one differing count is enough, in the last env the second verification round looks at
    det_c = det_b.copy()
    det_c[E - 1] = max(int(det_b[E - 1]), 1) % H + 1
    plan_c, _ = _make_plan(det_c, E, H)
    one = _act(pol, obs, hxs, masks, eps, plan_c)
    for k in KEYS:
        assert np.array_equal(one[k], none[k]), k
    pol.close()


def test_planned_launches_repeat_bit_for_bit():
    """Twenty launches of the two-tiles-per-workgroup case on unchanged inputs: the plan's loads that travel inside a tile (the next
    tile's items, the output rows) are asynchronous to the tile's work -- a missing wait shows as a difference."""
    E, H, D = 1024, 20, 2
    det = np.full(E, H)
    sd, pol = _policy(E, H, D)
    obs, hxs, masks, eps = _inputs(E, H, D, det, seed=11)
    plan, _ = _make_plan(det, E, H)
    od, pd = _dev(obs), torch.from_numpy(plan).cuda()
    hd, md, ed = torch.from_numpy(hxs).cuda(), torch.from_numpy(masks).cuda(), torch.from_numpy(eps).cuda()
    first = None
    for it in range(20):
        out = pol.act(od, hd, md, eps=ed, row_plan=pd)
        got = {k: out[k].clone() for k in KEYS}
        got["spatial_lin"] = pol.taps(E)["spatial_lin"].clone()
        if first is None:
            first = got
        else:
            for k in got:
                assert torch.equal(got[k], first[k]), (k, it)
    pol.close()
