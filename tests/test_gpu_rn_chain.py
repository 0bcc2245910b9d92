"""-m gpu: the fused robot-node kernel (rn_fused.hip) at the edges of its workgroup of 16 envs and of the attention's chunks of 8 rows,
with and without noise, with the taps on and off, against the numpy oracle at the project's bar."""
import functools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import policy_util as PU  # noqa: E402
from tests.golden_util import GOLDEN  # noqa: E402

TOL = 1e-4
D = 2
# row counts at the edges of the attention's chunks of 8, all inside the first workgroup (envs 0..15) when the batch has that many envs
DET_EDGES = [1, 7, 8, 9, 16, 17, 20]
# tail workgroup (1, 15), exactly one (16), two (17) and three (33) workgroups
CASES = [(1, 20), (15, 20), (16, 20), (17, 20), (33, 20), (17, 5)]


def _inputs(E, H):
    """Observation with the row counts of DET_EDGES (clipped to H) in the leading envs and random counts behind them; hidden state, done masks
    with zeros and ones mixed inside every workgroup, noise."""
    rs = np.random.RandomState(1000 * E + H)
    det = rs.randint(1, H + 1, size=E)
    k = min(E, len(DET_EDGES))
    det[:k] = np.minimum(DET_EDGES[:k], H)
    obs = PU.synth_obs(E, H, D, seed=E + H)
    spatial = np.full((E, H, D), 15.0, dtype=np.float32)
    for e in range(E):
        p = rs.uniform(-4, 4, (det[e], 2))
        spatial[e, :det[e]] = p[np.argsort(np.linalg.norm(p, axis=1))]
    obs["spatial_edges"] = spatial
    obs["detected_human_num"] = det.astype(np.float32).reshape(E, 1)
    hxs = rs.uniform(-1, 1, (E, 1, 128)).astype(np.float32)
    masks = (np.arange(E) % 3 != 1).astype(np.float32).reshape(E, 1)   # 1, 0, 1, 1, 0, ...
    if E > 1:
        assert masks.min() == 0.0 and masks.max() == 1.0
    eps = rs.standard_normal((E, 2)).astype(np.float32)
    return obs, hxs, masks, eps


@functools.lru_cache(maxsize=None)
def _weights():
    shapes = json.loads(str(np.load(os.path.join(GOLDEN, "policy_varnum_e4_h20.npz"))["meta"]))["shapes"]
    shapes["base.spatial_attn.embedding_layer.0.weight"] = [128, D]
    return PU.formula_state_dict({k: tuple(v) for k, v in shapes.items()})


@functools.lru_cache(maxsize=None)
def _reference(E, H):
    """The oracle's forward of _inputs(E, H), computed once and shared: value, mean, h_new, actor features, taps."""
    from oracle import policy_oracle as P
    obs, hxs, masks, _ = _inputs(E, H)
    taps = {}
    value, mean, _, h_new, feat = P.act(_weights(), obs, hxs.reshape(E, 128), masks, taps=taps)
    return value, mean, h_new, feat, taps


def _run(pol, E, H, with_eps):
    obs, hxs, masks, eps = _inputs(E, H)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in obs.items()}
    out = pol.act(dev, torch.from_numpy(hxs).cuda(), torch.from_numpy(masks).cuda(), eps=torch.from_numpy(eps).cuda() if with_eps else None)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("with_eps", [True, False], ids=["eps", "mode"])
@pytest.mark.parametrize("E,H", CASES, ids=lambda v: str(v))
def test_rn_chain_matches_oracle_taps_on_and_off(E, H, with_eps):
    from crowdnav_prediction_attngraph_amd.hip import HipPolicy
    from oracle import policy_oracle as P
    sd = _weights()
    pol = HipPolicy(H, D, E)
    pol.set_gemm_mode("fused")
    pol.set_weights({k: torch.from_numpy(v).cuda() for k, v in sd.items()})
    try:
        on = _run(pol, E, H, with_eps)                      # the library's default: taps on
        taps = {k: v.cpu().numpy() for k, v in pol.taps(E).items()}
        on2 = _run(pol, E, H, with_eps)
        pol.set_taps(False)
        off = _run(pol, E, H, with_eps)
        off2 = _run(pol, E, H, with_eps)
    finally:
        pol.close()
    value, mean, h_new, feat, otaps = _reference(E, H)
    _, _, _, eps = _inputs(E, H)
    logstd = sd["dist.logstd._bias"].astype(np.float64).reshape(1, 2)
    action = mean + np.exp(logstd) * eps if with_eps else mean
    logp = P.log_prob(mean, np.broadcast_to(logstd, mean.shape), action)
    for name, got in (("taps on", on), ("taps off", off)):
        np.testing.assert_allclose(got["value"], value, atol=TOL, rtol=0, err_msg=name)
        np.testing.assert_allclose(got["action"], action, atol=TOL, rtol=0, err_msg=name)
        np.testing.assert_allclose(got["logp"], logp, atol=TOL, rtol=0, err_msg=name)
        np.testing.assert_allclose(got["hxs"].reshape(E, 128), h_new, atol=TOL, rtol=0, err_msg=name)
    for k in ("value", "action", "logp", "hxs"):
        assert np.array_equal(on[k], off[k]), "taps on / off differ in " + k
        assert np.array_equal(on[k], on2[k]), "taps on: two forwards differ in " + k
        assert np.array_equal(off[k], off2[k]), "taps off: two forwards differ in " + k
    np.testing.assert_allclose(taps["robot_emb"], otaps["robot_emb"], atol=TOL, rtol=0)
    np.testing.assert_allclose(taps["hr_attn"], otaps["hr_attn"], atol=TOL, rtol=0)
    np.testing.assert_allclose(taps["hr_out"], otaps["hr_out"], atol=TOL, rtol=0)
    np.testing.assert_allclose(taps["actor_feat"], feat, atol=TOL, rtol=0)
