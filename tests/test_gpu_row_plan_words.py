"""-m gpu: the row plan (csrc/row_plan.h) word for word, for fixed detected_human_num vectors.

tests/test_gpu_row_plan.py checks the invariants of a plan (every env in one tile, equal fill); a different packing with the same
invariants would pass it and change the bits of the policy's forward, whose fp32 sums follow the tile composition.  Here the whole buffer
-- header, row offsets, tile counts, item lists, and the zeros the builder leaves alone -- is compared with the words the builder wrote
before its chains were shortened (tests/golden/row_plan_words.npz, recorded through cn_row_plan_build, which runs the builder the lane
kernel hosts on counts of the caller's).

Cases: 256, 512, 1024 and 4096 envs of 20 rows (1, 2, 4 and 8 groups; 4, 4, 4 and 8 envs per lane of a group) and 512 envs of 5 and of 32
rows; each with every count 1, every count H, a seeded random vector that also holds 0 and H + 1 (both are clamped), and at 4096 envs the
first step of tools/det_counts_sample.npz (a real rollout's counts)."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "row_plan_words.npz")
SHAPES = ((256, 20), (512, 20), (1024, 20), (4096, 20), (512, 5), (512, 32))
MAGIC = 0x52504C4E


def det_vectors(E, H):
    """name -> float32 [E] counts of the case (E, H)."""
    v = {"ones": np.ones(E, np.float32), "full": np.full(E, H, np.float32),
         "random": np.random.RandomState(1000 * E + H).randint(0, H + 2, size=E).astype(np.float32)}
    if E == 4096:
        v["sample"] = np.load(os.path.join(ROOT, "tools", "det_counts_sample.npz"))["det"][0].astype(np.float32)
    return v


CASES = [(E, H, name) for E, H in SHAPES for name in det_vectors(E, H)]


def build_plan(det, E, H):
    """The plan of `det` as int32 numpy words, from a buffer that was zero before."""
    import torch
    from crowdnav_prediction_attngraph_amd import _abi as A
    L = A.lib()
    d = torch.from_numpy(np.ascontiguousarray(det, dtype=np.float32)).cuda()
    plan = torch.zeros(int(L.cn_row_plan_words(E)), dtype=torch.int32, device="cuda")
    A.check(L.cn_row_plan_build(E, H, d.data_ptr(), plan.data_ptr(), None))
    torch.cuda.synchronize()
    return plan.cpu().numpy()


def takes(det, E, H):
    """Whether the builder makes a plan of these counts: at most 1024 tiles (RP_TMAX) of n per workgroup."""
    total = int(np.clip(det.astype(np.int64), 1, H).sum())
    NW = min(256, max(1, (E * H + 15) // 16))
    return max(1, -(-total // (62 * NW))) * NW <= 1024


def key(E, H, name):
    return "e%d_h%d_%s" % (E, H, name)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.gpu
@pytest.mark.parametrize("E,H,name", CASES)
def test_the_plan_is_the_recorded_one_word_for_word(golden, E, H, name):
    pytest.importorskip("torch")
    det = det_vectors(E, H)[name]
    k = key(E, H, name)
    np.testing.assert_array_equal(golden[k + "_det"], det, err_msg="the case's counts are not the recorded ones")
    want = golden[k]
    if takes(det, E, H):
        assert want[0] == MAGIC and want[4] == E and want[5] == H, "the recorded plan is not a complete one"
    else:
        assert want[0] == 0     # (4096 envs with all 20 rows live: 1536 tiles, more than the builder holds -- "no plan", and still its words)
    got = build_plan(det, E, H)
    bad = np.flatnonzero(got != want)
    print("%s: %d of %d words differ%s" % (k, len(bad), len(want), "".join(" [%d] %d != %d" % (i, got[i], want[i]) for i in bad[:8])))
    np.testing.assert_array_equal(got, want)


@pytest.mark.gpu
def test_the_stand_alone_builder_writes_the_plan_of_the_step():
    """cn_row_plan_build on the counts of a real observation equals the plan the step wrote beside it: the door the cases above go through
    leads to the builder the simulator runs."""
    torch = pytest.importorskip("torch")
    from crowdnav_prediction_attngraph_amd import _abi as A
    from crowdnav_prediction_attngraph_amd.hip import HipEnvBatch
    E, H = 1024, 20
    env = HipEnvBatch(A.default_env_config(human_num=H, nenv=E), E, 425)
    obs = env.reset()
    for _ in range(3):
        obs = env.step(torch.zeros(E, 2, device="cuda"))[0]
    torch.cuda.synchronize()
    want = env.row_plan.cpu().numpy()
    got = build_plan(obs["detected_human_num"].view(E).cpu().numpy(), E, H)
    assert want[0] == MAGIC
    # (the step's buffer keeps the items of earlier plans behind each list's terminator: compare what a consumer reads)
    oc = 8 + ((E + 1 + 3) & ~3)
    np.testing.assert_array_equal(got[:oc], want[:oc])
    T = int(want[6])
    np.testing.assert_array_equal(got[oc:oc + T], want[oc:oc + T])
    items_g, items_w = got[oc + 1024:].reshape(1024, 64), want[oc + 1024:].reshape(1024, 64)
    for t in range(T):
        n = int(want[oc + t])
        np.testing.assert_array_equal(items_g[t, :n + 1], items_w[t, :n + 1], err_msg="tile %d" % t)
    env.close()
