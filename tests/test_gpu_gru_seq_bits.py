"""-m gpu: the GRU sequence pair (cn_gru_seq_fwd_sized / cn_gru_seq_bwd_sized, csrc/gru_seq.h) gives the bits recorded in
tests/golden/gru_seq_bits.json -- sha256 digests of hs, hms, gates, dgi, dgh, dh0 written by tests/golden/make_golden_gru_bits.py from the build of
the commit the file names, before the R = 128 kernels and the R = 64 / 192 / 256 template became one.  R = 128 is the default network (checkpoints,
bench.py, every golden); the other R are policy_sizes training.  Inputs, cases and the guarded run live in the generator and are shared with it."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.golden import make_golden_gru_bits as G  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gru_seq_bits.json")) as f:
        return json.load(f)


def test_the_golden_file_holds_every_case_and_names_its_commit(golden):
    assert sorted(golden["cases"]) == sorted(G.case_id(c) for c in G.CASES)
    assert len(golden["commit"]) == 40 and golden["arrays"] == list(G.ARRAYS)
    assert all(sorted(d) == sorted(G.ARRAYS) for d in golden["cases"].values())


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_gru_sequence_pair_gives_the_recorded_bits(case, golden):
    inp = G.inputs(*case)
    first, again = G.run(*case, inp), G.run(*case, inp)
    for k in G.ARRAYS:
        assert torch.equal(first[k], again[k]), "%s differs between two calls on the same inputs" % k
    got, want = G.digests(first), golden["cases"][G.case_id(case)]
    wrong = [k for k in G.ARRAYS if got[k] != want[k]]
    assert not wrong, "%s: other bits than commit %s gave in %s" % (G.case_id(case), golden["commit"][:7], wrong)
