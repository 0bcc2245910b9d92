"""Host side of the DS-RNN edge-sequence training kernels (cn_srnn_seq_fwd / cn_srnn_seq_bwd): the ABI surface, the workspace rule -- which
runs without a device -- and the CPU path of SRNNBase.forward_sequence, which the train_edge_kernels switch must not touch."""
import os
import re

import pytest

from crowdnav_prediction_attngraph_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cn_srnn_seq_workspace_bytes", "cn_srnn_seq_fwd", "cn_srnn_seq_bwd")


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "crowdnav_hip.h")).read()
    lib = A.lib()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, hdr), s
        assert s in A.ABI_SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes, s
    # cn_srnn_edge_grads: the twelve edge-RNN parameters, in cn_srnn_weights field order
    body = re.search(r"typedef struct \{([^}]*)\} cn_srnn_edge_grads;", hdr).group(1)
    assert re.findall(r"\*(\w+)", body) == [f for f, _ in A.SRNN_EDGE_KEYS] == [f for f, _ in A.SRNN_WEIGHT_KEYS[:12]]
    assert [f for f, _ in A.SrnnEdgeGrads._fields_] == [f for f, _ in A.SRNN_EDGE_KEYS]
    chunks = int(re.search(r"#define CN_SRNN_SEQ_CHUNKS (\d+)", hdr).group(1))
    assert A.SRNN_SEQ_PARTIALS_BYTES == chunks * (768 * 256 + 1024 * 80 + 64 * 80) * 4


def test_workspace_bytes_needs_no_device():
    ws = A.lib().cn_srnn_seq_workspace_bytes
    for T, N, H, D in ((1, 1, 1, 2), (30, 2048, 20, 2), (5, 3, 64, 12)):
        b = ws(T, N, H, D)
        # the gates (4 x 256) and the embedding (64) of every row and step, at least
        assert b >= T * N * (H + 1) * (4 * 256 + 64) * 4, (T, N, H, D)
        assert ws(T + 1, N, H, D) > b and ws(T, N + 1, H, D) > b
    # the training shape stays under the 21 GB peak of the torch-op update it replaces, by a wide margin
    assert ws(30, 2048, 20, 2) < 7 * 2 ** 30
    assert ws(30, 2048, 65, 2) == 0 and ws(30, 2048, 0, 2) == 0
    assert ws(30, 2048, 20, 0) == 0 and ws(30, 2048, 20, 65) == 0
    assert ws(0, 2048, 20, 2) == 0 and ws(30, 0, 20, 2) == 0
    # T * N * (H+1) * 1024 saved floats past 32-bit element offsets: 30 * 2^16 * 65 rows
    assert ws(30, 1 << 16, 64, 2) == 0 and ws(30, 1 << 10, 64, 2) > 0


def test_cpu_forward_sequence_ignores_the_switch():
    torch = pytest.importorskip("torch")
    from crowdnav_prediction_attngraph_amd.policy import SRNNBase
    from tests import srnn_seq_util as Q
    T, N, H, D = 4, 3, 5, 2
    pol, seq = Q.policy(H, D, N, T), Q.sequence(T, N, H, D)
    assert SRNNBase.train_edge_kernels in (True, False)
    outs = []
    for flag in (True, False):
        pol.base.train_edge_kernels = flag
        pol.zero_grad()
        v, lp, ent, hx = pol.evaluate_actions(seq["obs"], {"human_node_rnn": seq["node_h0"], "human_human_edge_rnn": seq["edge_h0"]}, seq["masks"],
                                              seq["actions"])
        (v.sum() + lp.sum() + ent).backward()
        outs.append([v.detach(), lp.detach(), hx["human_human_edge_rnn"].detach()] + [p.grad.clone() for p in pol.parameters() if p.grad is not None])
    assert len(outs[0]) == len(outs[1])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # the edge state it returns is the last step of the op loop
    assert torch.equal(outs[0][2], Q.op_loop(pol, seq, T, N, torch.float32)[-1].detach())
