"""The robot-node sequence of the training path at off-default network sizes, the part that needs no GPU: the sized C entry points exist and are
bound, their host-only workspace functions agree with the unsized ones at the default sizes and return 0 outside the device box, the weight
shapes as a function of (R, M, A, O), the table of code paths each tuple of tests/test_gpu_rn_seq_sizes.py reaches, and two properties that
GPU test relies on: its reference graph on the folded weights IS the definition (Policy(...).double() in torch ops), and the fp32 mirror stays
inside every bar asserted against the fp64 graph at its shapes."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from crowdnav_prediction_attngraph_amd import _abi as A  # noqa: E402
from tests import rn_seq_util as U  # noqa: E402

SIZED = ["cn_rn_seq_fwd_sized", "cn_rn_seq_bwd_sized", "cn_rn_seq_workspace_floats_sized", "cn_rn_seq_fwd_workspace_floats_sized"]


def test_the_sized_symbols_are_exported_and_bound():
    L = A.lib()
    for name in SIZED + ["cn_gru_seq_fwd_sized", "cn_gru_seq_bwd_sized"]:
        assert name in A.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None, name
    assert L.cn_rn_seq_workspace_floats_sized.restype is C.c_int64 and L.cn_rn_seq_fwd_workspace_floats_sized.restype is C.c_int64
    assert len(L.cn_rn_seq_fwd_sized.argtypes) == len(L.cn_rn_seq_fwd.argtypes) + 1
    assert len(L.cn_rn_seq_bwd_sized.argtypes) == len(L.cn_rn_seq_bwd.argtypes) + 1


def test_workspaces_equal_the_unsized_ones_at_the_default_and_are_zero_outside_the_box():
    L = A.lib()
    d = A.PolicyDims(*A.DEFAULT_DIMS)
    assert L.cn_rn_seq_fwd_workspace_floats_sized(C.byref(d)) == L.cn_rn_seq_fwd_workspace_floats() > 0
    assert L.cn_rn_seq_fwd_workspace_floats_sized(None) == L.cn_rn_seq_fwd_workspace_floats()
    for T, N in ((1, 1), (3, 17), (5, 4), (30, 2048)):
        assert L.cn_rn_seq_workspace_floats_sized(T, N, C.byref(d)) == L.cn_rn_seq_workspace_floats(T, N) > 0
    for bad in ((96, 64, 64, 256), (128, 32, 64, 256), (128, 64, 64, 576), (128, 64, 0, 256)):
        b = A.PolicyDims(*bad)
        assert L.cn_rn_seq_fwd_workspace_floats_sized(C.byref(b)) == 0, bad
        assert L.cn_rn_seq_workspace_floats_sized(3, 17, C.byref(b)) == 0, bad
    # inside the box every tuple has a plan, and larger sizes never need less
    sizes = [L.cn_rn_seq_workspace_floats_sized(3, 17, C.byref(A.PolicyDims(*dims))) for dims in U.DIMS]
    assert all(s > 0 for s in sizes) and sizes[1] == max(sizes) and sizes[0] == min(sizes)
    assert L.cn_rn_seq_workspace_floats_sized(0, 17, C.byref(d)) == 0


def test_weight_shapes_are_a_function_of_the_dims():
    assert A.rn_weight_shapes() == A.RN_WEIGHT_SHAPES == A.rn_weight_shapes(A.DEFAULT_DIMS)
    assert len(A.RN_WEIGHT_SHAPES) == len(A.RN_WEIGHT_FIELDS)
    for dims in U.DIMS:
        pol = U.sized_policy(dims, 5)
        ws = U.folded_weights(pol)
        assert [tuple(w.shape) for w in ws] == A.rn_weight_shapes(dims), dims
        R, M, _, O = dims
        assert A.rn_saved_widths(dims, 5) == dict(rs=256, z=256 + 2 * M, hr=256, attn=5, gi=3 * R, hs=R, hms=R, gates=4 * R, a1=2 * O, a2=2 * O)
    with pytest.raises(NotImplementedError, match="device box"):
        A.rn_weight_shapes((96, 64, 64, 256))


def test_the_case_table_reaches_what_it_claims():
    for dims in U.DIMS:
        p = A.rn_seq_plan(dims)
        want = U.PLAN[dims]
        print("%-22s padded N %-60s K%%128 %-50s GRU %-11s head strides %d" % (dims, dict(p["padded_n"]), dict(p["ragged_k"]), p["gru"], p["head_strides"]))
        assert dict(p["padded_n"]) == want["padded_n"] and dict(p["ragged_k"]) == want["ragged_k"], dims
        assert p["gru"] == want["gru"] and p["head_strides"] == want["head_strides"] and p["gru_rows"] == 16
        # the products stay inside what the kernels take: padded widths and ragged K are multiples of 64
        assert all(n % 64 == 0 and n % 128 for n in dict(p["padded_n"]).values()) and all(k % 128 == 64 for k in dict(p["ragged_k"]).values())
    plans = [A.rn_seq_plan(d) for d in U.DIMS]
    # the table as a whole: all three GRU kernels, every padded product and every ragged-K gradient, the smallest and the largest head
    assert {p["gru"] for p in plans} == {"resident128", "resident", "streamed"}
    assert set().union(*[dict(p["padded_n"]) for p in plans]) == {"te", "gi", "a2", "c2", "d1_a", "d1_c", "dhs"}
    assert set().union(*[dict(p["ragged_k"]) for p in plans]) == {"a2_w", "c2_w", "ac0_w", "whh"}
    assert {p["head_strides"] for p in plans} >= {1, 4, 5, 7, 8}
    # the shapes: GRU workgroups past one and past two with a ragged last one, sample counts that leave a weight-gradient row tail
    rows = plans[0]["gru_rows"]
    assert {-(-N // rows) for _, N, _ in U.SHAPES} >= {2, 3} and all(N % rows for _, N, _ in U.SHAPES)
    assert all((T * N) % 32 for T, N, _ in U.SHAPES) and {T for T, _, _ in U.SHAPES} >= {1, 3} and {H for _, _, H in U.SHAPES} == {1, 5}
    for dims, (T, N, H) in U.CASES:
        inp = U.make_inputs(dims, T, N, H)
        assert inp["det"].min() == 1 and inp["det"].max() == H and inp["det"][0] == 1
        m = inp["masks"].reshape(T, N)
        assert T < 3 or (m[1, 1] == 0 and m[2, 2] == 0 and m[1:].sum() == (T - 1) * N - 2)


@pytest.mark.parametrize("dims", U.DIMS, ids=str)
def test_the_folded_graph_is_the_mirrors_definition(dims):
    """graph() on the folded weights against Policy(...).double(): forward_sequence + the DiagGaussian head in torch ops, with the human-human
    block replaced by the synthetic out_sp."""
    T, N, H = 3, 5, 5
    pol = U.sized_policy(dims, H).double()
    inp = U.make_inputs(dims, T, N, H)
    t = lambda x: torch.from_numpy(np.asarray(x)).double()   # noqa: E731
    pol.base._hh_block = lambda se, det: (t(inp["out_sp"]), torch.from_numpy(inp["valid"]))
    B = T * N
    obs = dict(robot_node=t(inp["robot_node"]).view(B, 1, 7), temporal_edges=t(inp["temporal"]).view(B, 1, 2), spatial_edges=torch.zeros(B, H, 2).double(),
               detected_human_num=t(inp["det"]).view(B, 1))
    with torch.no_grad():
        value, feat, h = pol.base.forward_sequence(obs, t(inp["h0"]), t(inp["masks"]).view(B, 1), T, N)
        mean = pol.dist.fc_mean(feat)
        logp = pol._log_prob(mean, pol.dist.logstd(torch.zeros_like(mean)).exp(), t(inp["actions"]))
    got = U.run_graph(U.folded_weights(pol), inp, dims, T, N, H, torch.float64)
    for a, b, what in ((got["value"], value, "value"), (got["logp"], logp, "logp"), (got["h_T"], h, "h_T")):
        err = float(np.abs(a.reshape(-1) - b.numpy().reshape(-1)).max())
        assert err <= 1e-12, (what, err)


@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_the_fp32_mirror_holds_every_bar_of_the_gpu_test(case):
    """The distance fp32 graph -- fp64 graph at the GPU test's weights, inputs and shapes, against the bars that test asserts: a fraction of each,
    so that the bars leave the kernels' bf16x3 products (about fp32's own rounding) room and no tensor's terms cancel below them."""
    dims, (T, N, H) = case
    ws = U.folded_weights(U.sized_policy(dims, H).double())
    inp = U.make_inputs(dims, T, N, H)
    ref = U.run_graph(ws, inp, dims, T, N, H, torch.float64)
    got = U.run_graph(ws, inp, dims, T, N, H, torch.float32)
    worst = 0.0
    for k, r in ref.items():
        bar = U.VALUE_BAR if k in ("value", "logp", "h_T") else U.grad_bar(r)
        err = float(np.abs(got[k] - r).max())
        worst = max(worst, err / bar)
        assert np.isfinite(r).all() and err <= 0.25 * bar, (k, err, bar)
    print("%s: fp32 mirror at most %.3f of a bar from the fp64 graph" % (U.case_id(case), worst))
