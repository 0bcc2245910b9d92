"""Shared by tests/test_train_wide_cases.py (CPU) and tests/test_gpu_train_wide.py (-m gpu): the ReLU gates of the training path, recorded on
the GPU route and imposed on the fp64 torch-op graph.

A ReLU unit whose pre-activation is within rounding of zero takes one gate on the GPU and the other in fp64; one such unit moves a bias
gradient by a whole row's entry with no kernel at fault (see the top of tests/test_gpu_minibatch_edges.py).  Comparing gradients at the SAME
gates removes that by construction: the GPU's gates of the human-human block's three ReLUs are read off the per-layer Functions' outputs and the
fp64 graph multiplies by them in place of its own relu, after the gates themselves have been held to fp64's wherever the pre-activation is
further than the forward bar from zero.

One Policy.evaluate_actions of the attention-graph network on CPU tensors calls torch.nn.functional.relu six times, in this order (RELU_CALLS):
robot_linear [B,256], embedding_layer.0 [rows,128], embedding_layer.2 [rows,512], spatial_linear.0 [rows,256], encoder_linear [B,64],
edge_attention_embed [B,64]; calls 1..3 are the block's, on the live rows in the order of row_off."""
import contextlib

RELU_CALLS = ("robot_linear", "e0", "e", "out_sp", "encoder", "edge_attention_embed")
BLOCK = (1, 2, 3)                       # the gate-imposed calls; the others (B x 384 units) run inside one kernel on the GPU and cannot be recorded


def record_gpu_gates(monkeypatch):
    """Wrap hip_train.Embed0.apply and hip_train.HipLinear.apply: the returned list receives [y > 0] (bool, on the host) of every Embed0 call and
    of every HipLinear call with relu = True, in call order -- e0, e, out_sp for one pass through the per-layer human-human block."""
    from crowdnav_prediction_attngraph_amd import hip_train
    gates = []
    embed0, linear = hip_train.Embed0.apply, hip_train.HipLinear.apply

    def embed0_rec(x, w, b):
        y = embed0(x, w, b)
        gates.append((y.detach() > 0).cpu())
        return y

    def linear_rec(x, w, b, relu):
        y = linear(x, w, b, relu)
        if relu:
            gates.append((y.detach() > 0).cpu())
        return y
    monkeypatch.setattr(hip_train.Embed0, "apply", embed0_rec)
    monkeypatch.setattr(hip_train.HipLinear, "apply", linear_rec)
    return gates


@contextlib.contextmanager
def relu_taps(gates=None):
    """Inside the block torch.nn.functional.relu records its argument (detached) in the yielded list, one entry per call; with `gates` (three bool
    tensors: e0, e, out_sp) calls 1..3 of every group of six return x * gate instead of relu(x)."""
    import torch.nn.functional as F
    real, pre = F.relu, []

    def relu(x, inplace=False):
        k = len(pre) % len(RELU_CALLS)
        pre.append(x.detach().clone())
        if gates is not None and k in BLOCK:
            g = gates[k - 1]
            assert g.shape == x.shape, (RELU_CALLS[k], tuple(g.shape), tuple(x.shape))
            return x * g.to(x.dtype)
        return real(x)
    F.relu = relu
    try:
        yield pre
    finally:
        F.relu = real


def gate_differences(gates, pre):
    """Per block ReLU: (units whose GPU gate differs from [fp64 pre-activation > 0], the largest |fp64 pre-activation| among them)."""
    out = []
    for k in BLOCK:
        diff = gates[k - 1] != (pre[k] > 0)
        out.append((int(diff.sum()), float(pre[k][diff].abs().max()) if bool(diff.any()) else 0.0))
    return out
