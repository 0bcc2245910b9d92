"""Host side of cn_ppo_minibatch_step_variant (no device): the binding declares the three entry points and cn_ppo_variant with the header's
layout, the workspace query runs on the host (NULL and {1, 1, NULL} are the sized query, the no-attention variant is smaller), one function gives
the parameter-to-field map to the rollout handle and to the steppers, and hip.*MinibatchStepper.supported stays false on CPU tensors for every
variant.  The GPU side: tests/test_gpu_minibatch_variants.py."""
import ctypes as C
import os
import re

import pytest

torch = pytest.importorskip("torch")

from crowdnav_prediction_attngraph_amd import _abi as A  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cn_ppo_minibatch_workspace_bytes_variant", "cn_ppo_minibatch_step_variant", "cn_ppo_row_totals_visible")
VARIANTS = [(False, True), (True, False), (False, False)]                # (use_self_attn, sort_humans)


def test_the_binding_declares_the_three_symbols_and_the_variant_struct():
    L = A.lib()
    for s in SYMBOLS:
        assert s in A.ABI_SYMBOLS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert L.cn_ppo_minibatch_workspace_bytes_variant.restype is C.c_int64
    hdr = open(os.path.join(ROOT, "include", "crowdnav_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} cn_ppo_variant;", hdr)
    assert m, "include/crowdnav_hip.h has no cn_ppo_variant"
    fields = [f.split()[-1].lstrip("*") for f in m.group(1).split(";") if f.strip()]
    assert fields == [n for n, _ in A.PpoVariant._fields_] == ["self_attn", "sort_humans", "visible_masks"]
    assert [t for _, t in A.PpoVariant._fields_] == [C.c_int32, C.c_int32, C.c_void_p]
    assert C.sizeof(A.PpoVariant) == 16 and A.PpoVariant.visible_masks.offset == 8 and A.PpoVariant.sort_humans.offset == 4
    assert C.sizeof(A.PolicyWeights) == 8 * 45                           # the existing struct keeps its layout


@pytest.mark.parametrize("shape", [(30, 2048, 20, 2, 405000), (1, 1, 1, 2, 1), (5, 17, 48, 16, 5 * 17 * 48)])
def test_the_variant_query_on_the_host(shape):
    L = A.lib()
    q = L.cn_ppo_minibatch_workspace_bytes_variant
    for dims in (None, A.PolicyDims(192, 64, 48, 320)):
        d = None if dims is None else C.byref(dims)
        want = L.cn_ppo_minibatch_workspace_bytes_sized(*shape, d)
        assert want > 0
        assert q(*shape, d, None) == want
        assert q(*shape, d, C.byref(A.PpoVariant(1, 1, None))) == want
        assert q(*shape, d, C.byref(A.PpoVariant(1, 0, None))) == want   # the gather's variant reserves nothing of its own
        no_attn = q(*shape, d, C.byref(A.PpoVariant(0, 1, None)))
        assert 0 < no_attn < want and no_attn % 256 == 0
        assert q(*shape, d, C.byref(A.PpoVariant(0, 0, None))) == no_attn
    T, N, H, D, rows = shape
    top = int(L.cn_ppo_minibatch_max_rows())
    v = A.PpoVariant(0, 0, None)                                         # the unchanged limits, also for the narrower buffers
    assert q(T, N, 49, D, rows, None, C.byref(v)) == 0 and q(T, N, H, 17, rows, None, C.byref(v)) == 0
    assert q(30, 2048, 48, 2, top, None, C.byref(v)) > 0 and q(30, 2048, 48, 2, top + 1, None, C.byref(v)) == 0
    bad = A.PolicyDims(96, 64, 64, 256)
    assert q(*shape, C.byref(bad), C.byref(v)) == 0


def _policy_and_storage(**kw):
    from crowdnav_prediction_attngraph_amd.policy import Policy, make_spaces
    from crowdnav_prediction_attngraph_amd.trainer import new_rollouts
    T, E, H, D = 2, 3, 5, 2
    ob_space, act_space = make_spaces(H, D)
    pol = Policy(ob_space.spaces, act_space, base="selfAttn_merge_srnn",
                 base_kwargs=dict(env_name="CrowdSimVarNum-v0", num_processes=E, num_mini_batch=1, seq_length=T, **kw))
    return pol, new_rollouts(pol, T, E, ob_space.spaces, act_space)


def test_one_function_gives_the_parameter_to_field_map():
    from crowdnav_prediction_attngraph_amd import hip
    from crowdnav_prediction_attngraph_amd.hip_policy import HipPolicy
    assert A.policy_weight_keys() is A.POLICY_WEIGHT_KEYS and A.policy_weight_keys(True) is A.POLICY_WEIGHT_KEYS
    off = A.policy_weight_keys(False)
    assert not any(k.startswith("base.spatial_attn.") for _, k in off)
    d = dict(off)
    assert d["emb0_w"] == "base.spatial_linear.0.weight" and d["emb0_b"] == "base.spatial_linear.0.bias"
    assert d["spatial_linear_w"] == "base.spatial_linear.2.weight" and d["spatial_linear_b"] == "base.spatial_linear.2.bias"
    fields = [f for f, _ in A.POLICY_WEIGHT_KEYS]
    dropped = fields[fields.index("emb2_w"):fields.index("out_proj_b") + 1]
    assert [f for f, _ in off] == [f for f in fields if f not in dropped] and len(dropped) == 12
    assert {f: k for f, k in off if f not in ("emb0_w", "emb0_b", "spatial_linear_w", "spatial_linear_b")}.items() <= dict(A.POLICY_WEIGHT_KEYS).items()
    # the rollout handle and the steppers read it from there
    h = HipPolicy.__new__(HipPolicy)
    assert h._weight_keys() is A.POLICY_WEIGHT_KEYS
    h._self_attn = False
    assert h._weight_keys() == off
    for attn in (True, False):
        pol, _ = _policy_and_storage(use_self_attn=attn)
        st = hip.MinibatchStepper(pol)
        assert st.weight_keys == A.policy_weight_keys(attn)
        names = dict(pol.named_parameters())
        assert all(k in names for _, k in st.weight_keys)
        assert st.uncovered == ["base.human_node_final_linear.weight", "base.human_node_final_linear.bias"]


@pytest.mark.parametrize("use_self_attn,sort_humans", VARIANTS + [(True, True)])
def test_supported_stays_false_on_cpu_tensors(use_self_attn, sort_humans):
    from crowdnav_prediction_attngraph_amd import hip
    pol, ro = _policy_and_storage(use_self_attn=use_self_attn, sort_humans=sort_humans)
    assert pol.base.use_self_attn == use_self_attn and pol.base.sort_humans == sort_humans and not ro.rewards.is_cuda
    assert ro.obs["visible_masks"].dtype == torch.bool
    assert not hip.MinibatchStepper.supported(pol, ro) and not hip.SizedMinibatchStepper.supported(pol, ro)
