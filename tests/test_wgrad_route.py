"""hip_train.wgrad on a shape the split-K kernel has no plan for (cn_linear_wgrad_splits == 0; host-only, no GPU needed): the torch route gives
the gated product where the caller allows it, and the callers that have checked their shapes beforehand (WgradLinear, HipLinear, the layers of
HHBlockFused pass required=True) get an error, not another route."""
import pytest

torch = pytest.importorskip("torch")

from crowdnav_prediction_attngraph_amd import _abi as A  # noqa: E402
from crowdnav_prediction_attngraph_amd import hip_train as H  # noqa: E402


def test_wgrad_without_a_plan_is_torch_or_an_error():
    g = torch.Generator().manual_seed(0)
    dy, x, gate = torch.randn(5, 10, generator=g), torch.randn(5, 7, generator=g), torch.randn(5, 10, generator=g)
    assert A.lib().cn_linear_wgrad_splits(5, 10, 7) == 0
    dw, db = H.wgrad(dy, x)
    assert torch.equal(dw, dy.t() @ x) and torch.equal(db, dy.sum(0))
    dw, db = H.wgrad(dy, x, gate)
    masked = dy * (gate > 0)
    assert torch.equal(dw, masked.t() @ x) and torch.equal(db, masked.sum(0))
    with pytest.raises(A.CnError, match="no split-K plan"):
        H.wgrad(dy, x, gate, required=True)
