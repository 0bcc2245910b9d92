"""flat_adam.FlatAdam.step on the MI355X against direct hip.adam_clip_step calls on a hand-packed bucket -- the same kernel on the same layout,
so bit for bit -- and a resume through optimizer.state_dict() / load_state_dict().  The six parameters of tests/test_flat_adam.py."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = ((1,), (2,), (3,), (4,), (5,), (2, 3))
OFFSETS, TOTAL = (0, 4, 8, 12, 16, 24), 32
LR, BETAS, EPS, CLIP, SCALE = 1e-2, (0.9, 0.999), 1e-8, 0.5, 0.25


def _values(seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=gen) for s in SHAPES]


def _pack(values):
    flat = torch.zeros(TOTAL)
    for off, t in zip(OFFSETS, values):
        flat[off:off + t.numel()] = t.reshape(-1)
    return flat.cuda()


def _fresh():
    named = [("p%d" % i, torch.nn.Parameter(t.cuda())) for i, t in enumerate(_values(0))]
    return named, torch.optim.Adam([p for _, p in named], lr=LR)


def _step(fa, k):
    for (_, gv, _, _), g in zip(fa.views, _values(100 + k)):       # seeded gradients, written the way autograd does: into the .grad views
        gv.copy_(g)
    fa.step(LR, BETAS, EPS, CLIP, grad_scale=SCALE)


def test_three_steps_equal_the_direct_kernel_calls_and_a_resume_equals_the_uninterrupted_run():
    from crowdnav_prediction_attngraph_amd import hip
    from crowdnav_prediction_attngraph_amd.flat_adam import FlatAdam
    pad = torch.ones(TOTAL, dtype=torch.bool)
    for off, s in zip(OFFSETS, SHAPES):
        pad[off:off + torch.Size(s).numel()] = False
    pad = pad.cuda()

    named, opt = _fresh()
    fa = FlatAdam(named, opt)
    p, m, v = _pack(_values(0)), torch.zeros(TOTAL, device="cuda"), torch.zeros(TOTAL, device="cuda")
    assert torch.equal(fa.p, p)
    after_two = None
    for k in range(3):
        _step(fa, k)
        hip.adam_clip_step(p, _pack(_values(100 + k)), m, v, k + 1, LR, BETAS, EPS, CLIP, grad_scale=SCALE)
        assert fa.step_no == k + 1
        for name, got, want in (("p", fa.p, p), ("m", fa.m, m), ("v", fa.v, v)):
            assert torch.equal(got, want), (name, k)
            assert bool((got[pad] == 0).all()), (name, k)
        for (_, q), (pv, _, _, _) in zip(named, fa.views):
            assert q.data_ptr() == pv.data_ptr()
        if k == 1:
            fa.sync_optimizer_state()
            after_two = ([q.detach().clone() for _, q in named], copy.deepcopy(opt.state_dict()))   # state_dict() hands out the views themselves
    assert bool(p.ne(_pack(_values(0))).any()) and fa.bound()

    # resume: the parameters and the optimiser state after two steps -> fresh tensors, a fresh optimiser, a new bucket -> the third step
    named2 = [("p%d" % i, torch.nn.Parameter(t.clone())) for i, t in enumerate(after_two[0])]
    opt2 = torch.optim.Adam([q for _, q in named2], lr=LR)
    opt2.load_state_dict(after_two[1])
    fb = FlatAdam(named2, opt2)
    assert fb.step_no == 2
    _step(fb, 2)
    assert fb.step_no == 3
    for name, got, want in (("p", fb.p, fa.p), ("m", fb.m, fa.m), ("v", fb.v, fa.v)):
        assert torch.equal(got, want), name
