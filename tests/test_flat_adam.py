"""flat_adam.FlatAdam on CPU tensors (binding needs neither the GPU nor the library): the bucket layout, the aliasing of p.data / p.grad /
optimiser state, adoption of restored optimiser state, bound() and re-binding, spans(), sync_optimizer_state().  Parameters of 1, 2, 3, 4, 5
and 2 x 3 elements put every rounding case of the 4-float alignment into play."""
import torch

from crowdnav_prediction_attngraph_amd.flat_adam import FlatAdam

SHAPES = ((1,), (2,), (3,), (4,), (5,), (2, 3))
OFFSETS, TOTAL = (0, 4, 8, 12, 16, 24), 32


def _named(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [("p%d" % i, torch.nn.Parameter(torch.randn(*s, generator=gen))) for i, s in enumerate(SHAPES)]


def _pad_mask():
    pad = torch.ones(TOTAL, dtype=torch.bool)
    for off, s in zip(OFFSETS, SHAPES):
        pad[off:off + torch.Size(s).numel()] = False
    return pad


def _two_adam_steps(named):
    opt = torch.optim.Adam([p for _, p in named], lr=1e-2)
    gen = torch.Generator().manual_seed(7)
    for _ in range(2):
        for _, p in named:
            p.grad = torch.randn(p.shape, generator=gen)
        opt.step()
    return opt


def test_layout_padding_and_aliasing():
    named = _named()
    want = [p.detach().clone() for _, p in named]
    opt = torch.optim.Adam([p for _, p in named], lr=1e-2)
    fa = FlatAdam(named, opt)
    assert [fa.offsets[n][0] for n, _ in named] == list(OFFSETS) and fa.offsets["p5"][1] == TOTAL
    assert all(b.shape == (TOTAL,) and b.dtype == torch.float32 for b in (fa.p, fa.g, fa.m, fa.v)) and fa.step_no == 0
    for (name, p), w, off, (pv, gv, mv, vv) in zip(named, want, OFFSETS, fa.views):
        k = p.numel()
        assert torch.equal(p.detach(), w) and torch.equal(fa.p[off:off + k].view_as(p), w), name
        assert p.data_ptr() == pv.data_ptr() == fa.p[off:].data_ptr() and p.grad.data_ptr() == gv.data_ptr() == fa.g[off:].data_ptr(), name
        # write through the tensor, read through the bucket -- and the other way round
        p.data.fill_(1.5); p.grad.fill_(2.5); opt.state[p]["exp_avg"].fill_(3.5); opt.state[p]["exp_avg_sq"].fill_(4.5)
        for b, val in ((fa.p, 1.5), (fa.g, 2.5), (fa.m, 3.5), (fa.v, 4.5)):
            assert bool((b[off:off + k] == val).all()), name
        for b in (fa.p, fa.g, fa.m, fa.v):
            b[off:off + k] = -1.0
        for t in (p.data, p.grad, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]):
            assert bool((t == -1.0).all()) and t.shape == p.shape, name
    pad = _pad_mask()
    assert int(pad.sum()) == TOTAL - 21
    for b in (fa.p, fa.g, fa.m, fa.v):
        assert bool((b[pad] == 0).all())
    assert fa.bound() and fa.bound([p for _, p in named])
    assert all(fa[k] is getattr(fa, k) for k in ("p", "g", "m", "v", "views"))       # the buckets by name, as when they were a dict


def test_state_restored_by_load_state_dict_is_adopted():
    named = _named()
    opt = _two_adam_steps(named)
    sd = opt.state_dict()
    fresh = [(n, torch.nn.Parameter(p.detach().clone())) for n, p in named]
    opt2 = torch.optim.Adam([p for _, p in fresh], lr=1e-2)
    opt2.load_state_dict(sd)
    fa = FlatAdam(fresh, opt2)
    assert fa.step_no == 2
    for (name, p), (_, q), (pv, gv, mv, vv) in zip(named, fresh, fa.views):
        assert torch.equal(mv, opt.state[p]["exp_avg"]) and torch.equal(vv, opt.state[p]["exp_avg_sq"]), name
        assert opt2.state[q]["exp_avg"].data_ptr() == mv.data_ptr() and opt2.state[q]["exp_avg_sq"].data_ptr() == vv.data_ptr(), name
        assert float(opt2.state[q]["step"]) == 2.0, name
    pad = _pad_mask()
    assert bool((fa.m[pad] == 0).all()) and bool((fa.v[pad] == 0).all())
    # the optimiser's own interface keeps working on the views
    back = opt2.state_dict()
    assert len(back["state"]) == len(SHAPES) and all(float(s["step"]) == 2.0 for s in back["state"].values())
    assert opt2.param_groups[0]["lr"] == 1e-2


def test_bound_turns_false_when_a_pointer_moves_and_a_rebind_keeps_the_values():
    def unbind_data(named, opt):
        named[2][1].data = named[2][1].data.clone()

    def unbind_grad(named, opt):
        named[3][1].grad = None

    def unbind_state(named, opt):
        opt.state.clear()

    for unbind in (unbind_data, unbind_grad, unbind_state):
        named = _named()
        opt = _two_adam_steps(named)
        fa = FlatAdam(named, opt)
        assert fa.bound() and fa.step_no == 2
        p_want, m_want, v_want = fa.p.clone(), fa.m.clone(), fa.v.clone()
        unbind(named, opt)
        assert not fa.bound(), unbind.__name__
        fb = FlatAdam(named, opt)
        assert fb.bound() and not fa.bound(), unbind.__name__
        assert torch.equal(fb.p, p_want), unbind.__name__
        if unbind is unbind_state:                 # nothing left to adopt: a fresh optimiser state
            assert fb.step_no == 0 and not fb.m.any() and not fb.v.any()
        else:
            assert fb.step_no == 2 and torch.equal(fb.m, m_want) and torch.equal(fb.v, v_want), unbind.__name__
    params = [p for _, p in named]
    assert fb.bound(params) and not fb.bound(params[:-1])       # another parameter count is not this bucket either


def test_claim_grads_points_a_replaced_grad_at_its_view_again():
    named = _named()
    fa = FlatAdam(named)
    p, (_, gv, _, _) = named[4][1], fa.views[4]
    for copy_in, want in ((True, 3.0), (False, 0.0)):
        fa.g.zero_()
        p.grad = torch.full(p.shape, 3.0)
        fa.claim_grads(copy_in)
        assert p.grad is gv and bool((fa.g[16:21] == want).all()) and fa.bound()
    p.grad = None
    fa.claim_grads(False)
    assert p.grad is gv


def test_spans_merges_adjacent_names_and_keeps_separated_ones_apart():
    fa = FlatAdam(_named())
    assert fa.spans(["p1", "p2"]) == [[4, 12]]
    assert fa.spans(["p2", "p1"]) == [[4, 12]]
    assert fa.spans(["p0", "p2", "p3", "p5"]) == [[0, 4], [8, 16], [24, 32]]
    assert fa.spans([n for n, _ in _named()]) == [[0, TOTAL]] and fa.spans([]) == []


def test_sync_optimizer_state_fills_the_step_tensors_in_place():
    named = _named()
    opt = torch.optim.Adam([p for _, p in named], lr=1e-2)
    fa = FlatAdam(named, opt)
    steps = [opt.state[p]["step"] for _, p in named]
    fa.step_no = 5
    fa.sync_optimizer_state()
    for (_, p), s in zip(named, steps):
        assert opt.state[p]["step"] is s and float(s) == 5.0
    assert FlatAdam(_named()).optimizer is None                 # without an optimiser the moments live in the buckets alone
