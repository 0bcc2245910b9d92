"""FlatAdam -- the flat-bucket optimiser of both training paths (ppo.PPO.update, gst_hip.HipGstTrainer) and the only place that knows the
bucket layout.  ONE fp32 buffer each for the parameters, their gradients and the two Adam moments; every p.data / p.grad /
optimizer.state[p]['exp_avg'|'exp_avg_sq'] is a view into them, so a gradient all-reduce needs no packing and grad-norm clip + Adam is one
boundary call (cn_adam_clip_step).  Binding is plain tensor work on the parameters' device; only step() reaches the library."""
import torch


class FlatAdam:
    def __init__(self, named_params, optimizer=None):
        """named_params: ordered (name, parameter) pairs.  A torch optimiser handed in stays the owner of the optimiser state (state_dict() /
        load_state_dict() / param_groups keep working): the moments and the step count it holds -- restored by load_state_dict(), or left by
        its own steps -- are adopted, and its state becomes the views plus a `step` tensor."""
        named_params = list(named_params)
        self.params, self.optimizer = [p for _, p in named_params], optimizer
        # every parameter starts on a 16-byte boundary of the bucket: its .data pointer is handed to kernels that load rows as float4
        # (cn_split_bf16, cn_embed0_*, cn_gru_seq_*, bias vectors ...); the 1- and 2-element tensors (critic_linear.bias, fc_mean.bias,
        # logstd) would otherwise leave everything behind them 4-byte aligned.  The padding stays zero in all four buckets: no
        # gradient, no moment, no update, nothing added to the gradient norm.
        n = sum((p.numel() + 3) // 4 * 4 for p in self.params)
        self.p, self.g, self.m, self.v = (torch.zeros(n, dtype=torch.float32, device=self.params[0].device) for _ in range(4))
        self.offsets, self.views, self.step_no, off = {}, [], 0, 0
        for name, p in named_params:
            pv, gv, mv, vv = (b[off:off + p.numel()].view_as(p) for b in (self.p, self.g, self.m, self.v))
            pv.copy_(p.data)
            s = optimizer.state.get(p) if optimizer is not None else None
            if s:
                mv.copy_(s["exp_avg"]); vv.copy_(s["exp_avg_sq"])
                self.step_no = max(self.step_no, int(float(s["step"])))
            p.data, p.grad = pv, gv
            if optimizer is not None:
                optimizer.state[p] = {"step": torch.tensor(0.0), "exp_avg": mv, "exp_avg_sq": vv}
            self.views.append((pv, gv, mv, vv))
            self.offsets[name] = (off, off + (p.numel() + 3) // 4 * 4)
            off = self.offsets[name][1]
        self.sync_optimizer_state()
        self._ws = None                            # cn_adam_workspace_doubles() doubles, allocated by the first step()

    def __getitem__(self, key):
        return getattr(self, key)                  # flat["p" | "g" | "m" | "v" | "views"], the names the buckets had as a dict

    def bound(self, params=None):
        """Whether the parameters (`params`: the model's current list), their gradients and their optimiser state still are the views."""
        params = self.params if params is None else params
        if self.p.device != params[0].device or len(params) != len(self.views):
            return False
        for p, (pv, gv, mv, vv) in zip(params, self.views):
            if p.data_ptr() != pv.data_ptr() or p.grad is None or p.grad.data_ptr() != gv.data_ptr():
                return False
            if self.optimizer is not None:
                s = self.optimizer.state.get(p)
                if not s or s["exp_avg"].data_ptr() != mv.data_ptr() or s["exp_avg_sq"].data_ptr() != vv.data_ptr():
                    return False
        return True

    def claim_grads(self, copy_in):
        """Once per update (O(parameters) of Python): a .grad that was replaced, not accumulated into, is its view again -- with copy_in, its value too."""
        for p, (_, gv, _, _) in zip(self.params, self.views):
            if p.grad is not gv and (p.grad is None or p.grad.data_ptr() != gv.data_ptr()):
                if copy_in and p.grad is not None:
                    gv.copy_(p.grad)
                p.grad = gv

    def spans(self, names):
        """Merged [start, end) ranges of the buckets that belong to the named parameters (adjacent ones become one range)."""
        spans = []
        for a, b in sorted(self.offsets[name] for name in names):
            if spans and spans[-1][1] == a:
                spans[-1][1] = b
            else:
                spans.append([a, b])
        return spans

    def step(self, lr, betas, eps, max_grad_norm, grad_scale=1.0):
        """clip_grad_norm_(parameters, max_grad_norm) of grad_scale * .g, then Adam.step(), over the whole bucket in place."""
        from . import hip
        if self._ws is None:
            self._ws = torch.empty(hip.A.lib().cn_adam_workspace_doubles(), dtype=torch.float64, device=self.p.device)
        self.step_no += 1
        hip.adam_clip_step(self.p, self.g, self.m, self.v, self.step_no, lr, betas, eps, max_grad_norm, grad_scale=grad_scale, workspace=self._ws)

    def sync_optimizer_state(self):
        """The optimiser's `step` tensors follow step_no, filled in place (before its state_dict() is read)."""
        if self.optimizer is not None:
            for s in filter(None, map(self.optimizer.state.get, self.params)):
                s["step"].fill_(float(self.step_no))
