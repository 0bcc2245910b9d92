"""PPO -- mirror of rl/ppo/ppo.py:6-101 (same constructor, `update(rollouts) -> (value_loss, action_loss, entropy)`).

Data-parallel extension (new, the reference is single process): when torch.distributed is initialised with world > 1
every rank owns a disjoint shard of envs and
  * the advantage statistics (sum, sum of squares, count) are all-reduced once per update() so mean / unbiased std are
    global (ppo.py:38-39 semantics over all T x E_total samples);
  * per optimiser step ONE all-reduce of a single flat fp32 gradient bucket (all parameters, ~10 MB) over RCCL/xGMI,
    averaged, then the grad-norm clip and Adam run identically on every rank.
The bucket and its optimiser step are flat_adam.FlatAdam, shared with gst_hip.HipGstTrainer.  update() is one epoch / minibatch loop: a
gradient producer (cn_ppo_minibatch_step / cn_ppo_minibatch_step_sized, or the autograd-joined graph), then _optimizer_step.
"""
import functools

import torch
import torch.nn as nn
import torch.optim as optim

from . import hip
from .flat_adam import FlatAdam


def _dist():
    """torch.distributed when this process is one of several ranks.  CN_FORCE_DIST=1 (test aid) also takes the collective branch with a
    single rank: tests/test_gpu_dist.py runs the RCCL all-reduces of update() that way on a box with one GPU."""
    import os
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or os.environ.get("CN_FORCE_DIST") == "1"):
        return dist
    return None


class PPO():
    def __init__(self, actor_critic, clip_param, ppo_epoch, num_mini_batch, value_loss_coef, entropy_coef, lr=None, eps=None,
                 max_grad_norm=None, use_clipped_value_loss=True):
        self.actor_critic = actor_critic
        self.clip_param = clip_param
        self.ppo_epoch = ppo_epoch
        self.num_mini_batch = num_mini_batch
        self.value_loss_coef = value_loss_coef
        self.entropy_coef = entropy_coef
        self.max_grad_norm = max_grad_norm
        self.use_clipped_value_loss = use_clipped_value_loss
        self.optimizer = optim.Adam(actor_critic.parameters(), lr=lr, eps=eps)
        self._flat = None          # flat_adam.FlatAdam, once update() has seen GPU tensors

    # ---- flat buckets (GPU path): flat_adam.FlatAdam --------------------------------------------------------------------
    # `self.optimizer` stays the owner of the optimiser state: its state_dict() / load_state_dict() / param_groups (learning-rate schedule of
    # train.py:148-152) keep working.
    def _bind_flat(self):
        """The bucket, bound now, or bound again (adopting restored moments and step count) because a pointer moved: optimizer.load_state_dict()."""
        named = [(n, p) for n, p in self.actor_critic.named_parameters() if p.requires_grad]
        if self._flat is None or not self._flat.bound([p for _, p in named]):
            self._flat = FlatAdam(named, self.optimizer)
            self._weights_changed()
        return self._flat

    def _weights_changed(self):
        # the rollout-side weight snapshot (cn_policy_set_weights) must be refreshed: raw-pointer writes bump no version
        getattr(self.actor_critic, "weights_changed", lambda: None)()

    def sync_optimizer_state(self):
        """Before optimizer.state_dict() is read (trainer.save_checkpoint): its `step` tensors follow the bucket's step count."""
        if self._flat is not None:
            self._flat.sync_optimizer_state()

    def _advantages(self, rollouts):
        ret, val = rollouts.returns, rollouts.value_preds
        T, N = rollouts.rewards.shape[0], rollouts.rewards.shape[1]
        d = _dist()
        if ret.is_cuda:
            stats = hip.adv_stats(ret, val, T * N)          # HIP kernel (first T rows are contiguous)
            if d is not None:
                d.all_reduce(stats)
            adv = torch.empty(T, N, 1, device=ret.device)
            hip.adv_normalize(ret, val, stats, T * N, adv)
            return adv
        # CPU tensors (unit tests / --no-cuda plumbing): ppo.py:37-39 in torch ops
        adv = ret[:-1] - val[:-1]
        if d is not None:
            a64 = adv.double()
            stats = torch.stack([a64.sum(), (a64 * a64).sum(), torch.tensor(float(adv.numel()), dtype=torch.float64)])
            d.all_reduce(stats)
            mean = stats[0] / stats[2]
            std = ((stats[1] - stats[2] * mean * mean) / (stats[2] - 1)).clamp(min=0).sqrt()
            return (adv - mean.float()) / (std.float() + 1e-5)
        return (adv - adv.mean()) / (adv.std() + 1e-5)

    def _losses(self, values, action_log_probs, old_logp, adv_targ, value_preds, returns):
        """(value_loss, action_loss) of ppo.py:66-84.  GPU tensors: one fused HIP kernel each way (cn_ppo_loss_fwd/bwd)."""
        if values.is_cuda:
            losses = hip.PPOLoss.apply(values, action_log_probs, old_logp, adv_targ, value_preds, returns, self.clip_param,
                                       self.use_clipped_value_loss)
            return losses[0], losses[1]
        ratio = torch.exp(action_log_probs - old_logp)
        surr1 = ratio * adv_targ
        surr2 = torch.clamp(ratio, 1.0 - self.clip_param, 1.0 + self.clip_param) * adv_targ
        action_loss = -torch.min(surr1, surr2).mean()
        if self.use_clipped_value_loss:
            value_pred_clipped = value_preds + (values - value_preds).clamp(-self.clip_param, self.clip_param)
            value_losses = (values - returns).pow(2)
            value_losses_clipped = (value_pred_clipped - returns).pow(2)
            value_loss = 0.5 * torch.max(value_losses, value_losses_clipped).mean()
        else:
            value_loss = 0.5 * (returns - values).pow(2).mean()
        return value_loss, action_loss

    # ---- one boundary call per minibatch (attention-graph network on the GPU) -----------------------------------------
    # cn_ppo_minibatch_step gathers the minibatch from the storage by env index, runs the train-mode forward, the losses and the whole
    # backward, and WRITES every parameter gradient into the flat bucket: no autograd graph, no framework kernel between the rollout
    # storage and the Adam step.  The default network sizes run it through hip.MinibatchStepper, every other (R, M, A, O) of the device box
    # through hip.SizedMinibatchStepper (cn_ppo_minibatch_step_sized); with use_self_attn or sort_humans off both pass the switches as
    # cn_ppo_variant (cn_ppo_minibatch_step_variant).  use_minibatch_step = False keeps the autograd-joined path below for every network;
    # what lies outside the step (fp32 arithmetic, crowds of 49 to 64 humans, edge widths above 16, the DS-RNN baseline, CPU tensors)
    # always takes it.
    use_minibatch_step = True

    def _stepper_class(self, rollouts):
        """hip.MinibatchStepper (default sizes), hip.SizedMinibatchStepper (any other tuple of the device box), or None: no one-call step."""
        if not (self.actor_critic.is_recurrent and hasattr(self.actor_critic, "base")):
            return None
        for cls in (hip.MinibatchStepper, hip.SizedMinibatchStepper):
            if cls.supported(self.actor_critic, rollouts):
                return cls
        return None

    def _fast_path(self, rollouts):
        return bool(self.use_minibatch_step) and self._stepper_class(rollouts) is not None

    def _fast_plan(self, rollouts):
        """(stepper, per-env row totals) when every minibatch this update() can draw fits one cn_ppo_minibatch_step, else None: the update then
        takes the autograd-joined path.  Decided on the host from the one readback update() makes anyway, before the first permutation is
        drawn and before any launch of the step: the npb envs with the most rows together bound every minibatch of every epoch."""
        cls = self._stepper_class(rollouts)
        if type(getattr(self, "_stepper", None)) is not cls or self._stepper.policy is not self.actor_critic:
            self._stepper = cls(self.actor_critic)
        E = rollouts.rewards.shape[1]
        assert E >= self.num_mini_batch, "PPO requires the number of processes ({}) to be greater than or equal to the number of PPO mini batches ({}).".format(E, self.num_mini_batch)
        totals = self._stepper.row_totals(rollouts)              # the ONE readback of update(): rows per env -> rows per minibatch on the host
        cap = self._stepper.max_rows()
        if int(totals.sum()) > cap and int(torch.sort(totals, descending=True).values[:E // self.num_mini_batch].sum()) > cap:
            return None
        return self._stepper, totals

    # ---- gradient producers -> (minibatches, produce) ---------------------------------------------------------------------
    # minibatches() yields one epoch's minibatches after drawing its ONE torch.randperm(E) (storage.py:193); produce(minibatch, losses_out) leaves
    # the minibatch's gradients in the bucket (CPU tensors: in the .grads) and its (value_loss, action_loss, entropy) in losses_out [3] on the device.
    def _minibatch_step_producer(self, rollouts, advantages, flat, stepper, totals):
        flat.claim_grads(copy_in=False)                         # the bucket views must still be the gradients (checked once per update())
        # The slices the step never writes still enter the all-reduce, the clip norm and Adam: exact zeros once per update(), like the
        # bucket-wide zero_() of the autograd producer, whatever was left there before.
        for a, b in flat.spans(stepper.uncovered):
            flat.g[a:b].zero_()
        E, dev, npb = rollouts.rewards.shape[1], rollouts.rewards.device, rollouts.rewards.shape[1] // self.num_mini_batch
        hyper = (self.clip_param, self.value_loss_coef, self.entropy_coef, self.use_clipped_value_loss)

        def minibatches():
            perm = torch.randperm(E)
            for start in range(0, E, npb):
                if start + npb > E:                              # storage.py:209-210 raises here, after the complete groups (see storage.py)
                    raise IndexError("index {} is out of bounds for dimension 0 with size {}".format(E, E))
                yield perm[start:start + npb]

        def produce(idx, losses_out):
            stepper.step(rollouts, advantages, idx.to(device=dev, dtype=torch.int32), int(totals[idx].sum()), hyper, losses_out)
        return minibatches, produce

    def _autograd_producer(self, rollouts, advantages, flat):
        """flat None: CPU tensors, the gradients stay in the .grads for optimizer.step()."""
        if not self.actor_critic.is_recurrent:
            raise NotImplementedError("feed-forward policies are out of scope")
        unclaimed = flat is not None

        def produce(sample, losses_out):
            nonlocal unclaimed
            obs_batch, hxs_batch, actions_batch, value_preds_batch, return_batch, masks_batch, old_logp_batch, adv_targ = sample
            values, action_log_probs, dist_entropy, _ = self.actor_critic.evaluate_actions(obs_batch, hxs_batch, masks_batch, actions_batch)
            value_loss, action_loss = self._losses(values, action_log_probs, old_logp_batch, adv_targ, value_preds_batch, return_batch)
            total_loss = value_loss * self.value_loss_coef + action_loss - dist_entropy * self.entropy_coef
            (self.optimizer.zero_grad if flat is None else flat.g.zero_)()    # the bucket-wide zero_() is optimizer.zero_grad() with the views kept bound
            total_loss.backward()
            if unclaimed:                                        # autograd accumulates into the bound views; checked once per update()
                flat.claim_grads(copy_in=True)
                unclaimed = False
            torch.stack((value_loss.detach(), action_loss.detach(), dist_entropy.detach()), out=losses_out)
        return (lambda: rollouts.recurrent_generator(advantages, self.num_mini_batch)), produce

    def _optimizer_step(self, flat, d, ar_events):
        """Gradient average over the ranks (ONE collective), grad-norm clip and Adam: on the bucket, or (flat None: CPU tensors) in torch ops."""
        if flat is None:
            if d is not None:                                    # gloo tests: pack, one all-reduce, unpack
                ps = [p for p in self.actor_critic.parameters() if p.requires_grad and p.grad is not None]
                bucket = torch.cat([p.grad.reshape(-1) for p in ps])
                d.all_reduce(bucket)
                bucket /= d.get_world_size()
                for p, b in zip(ps, bucket.split([p.numel() for p in ps])):
                    p.grad.copy_(b.view_as(p))
            nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)
            self.optimizer.step()
            return
        scale = 1.0
        if d is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
            d.all_reduce(flat.g)                                 # RCCL over xGMI
            ev[1].record()
            ar_events.append(ev)
            scale = 1.0 / d.get_world_size()
        g = self.optimizer.param_groups[0]
        flat.step(g["lr"], g["betas"], g["eps"], self.max_grad_norm, grad_scale=scale)
        # after every step, not once per update(): it only clears a flag, and the DS-RNN baseline's evaluate_actions reads the snapshot (the
        # edge-GRU sequence kernels take the cn_srnn handle's weights)
        self._weights_changed()

    def update(self, rollouts):
        advantages = self._advantages(rollouts)
        E, dev, d = rollouts.rewards.shape[1], rollouts.rewards.device, _dist()
        flat = self._bind_flat() if dev.type == "cuda" else None
        self.last_allreduce_ms = None
        plan = self._fast_plan(rollouts) if flat is not None and self._fast_path(rollouts) else None
        minibatches, produce = self._autograd_producer(rollouts, advantages, flat) if plan is None else self._minibatch_step_producer(rollouts, advantages, flat, *plan)
        losses = torch.zeros(self.ppo_epoch * len(range(0, E, max(E // self.num_mini_batch, 1))), 3, device=dev)   # one row per optimiser step
        ar_events, k = [], 0
        for e in range(self.ppo_epoch):
            for minibatch in minibatches():
                produce(minibatch, losses[k])
                self._optimizer_step(flat, d, ar_events)
                k += 1
        if flat is not None:
            flat.sync_optimizer_state()
        if ar_events:      # mean duration of the gradient all-reduce on this rank's stream
            torch.cuda.synchronize()
            self.last_allreduce_ms = sum(a.elapsed_time(b) for a, b in ar_events) / len(ar_events)
        # the autograd producer's rows are added one after the other, the order its sum always had: the reported means keep their last bit
        sums = losses[:k].sum(0) if plan is not None else functools.reduce(torch.add, losses[:k], torch.zeros(3, device=dev))
        if d is not None:
            d.all_reduce(sums)
            sums /= d.get_world_size()
        return tuple((sums / (self.ppo_epoch * self.num_mini_batch)).tolist())   # (value_loss, action_loss, entropy): single host sync per update()
