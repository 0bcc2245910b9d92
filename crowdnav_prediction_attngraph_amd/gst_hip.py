"""The GST predictor's boundary calls: thin object wrappers over the C ABI of csrc/gst.hip (HipGST: cn_gst_predict and the
VecPretextNormalize processing, cn_gst_wrapper_*), csrc/gst_train.hip (HipGstTrainer: cn_gst_train_step + the flat Adam bucket) and
csrc/gst_eval.hip (HipGstEvaluator: cn_gst_eval_step), and the three things they share: the cn_gst_weights struct over a list of tensors, a
batch of sequences brought to the call's device and layout, the grow-only workspace."""
import ctypes as C

import torch

from . import _abi as A
from .flat_adam import FlatAdam
from .hip_policy import HipHandle


def gst_weights(tensors, who):
    """The cn_gst_weights struct over `tensors` (in _abi.GST_WEIGHT_KEYS order), read by the kernels where they are: nothing is copied."""
    tensors = list(tensors)
    if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in tensors):
        raise A.CnError("%s: the predictor must live on the GPU in float32 (there is no CPU fallback of the HIP path)" % who)
    w = A.GstWeights()
    for (field, _), t in zip(A.GST_WEIGHT_KEYS, tensors):
        setattr(w, field, t.data_ptr())
    return w


def predictor_params(model):
    """The predictor's parameters in _abi.GST_WEIGHT_KEYS order."""
    named = dict(model.named_parameters())
    return [(k, named[k]) for _, k in A.GST_WEIGHT_KEYS]


def gst_batch(who, dev, v_obs, v_pred, loss_mask_rel, noise=None, max_samples=64):
    """v_obs [B,5,N,2], v_pred [B,P,N,2], loss_mask_rel [B,N,5+P], noise None or [B,S,P,N,2] (any device), P = the prediction horizon in 1 .. 8
    -> N, P and the four as contiguous float32 on `dev`, padded along the pedestrian axis to max(N, 4) with absent pedestrians (zeros)."""
    B, T, N, _ = v_obs.shape
    P = int(v_pred.shape[1])
    if T != A.GST_OBS_LEN or not 1 <= P <= A.CN_MAX_PRED or N > A.CN_MAX_HUMANS:
        raise A.CnError("%s: %s and at most %d pedestrians per sequence (got %d + %d steps, %d pedestrians)" % (who, A.HORIZON_BOX, A.CN_MAX_HUMANS, T, P, N))
    if tuple(v_pred.shape) != (B, P, N, 2) or tuple(loss_mask_rel.shape) != (B, N, T + P):
        raise A.CnError("%s: v_pred must be [B,P,N,2] and loss_mask_rel [B,N,5+P] (got %s and %s for B=%d, N=%d, P=%d)"
                        % (who, tuple(v_pred.shape), tuple(loss_mask_rel.shape), B, N, P))
    if noise is not None and (not 1 <= noise.shape[1] <= max_samples or tuple(noise.shape) != (B, noise.shape[1], P, N, 2)):
        raise A.CnError("%s: noise must be [B,S,P,N,2] with 1 <= S <= %d (got %s for B=%d, N=%d, P=%d)" % (who, max_samples, tuple(noise.shape), B, N, P))
    out = []
    for t in (v_obs, v_pred, loss_mask_rel, noise):
        if t is not None:
            if N < 4:
                t = torch.nn.functional.pad(t, (0, 0, 0, 4 - N))
            t = t.to(dev, torch.float32, non_blocking=True).contiguous()
        out.append(t)
    return [N, P] + out


def workspace(ws, need, dev):
    """The grow-only scratch buffer of a boundary call: `ws` if it holds `need` bytes, a larger one otherwise."""
    return ws if ws is not None and ws.numel() >= need else torch.empty(need, dtype=torch.uint8, device=dev)


class HipGST(HipHandle):
    """cn_gst handle: GST predictor (cn_gst_predict) and the VecPretextNormalize processing (cn_gst_wrapper_*).  pred_steps: the prediction
    horizon P = pred_seq_len of the predictor = sim.predict_steps of the env, 1 .. 8 (A.gst_horizon); 5 observed frames always."""
    _sym, _weights = "cn_gst", (A.GstWeights, A.GST_WEIGHT_KEYS)

    def __init__(self, human_num, max_envs, device=None, pred_steps=5):
        self.P = A.gst_horizon(pred_steps)                    # raises outside the box before anything is allocated
        self.H, self.maxE = int(human_num), int(max_envs)
        self._open(device, self.H, self.maxE, self.P, create="cn_gst_create_horizon")    # (cn_gst_create is this call with P = 5)

    def _weights_struct(self, fields, tensors):
        return gst_weights(tensors, "HipGST")

    def predict(self, in_traj, in_mask):
        """in_traj [E,H,5,2], in_mask [E,H,5] or [E,H,5,1] float -> (out_traj [E,H,P,5], out_mask [E,H,1])."""
        E = in_traj.shape[0]
        if tuple(in_traj.shape[1:]) != (self.H, 5, 2) or in_mask.numel() != E * self.H * 5:
            raise A.CnError("HipGST.predict: in_traj must be [E,%d,5,2] and in_mask [E,%d,5] (got %s and %s): %s"
                            % (self.H, self.H, tuple(in_traj.shape), tuple(in_mask.shape), A.HORIZON_BOX))
        out = torch.empty(E, self.H, self.P, 5, device=self.device)
        om = torch.empty(E, self.H, device=self.device)
        A.call("cn_gst_predict", self._h, E, A.ptr(in_traj.float().contiguous()), A.ptr(in_mask.float().reshape(E, self.H, 5).contiguous()),
               A.ptr(out), A.ptr(om), A.stream_ptr(), device=self.device)
        return out, om.unsqueeze(-1)

    def wrapper_reset(self, E):
        A.call("cn_gst_wrapper_reset", self._h, int(E), A.stream_ptr(), device=self.device)
        self._wrap_E = int(E)

    def wrapper_set_interval(self, pred_interval):
        """int(data.pred_timestep // env.time_step): the history keeps 4 * pred_interval + 1 observations, every pred_interval-th is fed."""
        A.call("cn_gst_wrapper_set_interval", self._h, int(pred_interval))

    def wrapper_state(self):
        """(traj [len,E,H,2] float32, mask [len,E,H] uint8) = the observation history in time order, oldest first (cn_gst_wrapper_save)."""
        L, E = int(A.lib().cn_gst_wrapper_history_len(self._h)), self._wrap_E
        traj = torch.empty(L, E, self.H, 2, device=self.device)
        mask = torch.empty(L, E, self.H, dtype=torch.uint8, device=self.device)
        A.call("cn_gst_wrapper_save", self._h, A.ptr(traj), A.ptr(mask), A.stream_ptr(), device=self.device)
        return traj, mask

    def wrapper_load_state(self, traj, mask):
        L = int(A.lib().cn_gst_wrapper_history_len(self._h))
        if traj.shape[0] != L or tuple(traj.shape[2:]) != (self.H, 2) or tuple(mask.shape) != tuple(traj.shape[:3]):
            raise A.CnError("history of shape %s / %s does not fit this wrapper (length %d, %d humans)" % (tuple(traj.shape), tuple(mask.shape), L, self.H))
        E = int(traj.shape[1])
        traj = traj.to(device=self.device, dtype=torch.float32).contiguous()
        mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
        A.call("cn_gst_wrapper_load", self._h, E, A.ptr(traj), A.ptr(mask), A.stream_ptr(), device=self.device)
        torch.cuda.current_stream(self.device).synchronize()   # the sources are temporaries
        self._wrap_E = E

    def wrapper_step(self, obs, rewards, dist, collision_penalty, out=None):
        """obs: raw env observation (spatial_edges [E,H,2(P+1)] by human id, visible_masks u8/bool); rewards [E] float32 updated in place."""
        E, D = obs["robot_node"].shape[0], 2 * (self.P + 1)
        if tuple(obs["spatial_edges"].shape) != (E, self.H, D) or (out is not None and tuple(out.shape) != (E, self.H, D)):
            raise A.CnError("HipGST.wrapper_step: spatial_edges (and out) must be [%d,%d,%d] for a horizon of %d steps (got %s)"
                            % (E, self.H, D, self.P, tuple(obs["spatial_edges"].shape)))
        if out is None:
            out = torch.empty(E, self.H, D, device=self.device)
        o = A.Obs()
        o.robot_node = A.ptr(obs["robot_node"])
        o.spatial_edges = A.ptr(obs["spatial_edges"])
        vm = obs["visible_masks"]
        vm = vm.view(torch.uint8) if vm.dtype == torch.bool else vm
        o.visible_masks = A.ptr(vm.contiguous())
        A.call("cn_gst_wrapper_step", self._h, E, C.byref(o), float(dist), float(collision_penalty), A.ptr(rewards), A.ptr(out), A.stream_ptr(), device=self.device)
        return out


class HipGstTrainer:
    """The training step of the predictor on the MI355X through the C ABI: forward + negative log-likelihood + backward as ONE boundary call
    (cn_gst_train_step, csrc/gst_train.hip: one workgroup per sequence, hand-derived reverse pass, the reference's four dropout sites with the
    library's own counter-based masks) and gradient-norm clip + Adam as another (flat_adam.FlatAdam: cn_adam_clip_step over one flat bucket).  Replaces, per
    optimiser step, train.py:121-146: model(...) -> negative_log_likelihood_full_partial -> loss.backward() -> clip_grad_norm_ -> optimizer.step().
    The model's parameters become views of the flat bucket, so state_dict() / checkpoints are those of the torch path."""

    def __init__(self, model, lr=1e-3, clip_grad=10.0, betas=(0.9, 0.999), eps=1e-8, seed=1000, optimizer=None):
        named = predictor_params(model)
        gst_weights([p for _, p in named], "HipGstTrainer")   # refuses a CPU model before anything is rebound
        self.model = model
        self.flat = FlatAdam(named, optimizer)   # the torch optimiser object stays the owner of the moments (its state_dict() goes into the checkpoints)
        self.w, self.g = (gst_weights([v[i] for v in self.flat.views], "HipGstTrainer") for i in (0, 1))
        self.lr, self.clip_grad, self.betas, self.eps, self.seed = float(lr), clip_grad, betas, float(eps), int(seed)
        self.ws, self.dev = None, self.flat.p.device

    @property
    def step_no(self):
        return self.flat.step_no

    def loss_and_grads(self, v_obs, v_pred, loss_mask_rel, p_drop=0.1, seed=None):
        """v_obs [B,5,N,2], v_pred [B,P,N,2], loss_mask_rel [B,N,5+P] (any device; P = the horizon, 1 .. 8) -> (loss_and_count [2] on the device,
        gauss [B,P,N,5]: mu_x, mu_y, sigma_x, sigma_y, corr); the gradients land in the flat bucket (every parameter's .grad).  Crowds of fewer than 4 pedestrians are padded
        with absent ones."""
        N, P, vo, vp, lm, _ = gst_batch("HipGstTrainer", self.dev, v_obs, v_pred, loss_mask_rel)
        B, Np = vo.shape[0], vo.shape[2]
        self.ws = workspace(self.ws, int(A.lib().cn_gst_train_workspace_bytes_horizon(B, Np, P)), self.dev)
        out = torch.empty(2, device=self.dev)
        gauss = torch.empty(B, P, Np, 5, device=self.dev)
        sd = self.seed + 7919 * self.step_no if seed is None else int(seed)
        A.call("cn_gst_train_step_horizon", B, Np, P, A.ptr(vo), A.ptr(vp), A.ptr(lm), C.byref(self.w), C.byref(self.g), float(p_drop), C.c_uint64(sd & (2 ** 64 - 1)),
               C.c_void_p(self.ws.data_ptr()), int(self.ws.numel()), A.ptr(out), A.ptr(gauss), A.stream_ptr(), device=self.dev)
        return out, gauss[:, :, :N]

    def optimizer_step(self, grad_scale=1.0):
        """clip_grad_norm_(parameters, clip_grad) + Adam.step() (train.py:143-146) over the flat bucket.  grad_scale multiplies the gradient before
        the norm is taken (train.py:134: loss / args.batch_size ahead of backward and clip_grad_norm_)."""
        self.flat.step(self.lr, self.betas, self.eps, self.clip_grad, grad_scale=grad_scale)
        self.flat.sync_optimizer_state()


class HipGstEvaluator:
    """Evaluation of the predictor on the MI355X through the C ABI: cn_gst_eval_step (csrc/gst_eval.hip) runs, for a batch of sequences in one
    boundary call, what eval.py:63-117 does per sequence -- the forward with dropout off, the masked negative log-likelihood and the
    average / final offset errors; validation (the mean fed back) or the test protocol (S sampled decodes per sequence on the caller's draws).
    The kernels read the model's parameters where they are (also when they are views of a HipGstTrainer's flat bucket): nothing is copied."""

    MAX_PEDS, MAX_SAMPLES = 64, 64

    def __init__(self, model):
        self.model = model
        params = self._params()
        gst_weights(params, "HipGstEvaluator")                # refuses a CPU model
        self.dev, self.ws = params[0].device, None

    def _params(self):
        return [p for _, p in predictor_params(self.model)]

    def evaluate_batch(self, v_obs, v_pred, loss_mask_rel, noise=None):
        """v_obs [B,5,N,2], v_pred [B,P,N,2], loss_mask_rel [B,N,5+P] (any device; P = the horizon, 1 .. 8), or lists of B per-sequence tensors
        ([5,N_b,2] / [P,N_b,2] / [N_b,5+P], a leading axis of one allowed) of different crowd sizes; noise None (validation) or [B,S,P,N,2] / a
        list of [S,P,N_b,2] (test: S decodes per
        sequence on these standard-normal draws).  Crowds are padded to the batch's largest (at least four) with absent pedestrians.
        -> seq [B,R,4] (NLL sum, valid pairs, sum of masked aoe, sum of masked foe), ped [B,R,N,3] (aoe, foe, loss_mask_per_pedestrian),
        gauss [B,R,P,N,5] (mu_x, mu_y, sigma_x, sigma_y, corr), R = max(S, 1), all on the device (nothing is read back here)."""
        N, P, vo, vp, lm, nz = gst_batch("HipGstEvaluator", self.dev, self._stack(v_obs, 3, 1), self._stack(v_pred, 3, 1), self._stack(loss_mask_rel, 2, 0),
                                      None if noise is None else self._stack(noise, 4, 2), self.MAX_SAMPLES)
        B, Np, S = vo.shape[0], vo.shape[2], 0 if nz is None else int(nz.shape[1])
        w = gst_weights(self._params(), "HipGstEvaluator")    # on every call: the parameters may be views of a trainer's bucket rebound since
        self.ws = workspace(self.ws, int(A.lib().cn_gst_eval_workspace_bytes_horizon(B, Np, S, P)), self.dev)
        R = max(S, 1)
        seq, ped, gauss = torch.empty(B, R, 4, device=self.dev), torch.empty(B, R, Np, 3, device=self.dev), torch.empty(B, R, P, Np, 5, device=self.dev)
        A.call("cn_gst_eval_step_horizon", B, Np, S, P, A.ptr(vo), A.ptr(vp), A.ptr(lm), C.byref(w), A.ptr(nz), C.c_void_p(self.ws.data_ptr()), int(self.ws.numel()),
               A.ptr(seq), A.ptr(ped), A.ptr(gauss), A.stream_ptr(), device=self.dev)
        return seq, ped[:, :, :N], gauss[:, :, :, :N]

    @staticmethod
    def _stack(x, rank, ax):
        """A tensor as it is; a list of per-sequence tensors of `rank` axes (a leading axis of one allowed) padded along the pedestrian axis `ax`
        with zeros (absent pedestrians) and stacked."""
        if torch.is_tensor(x):
            return x
        xs = [t[0] if t.dim() == rank + 1 else t for t in x]
        n = max(t.shape[ax] for t in xs)
        out = []
        for t in xs:
            if t.shape[ax] != n:
                shape = list(t.shape)
                shape[ax] = n - t.shape[ax]
                t = torch.cat((t, torch.zeros(shape, dtype=t.dtype, device=t.device)), dim=ax)
            out.append(t)
        return torch.stack(out, 0)
