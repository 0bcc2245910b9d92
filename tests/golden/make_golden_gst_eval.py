#!/usr/bin/env python3
"""Golden vectors for the GST EVALUATION path (build container only): the reference's model, loss and offset errors driven the way
gst_updated/scripts/experiments/eval.py `inference` drives them, on the 120-frame file of make_golden_gst_train.py with the same formula weights.

  (i)  mode 'val' (eval.py:69-82, :138-147) over the validation split (TrajectoriesDataset mode='val'): per-sequence loss, sum of masked aoe / foe,
       number of fully present pedestrians, and the pass's triple;
  (ii) mode 'test' (eval.py:84-117, :148-157) with 20 samples for sequences 0, 41, 77 of the whole file: the standard-normal draws the reference's
       sample_gaussian consumed (recorded from Tensor.normal_ while st_model.forward runs: five draws of [1,1,N,2] per decode), the per-sample
       loss / aoe sum / foe sum, the Gaussian parameters of every sample and the seven aggregated numbers over the three sequences.
"""
import argparse
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import as R  # noqa: E402
import make_golden_gst as MG  # noqa: E402

R.install()
sys.path.insert(0, os.path.join(R.REF, "gst_updated"))
FRAMES = 120
ITEMS = (0, 41, 77)
SAMPLES = 20


def main():
    import torch
    from src.mgnn.trajectories import TrajectoriesDataset
    from src.mgnn.utils import average_offset_error, final_offset_error
    from gst_updated.src.gumbel_social_transformer.st_model import st_model, negative_log_likelihood_full_partial
    z = np.load(os.path.join(HERE, "collect_h20_nonrand_r0.npz"))
    lines = [ln for ln in str(z["lines"]).split("\n") if float(ln.split("\t")[0]) < FRAMES]
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "0.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        ds = TrajectoriesDataset(d, obs_seq_len=5, pred_seq_len=5, skip=1, delim="\t", frame_diff=1.0)
        ds_val = TrajectoriesDataset(d, obs_seq_len=5, pred_seq_len=5, skip=1, delim="\t", frame_diff=1.0, mode="val")
    args = argparse.Namespace(**MG.GST_ARGS)
    torch.manual_seed(0)
    model = st_model(args, device="cpu")
    sd = MG.gst_formula_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.eval()

    def run(item, sampling, hard):
        obs_traj, pred_traj_gt, obs_traj_rel, pred_traj_rel_gt, loss_mask_rel, loss_mask, v_obs, A_obs, v_pred_gt, A_pred_gt, amo, amp = [t.unsqueeze(0) for t in item]
        gp, xs, info = model(v_obs, A_obs, amo, loss_mask_rel, tau=0.03, hard=hard, sampling=sampling, device="cpu")
        prob_loss, elm = negative_log_likelihood_full_partial(gp, v_pred_gt, info["loss_mask_rel_full_partial"], loss_mask_rel[:, :, -args.pred_seq_len:])
        lm = info["loss_mask_per_pedestrian"]
        return (prob_loss.sum() / elm.sum(), average_offset_error(xs, v_pred_gt, loss_mask=lm), final_offset_error(xs, v_pred_gt, loss_mask=lm), lm, gp)

    out = {"val_num_seq": np.array(len(ds_val)), "val_frame_id_seq": np.array(ds_val.frame_id_seq), "items": np.array(ITEMS), "samples": np.array(SAMPLES)}
    with torch.no_grad():
        # (i) validation mode
        loss, aoe, foe, m = [], [], [], []
        for it in range(len(ds_val)):
            l, a, f, lm, _ = run(ds_val[it], False, False)
            loss.append(l.item()); aoe.append(a.numpy()); foe.append(f.numpy()); m.append(lm[0].numpy())
        out["val_loss"] = np.array(loss, dtype=np.float32)
        out["val_aoe_sum"] = np.array([a.sum() for a in aoe], dtype=np.float32)
        out["val_foe_sum"] = np.array([f.sum() for f in foe], dtype=np.float32)
        out["val_m"] = np.array([x.sum() for x in m], dtype=np.float32)
        msum = np.concatenate(m).sum()
        out["val_triple"] = np.array([np.mean(loss), np.concatenate(aoe).sum() / msum, np.concatenate(foe).sum() / msum], dtype=np.float64)
        # (ii) test mode, the draws recorded as the reference consumes them
        draws = []
        orig = torch.Tensor.normal_

        def recording_normal_(self, *a, **k):
            r = orig(self, *a, **k)
            draws.append(r.detach().clone())
            return r

        torch.manual_seed(2024)
        agg = {k: [] for k in ("loss", "aoe_mean", "aoe_std", "aoe_min", "foe_mean", "foe_std", "foe_min")}
        masks = []
        for it in ITEMS:
            n = ds[it][0].shape[0]
            noise, l_s, a_s, f_s, gauss = [], [], [], [], []
            for _ in range(SAMPLES):
                del draws[:]
                torch.Tensor.normal_ = recording_normal_
                try:
                    l, a, f, lm, gp = run(ds[it], True, True)
                finally:
                    torch.Tensor.normal_ = orig
                assert len(draws) == 5 and all(tuple(t.shape) == (1, 1, n, 2) for t in draws), [tuple(t.shape) for t in draws]
                noise.append(torch.cat(draws, 1)[0].numpy().copy())
                l_s.append(l); a_s.append(a); f_s.append(f)
                gauss.append(torch.cat(gp, -1)[0].numpy())
            a_t, f_t = torch.stack(a_s, 0).sum(1), torch.stack(f_s, 0).sum(1)
            out["test%d_noise" % it] = np.stack(noise).astype(np.float32)              # [S,5,N,2]
            out["test%d_loss" % it] = np.array([x.item() for x in l_s], dtype=np.float32)
            out["test%d_aoe_sum" % it] = a_t.numpy()
            out["test%d_foe_sum" % it] = f_t.numpy()
            out["test%d_gauss" % it] = np.stack(gauss).astype(np.float32)              # [S,5,N,5]
            out["test%d_m" % it] = np.array(lm[0].numpy().sum(), dtype=np.float32)
            agg["loss"].append((sum(l_s) / len(l_s)).item())
            for k, t in (("aoe", a_t), ("foe", f_t)):
                agg[k + "_mean"].append(t.mean().item()); agg[k + "_std"].append(t.std().item()); agg[k + "_min"].append(t.min().item())
            masks.append(lm[0].numpy())
            for k in ("loss", "aoe_mean", "aoe_std", "aoe_min", "foe_mean", "foe_std", "foe_min"):
                out["test%d_agg_%s" % (it, k)] = np.array(agg[k][-1], dtype=np.float64)
        msum = np.concatenate(masks).sum()
        out["test_seven"] = np.array([np.mean(agg["loss"]), sum(agg["aoe_mean"]) / msum, sum(agg["foe_mean"]) / msum, sum(agg["aoe_std"]) / msum,
                                      sum(agg["foe_std"]) / msum, sum(agg["aoe_min"]) / msum, sum(agg["foe_min"]) / msum], dtype=np.float64)
    path = os.path.join(HERE, "gst_eval_h20.npz")
    np.savez_compressed(path, **out)
    print("validation sequences %d, triple %s; test items %s x %d samples, seven %s -> %s (%.0f KB)"
          % (len(ds_val), out["val_triple"], ITEMS, SAMPLES, np.round(out["test_seven"], 4), os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
