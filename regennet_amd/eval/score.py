"""Score held-out motions with the terms of the training objective (`diffusion.training_losses`): a table of the mean of each term per
timestep, and the per-motion values in `scores.npy`. Far cheaper than the FID evaluation: one denoiser evaluation and one kernel
(rgn_loss_terms) per batch and timestep, no sampling.

    python -m regennet_amd.eval.score --model_path save/cmdm_ntu/model000300000.pt --data_path heldout.npy --skeleton skel.npz --t_grid 10
    python -m regennet_amd.eval.score --synthetic --skeleton synthetic --num_samples 8 --t_grid 5

--data_path FILE.npy holds a dict with 'motion' [N, 56, 6, T] (the reactions, rot6d rows + translation row), 'cmotion' (the actors, same shape)
and 'lengths' [N] (+ 'action' [N] for an action-conditioned model); without one, --num_samples synthetic motions. --skeleton FILE.npz |
synthetic supplies the rest joints of the joint terms (tools/make_skeleton.py). Every motion is scored at --t_grid evenly spaced timesteps of the
(respaced) schedule with Philox noise keyed by (--seed, motion, timestep), so a motion's noise depends neither on the batch size nor on
the other motions. The weights: parser_util.score_args.

    python -m regennet_amd.eval.score --bpd --model_path save/cmdm_ntu/model000300000.pt --data_path heldout.npy --t_grid 10

--bpd scores with the variational bound instead (`diffusion.calc_bpd_loop`, rgn_q_sample_rows + rgn_vb_terms): every timestep of the (respaced)
schedule in bits per dimension, the number that compares checkpoints and noise schedules without sampling. The table shows vb, xstart_mse and
mse at --t_grid timesteps and the mean prior_bpd / total_bpd; scores.npy holds total_bpd, prior_bpd [N] and vb, xstart_mse, mse [S, N] in
ascending t. The noise is keyed as above; no skeleton is needed."""
import os
import types

import numpy as np
import torch

from .. import synth
from ..sample.cgenerate import set_skeleton
from ..utils import dist_util
from ..utils.fixseed import fixseed
from ..utils.model_util import create_model_and_diffusion, load_model_wo_clip
from ..utils.parser_util import score_args


def load_motions(args, cfg):
    """-> motion, cmotion fp32 [N, njoints, nfeats, T], lengths int64 [N], action int64 [N, 1]."""
    if args.data_path:
        d = np.load(args.data_path, allow_pickle=True).item()
        motion, cmotion = (np.asarray(d[k], dtype=np.float32) for k in ("motion", "cmotion"))
        lengths = np.asarray(d["lengths"], dtype=np.int64).reshape(-1)
        action = np.asarray(d["action"], dtype=np.int64).reshape(-1, 1) if "action" in d else np.zeros((len(motion), 1), np.int64)
    else:
        n = args.num_samples
        motion, cmotion = synth.make_cmotion(cfg, n, seed=4), synth.make_cmotion(cfg, n, seed=1)
        lengths, action = np.full(n, cfg["num_frames"], np.int64), synth.make_actions(cfg, n, seed=2)
    if motion.shape != cmotion.shape or len(lengths) != len(motion) or lengths.min() < 1 or lengths.max() > motion.shape[-1]:
        raise SystemExit(f"motion {motion.shape}, cmotion {cmotion.shape}, lengths {lengths.shape}: two [N, njoints, nfeats, T] arrays and N lengths in [1, T] expected")
    return motion, cmotion, lengths, action


def timestep_grid(num_timesteps, n):
    """n evenly spaced indices of the schedule, first and last included (n = 1: the middle)."""
    if n == 1:
        return [num_timesteps // 2]
    return sorted({int(round(i * (num_timesteps - 1) / (n - 1))) for i in range(n)})


def format_table(grid, scores):
    keys = [k for k in scores if k != "loss"] + ["loss"]
    lines = ["%6s " % "t" + " ".join("%12s" % k for k in keys)]
    for i, t in enumerate(grid):
        lines.append("%6d " % t + " ".join("%12.5e" % float(np.nanmean(scores[k][i])) for k in keys))
    return "\n".join(lines)


BPD_COLUMNS = ("vb", "xstart_mse", "mse")


def format_bpd_table(grid, scores):
    lines = ["%6s " % "t" + " ".join("%12s" % k for k in BPD_COLUMNS)]
    for t in grid:
        lines.append("%6d " % t + " ".join("%12.5e" % float(np.nanmean(scores[k][t])) for k in BPD_COLUMNS))
    return "\n".join(lines)


def score_bpd(args, model, diffusion, cfg, dev):
    """--bpd: diffusion.calc_bpd_loop over the whole (respaced) schedule, batch by batch. The noise of (motion i, timestep t) is the Philox draw
    keyed by (--seed, i, t): a motion's numbers depend neither on --batch_size nor on the other motions."""
    motion, cmotion, lengths, action = load_motions(args, cfg)
    if motion.shape[1:3] != (model.njoints, model.nfeats):
        raise SystemExit(f"motions {motion.shape} do not fit the model's [N, {model.njoints}, {model.nfeats}, T]")
    N, T = len(motion), motion.shape[-1]
    S = diffusion.num_timesteps
    bs = max(1, min(args.batch_size, N))
    parts = {}
    for lo in range(0, N, bs):
        hi = min(N, lo + bs)
        y = {"cmotion": torch.from_numpy(cmotion[lo:hi]).to(dev), "lengths": torch.from_numpy(lengths[lo:hi]),
             "mask": (torch.arange(T)[None, :] < torch.from_numpy(lengths[lo:hi])[:, None]).reshape(hi - lo, 1, 1, T)}
        if model.cond_mode == "action":
            y["action"] = torch.from_numpy(action[lo:hi]).to(dev)
        out = diffusion.calc_bpd_loop(model, torch.from_numpy(motion[lo:hi]).to(dev), clip_denoised=True, model_kwargs={"y": y}, seed=args.seed,
                                      sample_offset=lo)
        for k, v in out.items():
            parts.setdefault(k, []).append(v.cpu().numpy())
    scores = {k: np.concatenate(v) for k, v in parts.items()}
    for k in BPD_COLUMNS:
        scores[k] = np.ascontiguousarray(scores[k][:, ::-1].T)              # [N, S] in the loop's descending order -> [S, N], ascending t
    grid = timestep_grid(S, args.t_grid)
    print(f"{N} motions of {T} frames, variational bound over {S} timesteps in bits per dimension; mean per timestep at {len(grid)} of them:")
    print(format_bpd_table(grid, scores))
    print("prior_bpd %.5e  total_bpd %.5e" % (float(np.nanmean(scores["prior_bpd"])), float(np.nanmean(scores["total_bpd"]))))
    out_dir = args.output_dir or os.path.dirname(args.model_path) or "."
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "scores.npy")
    np.save(path, dict(scores, timesteps=np.arange(S), lengths=lengths))
    print(f"saved the per-motion values to [{os.path.abspath(path)}]")
    return path


def main(argv=None):
    args = score_args(argv)
    if args.arch == "gru":
        raise NotImplementedError("eval.score does not take --arch gru: its --bpd path stacks timesteps as rows of one evaluation, and the gru model's "
                                  "batch scan (the reference's recurrence over the samples of a call) would couple them (DESIGN.md §9)")
    fixseed(args.seed)
    dev = dist_util.setup_dist()
    cfg = synth.get_config("chi3d" if args.dataset == "chi3d" else ("ntu" if args.unconstrained else "ntu_action"))
    data = types.SimpleNamespace(dataset=types.SimpleNamespace(num_actions=cfg["num_actions"], num_person=2))
    model, diffusion = create_model_and_diffusion(args, data, allow_mlp=True)
    model.precision = args.precision
    if args.synthetic or not args.model_path:
        sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(model.engine_config() | {"layers": model.num_layers}, seed=0).items()}
    else:
        print(f"Loading checkpoints from [{args.model_path}]...")
        sd = torch.load(args.model_path, map_location="cpu")
    load_model_wo_clip(model, sd)
    model.to(dev)
    model.eval()
    if args.bpd:
        return score_bpd(args, model, diffusion, cfg, dev)
    if not set_skeleton(model, args):
        raise SystemExit("the joint terms need rest joints: --skeleton FILE.npz (tools/make_skeleton.py) or --skeleton synthetic")
    motion, cmotion, lengths, action = load_motions(args, cfg)
    if motion.shape[1:3] != (model.njoints, model.nfeats):
        raise SystemExit(f"motions {motion.shape} do not fit the model's [N, {model.njoints}, {model.nfeats}, T]")
    N, T = len(motion), motion.shape[-1]
    grid = timestep_grid(diffusion.num_timesteps, args.t_grid)
    bs = max(1, min(args.batch_size, N))
    eng, _ = model._get_engine(bs, T)
    scores = {}
    for gi, ts in enumerate(grid):
        rows = {}
        for lo in range(0, N, bs):
            hi = min(N, lo + bs)
            x0 = torch.from_numpy(motion[lo:hi]).to(dev)
            y = {"cmotion": torch.from_numpy(cmotion[lo:hi]).to(dev), "lengths": torch.from_numpy(lengths[lo:hi]),
                 "mask": (torch.arange(T)[None, :] < torch.from_numpy(lengths[lo:hi])[:, None]).reshape(hi - lo, 1, 1, T)}
            if model.cond_mode == "action":
                y["action"] = torch.from_numpy(action[lo:hi]).to(dev)
            noise = diffusion._keyed_normal(eng, x0.shape, args.seed, lo, ts, dev)
            out = diffusion.training_losses(model, x0, torch.full((hi - lo,), ts, device=dev, dtype=torch.long), model_kwargs={"y": y}, noise=noise,
                                            dataset=args.dataset)
            for k, v in out.items():
                rows.setdefault(k, []).append(v.cpu().numpy())
        for k, v in rows.items():
            scores.setdefault(k, []).append(np.concatenate(v))
    scores = {k: np.stack(v) for k, v in scores.items()}                    # [len(grid), N] each
    print(f"{N} motions of {T} frames at {len(grid)} of {diffusion.num_timesteps} timesteps; mean per timestep:")
    print(format_table(grid, scores))
    out_dir = args.output_dir or os.path.dirname(args.model_path) or "."
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "scores.npy")
    np.save(path, dict(scores, timesteps=np.array(grid), lengths=lengths))
    print(f"saved the per-motion values to [{os.path.abspath(path)}]")
    return path


if __name__ == "__main__":
    main()
