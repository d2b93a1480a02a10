"""`python -m regennet_amd.sample.edit` — counterpart of the reference's `sample/edit.py` (motion in-painting) on this project's CLI
conventions (sample/cgenerate.py: --synthetic, --arch, --guidance_param, --unconstrained, batch sharding under torch.distributed.run,
the same output file layout).

The known part of a reactor motion is kept and the rest is generated: y['inpainting_mask'] (True = keep the input) and
y['inpainted_motion'] go to p_sample_loop / ddim_sample_loop, which blend them into every step's prediction inside the fused engine
loop (gaussian_diffusion.py:319-323, rgn_set_inpainting).

  --edit_mode in_between   frames [int(prefix_end * T), int(suffix_start * T)) are generated, all others kept (edit.py:76-83)
  --edit_mode rows         the pose rows of --keep_rows (e.g. 0-21,55) are kept in every frame, the others generated. This takes the place
                           of the reference's 'upper_body', a HumanML3D feature mask with no meaning for 56 SMPL-X rows.
  --edit_mode upper_body   --dataset humanml only: the rows of humanml_utils.HML_LOWER_BODY_MASK (root, lower-body joints, foot contacts) are
                           kept in every frame and the upper body is generated (edit.py:84-88). 'motion' and 'input_motion' then hold the joint
                           positions of the result and of the input motions (edit.py:117-121, :153-156; utils/hml.py), de-normalised with
                           --hml_stats when given.

Input motions: --input_motions FILE.npy [N, njoints, nfeats, T], or synthetic ones with --synthetic. Like the reference's edit.py (and
unlike cgenerate) the result is stored unsmoothed, so its kept part equals the input bit for bit; 'mask' and 'input_motions' are stored
beside 'output' and 'cmotion'. With --skeleton FILE.npz | synthetic (see cgenerate) 'motion' holds the joint positions model.rot2xyz gives
for that output."""
import os
import time
import types

import numpy as np


def in_between_mask(shape, prefix_end, suffix_start):
    """bool [B, njoints, nfeats, T], True = keep the input: every frame outside [int(prefix_end * T), int(suffix_start * T))
    (edit.py:76-83 with full-length motions)."""
    T = int(shape[-1])
    mask = np.ones(tuple(int(s) for s in shape), dtype=bool)
    mask[..., int(prefix_end * T):int(suffix_start * T)] = False
    return mask


def rows_mask(shape, rows):
    """bool [B, njoints, nfeats, T], True = keep the input: the pose rows `rows` of every frame."""
    rows = [int(r) for r in rows]
    if any(r < 0 or r >= int(shape[1]) for r in rows):
        raise ValueError(f"keep_rows {rows} outside [0, {int(shape[1])})")
    mask = np.zeros(tuple(int(s) for s in shape), dtype=bool)
    mask[:, rows] = True
    return mask


def parse_rows(spec):
    """'0-21,55' -> [0, 1, ..., 21, 55]."""
    rows = []
    for part in str(spec).split(","):
        part = part.strip()
        if not part:
            continue
        lo, _, hi = part.partition("-")
        rows.extend(range(int(lo), int(hi if hi else lo) + 1))
    if not rows:
        raise ValueError("--edit_mode rows needs --keep_rows, e.g. 0-21,55")
    return sorted(set(rows))


def upper_body_mask(shape):
    """bool [B, 263, 1, T], True = keep the input: HML_LOWER_BODY_MASK over every motion, feature and frame (edit.py:84-88), so the lower body and
    the root are kept and the upper body is generated."""
    from ..data_loaders.humanml_utils import HML_LOWER_BODY_MASK
    return np.ascontiguousarray(np.broadcast_to(HML_LOWER_BODY_MASK[None, :, None, None], tuple(int(s) for s in shape)))


def build_mask(args, shape):
    if args.edit_mode == "in_between":
        return in_between_mask(shape, args.prefix_end, args.suffix_start)
    if args.edit_mode == "rows":
        return rows_mask(shape, parse_rows(args.keep_rows))
    if len(shape) == 4 and tuple(int(s) for s in shape[1:3]) == (263, 1):      # the HumanML3D vector, the one layout the reference's mask is written for
        return upper_body_mask(shape)
    raise NotImplementedError(
        "--edit_mode upper_body is the reference's HumanML3D feature mask (humanml_utils.HML_LOWER_BODY_MASK): it is written for the 263 x 1 rows of "
        "--dataset humanml and has no meaning for KIT's 251 rows or the "
        "56 SMPL-X pose rows of a reaction model: name the rows to keep instead, --edit_mode rows --keep_rows 0-21,55")


def main(argv=None):
    """Single process or sharded under `python -m torch.distributed.run --nproc-per-node N -m regennet_amd.sample.edit ...`, exactly as
    cgenerate: contiguous shards of every repetition, Philox noise keyed by the global sample index, rank 0 gathers and saves."""
    import torch

    from .. import synth
    from ..model.cfg_sampler import ClassifierFreeSampleModel
    from ..utils import dist_util
    from ..utils.fixseed import fixseed
    from ..utils.model_util import create_model_and_diffusion, load_model_wo_clip
    from ..utils.parser_util import edit_args
    from .cgenerate import (HML_DATASETS, HML_MAX_FRAMES, dataset_config, hml_statistics, joint_positions, load_text_features, mesh_results, motion_rows,
                            set_skeleton, vertex_positions)

    args = edit_args(argv)
    fixseed(args.seed)
    hml = args.dataset in HML_DATASETS
    max_frames = HML_MAX_FRAMES if hml else 150 if args.dataset == "chi3d" else 60
    n_frames = min(max_frames, int(args.motion_length))
    cfg = dataset_config(args)
    B = args.num_samples
    full_mask = build_mask(args, (B, cfg["njoints"], cfg["nfeats"], n_frames))       # (raises for upper_body before anything is built)
    hml_mean, hml_std = hml_statistics(args) if hml else (None, None)
    dev = dist_util.setup_dist()
    rank, world = dist_util.world()
    assert args.num_samples <= args.batch_size, \
        f"Please either increase batch_size({args.batch_size}) or reduce num_samples({args.num_samples})"
    args.batch_size = B
    data = types.SimpleNamespace(dataset=types.SimpleNamespace(num_actions=cfg["num_actions"], num_person=2))
    if args.arch == "gru":     # (--gru_scan reaches the model through get_model_args)
        model, diffusion = create_model_and_diffusion(args, data, allow_gru=True)
    else:
        model, diffusion = create_model_and_diffusion(args, data, allow_mlp=True)
    model.precision = args.precision
    if args.synthetic or not args.model_path:
        sd = {k: torch.from_numpy(v) for k, v in
              synth.make_state_dict(model.engine_config() | {"layers": model.num_layers}, seed=0 if rank == 0 else 1000 + rank).items()}
    else:
        sd = torch.load(args.model_path, map_location="cpu")
    load_model_wo_clip(model, sd)
    if args.guidance_param != 1:
        model = ClassifierFreeSampleModel(model)
    model.to(dev)
    model.eval()
    dist_util.sync_model_weights(model, 0)
    reps = max(1, args.num_repetitions)
    if args.cmotion_npz:
        z = np.load(args.cmotion_npz)
        clips = np.asarray(z["cmotion"], dtype=np.float32)
        actions = np.asarray(z["action"], dtype=np.int64).reshape(-1, 1) if "action" in z else np.zeros((len(clips), 1), np.int64)
    else:
        clips, actions = synth.make_cmotion(cfg, B * reps, seed=1), synth.make_actions(cfg, B * reps, seed=2)
    if args.input_motions:
        inputs = np.asarray(np.load(args.input_motions), dtype=np.float32)
    elif args.synthetic or not args.model_path:
        inputs = synth.make_cmotion(cfg, B * reps, seed=4)                              # (a second family of rot6d clips: the motions to edit)
    else:
        raise SystemExit("--input_motions FILE.npy is required (or --synthetic)")
    for name, a in (("actor clips", clips), ("input motions", inputs)):
        assert a.ndim == 4 and a.shape[1:3] == (cfg["njoints"], cfg["nfeats"]) and a.shape[3] >= n_frames, \
            f"{name} {a.shape} do not cover [N, {cfg['njoints']}, {cfg['nfeats']}, {n_frames}]"
    clips, inputs = clips[..., :n_frames], inputs[..., :n_frames]
    lo, hi = dist_util.shard_bounds(B)
    Bl = hi - lo
    sample_fn = diffusion.p_sample_loop if not args.use_ddim else diffusion.ddim_sample_loop
    inner = model.model if isinstance(model, ClassifierFreeSampleModel) else model
    shape = (Bl, inner.njoints, inner.nfeats, n_frames)
    with_motion = hml or set_skeleton(inner, args)
    if getattr(args, "betas_npz", ""):
        raise SystemExit("--betas_npz is served by cgenerate and render; the edit CLI draws every motion on the file's one shape")
    texts = load_text_features(args, B, inner.clip_dim) if inner.cond_mode == "text" else None
    if hml:
        from ..utils.hml import hml_to_joints, joints_of
        eng, _ = inner._get_engine(max(Bl, 1), n_frames)

        def hml_joints(x):       # edit.py:117-121, :153-156: inv_transform + recover_from_ric, one launch
            return hml_to_joints(x, hml_mean, hml_std, engine=eng) if Bl > 0 else torch.empty((0, joints_of(inner.njoints), 3, n_frames), device=dev)

    def make_y(rep_i):
        idx = (np.arange(lo, hi) + rep_i * B) % len(clips)
        idm = (np.arange(lo, hi) + rep_i * B) % len(inputs)
        y = {"cmotion": torch.from_numpy(np.ascontiguousarray(clips[idx])).to(dev), "lengths": torch.full((Bl,), n_frames),
             "mask": torch.ones(Bl, 1, 1, n_frames, dtype=torch.bool),
             "inpainted_motion": torch.from_numpy(np.ascontiguousarray(inputs[idm])).to(dev),
             "inpainting_mask": torch.from_numpy(np.ascontiguousarray(full_mask[lo:hi])).to(dev)}      # True means: use the input motion
        if inner.cond_mode == "action":
            y["action"] = torch.from_numpy(actions[idx]).to(dev)
        if inner.cond_mode == "text":
            y["text_features"] = torch.from_numpy(np.ascontiguousarray(texts[(np.arange(lo, hi) + rep_i * B) % len(texts)])).to(dev)
        if args.guidance_param != 1:
            y["scale"] = torch.ones(Bl, device=dev) * args.guidance_param
        return y

    if world > 1:
        diffusion.agree_x3_tail(model, shape, {"y": make_y(0)} if Bl > 0 else None, sampler="ddim" if args.use_ddim else "ddpm")
    with_vertices = with_motion and args.vertices
    nverts = inner.rot2xyz.mesh["v_template"].shape[0] if with_vertices else 0
    outs, cms, ins, motions, vertices, in_joints = [], [], [], [], [], []
    for rep_i in range(args.num_repetitions):
        if rank == 0:
            print(f"### Start sampling [repetitions #{rep_i}]")
        y = make_y(rep_i)
        dist_util.synchronize()
        t_start = time.time()
        if Bl > 0:
            sample = sample_fn(model, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=0, init_image=None,
                               progress=(rank == 0), dump_steps=None, noise=None, const_noise=False,
                               seed=args.seed * 1000003 + rep_i, sample_offset=rep_i * B + lo)
        else:
            sample = torch.empty(shape, device=dev)
        dist_util.synchronize()
        if rank == 0:
            print("Editing time consumption: %s ms" % ((time.time() - t_start) * 1000))
        outs.append(dist_util.all_gather_samples(sample, B).cpu().numpy())
        cms.append(dist_util.all_gather_samples(y["cmotion"], B).cpu().numpy())
        ins.append(dist_util.all_gather_samples(y["inpainted_motion"], B).cpu().numpy())
        if hml:
            motions.append(dist_util.all_gather_samples(hml_joints(sample), B).cpu().numpy())
            in_joints.append(dist_util.all_gather_samples(hml_joints(y["inpainted_motion"]), B).cpu().numpy())
        elif with_motion:
            motion = joint_positions(inner, args, sample, y) if Bl > 0 else torch.empty((0, motion_rows(inner, args), 3, n_frames), device=dev)
            motions.append(dist_util.all_gather_samples(motion, B).cpu().numpy())
        if with_vertices:
            verts = vertex_positions(inner, args, sample, y) if Bl > 0 else torch.empty((0, nverts, 3, n_frames), device=dev)
            vertices.append(dist_util.all_gather_samples(verts, B).cpu().numpy())
    npy_path = None
    if rank == 0:
        out_path = args.output_dir or os.path.join(os.path.dirname(args.model_path) or ".", f"edit_seed{args.seed}_{args.edit_mode}")
        os.makedirs(out_path, exist_ok=True)
        npy_path = os.path.join(out_path, "results.npy")
        print(f"saving results file to [{npy_path}]")
        np.save(npy_path, {**({"motion": np.concatenate(motions)} if with_motion else {}),
                           **({"input_motion": np.concatenate(in_joints)} if hml else {}),
                           **(mesh_results(inner, args, vertices, np.full((len(outs) * B,), n_frames)) if with_vertices else {}), "output": np.concatenate(outs), "cmotion": np.concatenate(cms), "input_motions": np.concatenate(ins),
                           "mask": np.concatenate([full_mask] * len(outs)), "edit_mode": args.edit_mode,
                           "lengths": np.full((len(outs) * B,), n_frames), "num_samples": args.num_samples,
                           "num_repetitions": args.num_repetitions, "world_size": world})
        print(f"[Done] Results are at [{os.path.abspath(out_path)}]")
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    return npy_path


if __name__ == "__main__":
    main()
