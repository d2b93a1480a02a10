"""`python -m regennet_amd.sample.cgenerate` — counterpart of the reference's `sample/cgenerate.py` for the
sampling hot path: build model+diffusion through the reference-shaped factory, loop `num_repetitions` x
sample_fn with the reference's own timing hook (cgenerate.py:123,136-140,169), smooth with the sigma=1
temporal Gaussian (cgenerate.py:142) — here on the device — and save `results.npy`.

The reference pulls actor clips from its h5 datasets (licence-restricted, absent here) and finishes with SMPL-X
`rot2xyz`; this CLI takes actor clips from an .npz (or synthetic ones) and stores the rot6d output ('output',
'cmotion' keys as in the reference). With `--skeleton FILE.npz` (tools/make_skeleton.py; `synthetic`: synth.make_skeleton, NOT a body model's
skeleton) it also stores 'motion', the joint positions `model.rot2xyz` gives for the smoothed sample (cgenerate.py:154-163) - forward
kinematics on the device, no body model needed. With `--vertices` and a `--skeleton` that carries a mesh (a body file of
`tools/make_skeleton.py --mesh`; `synthetic`: synth.make_body) it also stores 'vertices' [N, V, 3, T] and 'faces', the meshes the reference
renders from (visualize/vis_utils.py:35-41), and `--obj_dir DIR` writes them as DIR/sample{i:02d}/frame{t:03d}.obj. `--render_dir DIR` draws them on the
device (utils/render.py; `--render_size N`, default 1024 as render/crendermotion.py:109-110) and writes DIR/sample{i:02d}/frame{t:03d}.png.
`--betas_npz FILE` ('betas' [N, nb]; `synthetic`: seeded N(0, 1)) gives every generated sample its own body shape - joints and meshes alike, read
per frame on the device (`betas_per_motion`) - cycled over repetitions like the actor clips, and stores 'betas' beside them.
`--jointstype vibe | a2m | a2mpl` makes 'motion' that joint type of the reference's SMPL layer (regressed from the mesh; [N, len(map), 3, T]) in
place of the skeleton's joints: it needs a `--skeleton` body file that holds the regressors and the type's map (`synthetic`:
synth.make_joint_regressors).

`--dataset humanml | kit` samples the HumanML3D / KIT feature vector (263 / 251 rows of one feature, up to 196 frames, text-conditioned: the CLIP
tower is out of scope, `--text_features FILE.npy` [N, clip_dim] or `--synthetic` ones go into y['text_features']). 'motion' is then what the reference
stores for such a model (cgenerate.py:147-152): the smoothed sample de-normalised with the dataset's Mean / Std (`--hml_stats PATH`) and turned into
joint positions [N, 22 | 21, 3, T] by recover_from_ric - one launch on the device (utils/hml.py, rgn_hml_to_joints). It needs no skeleton; the
options that need a body are refused."""
import os
import time
import types

import numpy as np
import torch

from .. import synth
from ..model.cfg_sampler import ClassifierFreeSampleModel
from ..utils import dist_util
from ..utils.fixseed import fixseed
from ..utils.model_util import create_model_and_diffusion, load_model_wo_clip
from ..utils.parser_util import cgenerate_args


def _load_clips(args, cfg, n):
    if args.cmotion_npz:
        z = np.load(args.cmotion_npz)
        cm = np.asarray(z["cmotion"], dtype=np.float32)
        act = np.asarray(z["action"], dtype=np.int64).reshape(-1, 1) if "action" in z else np.zeros((len(cm), 1), np.int64)
        return cm, act
    reps = max(1, args.num_repetitions)
    return synth.make_cmotion(cfg, n * reps, seed=1), synth.make_actions(cfg, n * reps, seed=2)


HML_DATASETS = ("humanml", "kit")
HML_MAX_FRAMES = 196        # max_motion_length of both datasets (data_loaders/humanml/utils/get_opt.py:63,70)


def dataset_config(args):
    """The synthetic configuration whose geometry the dataset's inputs (actor clips, text features) are drawn at."""
    if args.dataset in HML_DATASETS:
        return synth.get_config("ntu" if args.unconstrained else "text150", dataset=args.dataset, njoints={"humanml": 263, "kit": 251}[args.dataset],
                                nfeats=1, num_frames=HML_MAX_FRAMES, num_actions=1)
    return synth.get_config("chi3d" if args.dataset == "chi3d" else ("ntu" if args.unconstrained else "ntu_action"))


def hml_statistics(args):
    """--dataset humanml | kit: refuse what needs a body, then (mean, std) of --hml_stats, or (None, None) and one line that says so."""
    for flag, given in (("--skeleton", args.skeleton), ("--vertices", getattr(args, "vertices", False)), ("--jointstype", getattr(args, "jointstype", "")),
                        ("--betas_npz", getattr(args, "betas_npz", ""))):
        if given:
            raise SystemExit(f"{flag}: --dataset {args.dataset} samples a feature vector whose joint positions come from recover_from_ric, not from a "
                             f"body model's skeleton or mesh - there is no body for {flag} to act on")
    if not args.hml_stats:
        print("no --hml_stats: the features are taken as already de-normalised (the dataset's Mean / Std are not applied)")
        return None, None
    from ..utils.hml import load_hml_stats
    mean, std = load_hml_stats(args.hml_stats)
    rows = {"humanml": 263, "kit": 251}[args.dataset]
    if len(mean) != rows:
        raise SystemExit(f"--hml_stats: {args.hml_stats} holds {len(mean)} rows, --dataset {args.dataset} has {rows}")
    return mean, std


def load_text_features(args, n, clip_dim):
    """--text_features FILE.npy [N, clip_dim] (cycled over repetitions like the actor clips), or seeded synthetic ones."""
    if args.text_features:
        feats = np.ascontiguousarray(np.load(args.text_features, allow_pickle=False), dtype=np.float32)
        if feats.ndim != 2 or not len(feats) or feats.shape[1] != clip_dim:
            raise SystemExit(f"--text_features: {args.text_features} holds {feats.shape}, [N, {clip_dim}] expected")
        return feats
    if args.synthetic or not args.model_path:
        return synth.make_text_features({"clip_dim": clip_dim}, n * max(1, args.num_repetitions), seed=3)
    raise SystemExit("a text-conditioned model needs --text_features FILE.npy [N, clip_dim] (the CLIP tower is out of scope), or --synthetic")


def set_skeleton(model, args):
    """--skeleton FILE.npz | synthetic -> model.set_skeleton (the model inside a guidance wrapper). True when one was given."""
    vertices = getattr(args, "vertices", False)
    if getattr(args, "obj_dir", "") and not vertices:
        raise SystemExit("--obj_dir writes the meshes of --vertices")
    if getattr(args, "render_dir", "") and not vertices:
        raise SystemExit("--render_dir renders the meshes of --vertices")
    jointstype = getattr(args, "jointstype", "")
    if not args.skeleton:
        if vertices:
            raise SystemExit("--vertices needs --skeleton BODY.npz (tools/make_skeleton.py --mesh) or --skeleton synthetic")
        if jointstype:
            raise SystemExit("--jointstype needs --skeleton BODY.npz (tools/make_skeleton.py --mesh with the joint regressors) or --skeleton synthetic")
        return False
    from ..model.rotation2xyz import load_skeleton_or_body
    if args.skeleton == "synthetic":
        sk = synth.make_body(model.njoints - 1) if vertices or jointstype else synth.make_skeleton(model.njoints - 1)
        if jointstype:
            sk["mesh"].update(synth.make_joint_regressors(sk))
        print(f"--skeleton synthetic: a synthetic {model.njoints - 1}-joint tree (synth.make_skeleton), not a body model's skeleton"
              + (f", under a synthetic {sk['mesh']['v_template'].shape[0]}-vertex surface (synth.make_body)" if vertices or jointstype else "")
              + (", with synthetic vertex joints, regressor and joint maps (synth.make_joint_regressors)" if jointstype else ""))
    else:
        sk = load_skeleton_or_body(args.skeleton)
    if vertices and sk.get("mesh", None) is None:
        raise SystemExit(f"--vertices: {args.skeleton} is a skeleton file without mesh arrays (write a body file with tools/make_skeleton.py --mesh)")
    if jointstype and (sk.get("mesh", None) is None or sk["mesh"].get("vertex_joints", None) is None or jointstype not in sk["mesh"]["joint_maps"]):
        raise SystemExit(f"--jointstype {jointstype}: {args.skeleton} holds no joint regressors (vertex_joints / J_regressor_extra) or no map_{jointstype} "
                         f"(write a body file with tools/make_skeleton.py --mesh --vertex_joints ... --joint_regressor_extra ... --joint_maps ...)")
    model.set_skeleton(sk)
    return True


def load_betas(args, n, nb):
    """--betas_npz FILE | synthetic -> fp32 [N, nb'] body shapes, one per generated sample (None without the option). `synthetic`: `n` seeded
    N(0, 1) shapes over the skeleton's `nb` directions."""
    if not getattr(args, "betas_npz", ""):
        return None
    if not args.skeleton:
        raise SystemExit("--betas_npz shapes the joints and meshes of --skeleton: give one")
    if args.betas_npz == "synthetic":
        return np.random.Generator(np.random.PCG64(args.seed)).standard_normal((n, nb)).astype(np.float32)
    with np.load(args.betas_npz, allow_pickle=False) as z:
        if "betas" not in z.files:
            raise SystemExit(f"--betas_npz: {args.betas_npz} holds no 'betas'")
        betas = np.ascontiguousarray(z["betas"], dtype=np.float32)
    if betas.ndim != 2 or not len(betas) or not 1 <= betas.shape[1] <= nb:
        raise SystemExit(f"--betas_npz: 'betas' {betas.shape} is not [N, nb] with 1 <= nb <= {nb} (the skeleton file's shape directions)")
    return betas


def joint_positions(model, args, sample, y, jointstype=None, betas=None):
    """The reference's closing call (cgenerate.py:154-158) on this model's rot2xyz: [B, njoints, nfeats, T] -> [B, J, 3, T]; betas [B, nb]: a body
    shape per motion (--betas_npz)."""
    pose_rep = "xyz" if model.data_rep in ("xyz", "hml_vec") else model.data_rep
    mask = None if pose_rep == "xyz" else y["mask"].reshape(sample.shape[0], sample.shape[-1]).bool()
    shapes = {} if betas is None or pose_rep == "xyz" else {"betas_per_motion": torch.from_numpy(np.ascontiguousarray(betas))}
    jointstype = jointstype or getattr(args, "jointstype", "") or args.body_model
    return model.rot2xyz(x=sample, mask=mask, pose_rep=pose_rep, glob=True, translation=True, jointstype=jointstype, vertstrans=True,
                         num_person=1, betas=None, beta=0, glob_rot=None, get_rotations_back=False, **shapes)


def motion_rows(model, args):
    """Rows of 'motion': the skeleton's joints, or with --jointstype the entries of that type's map."""
    jointstype = getattr(args, "jointstype", "")
    return len(model.rot2xyz.mesh["joint_maps"][jointstype]) if jointstype else model.njoints - 1


def vertex_positions(model, args, sample, y, betas=None):
    """... and the call the reference's mesh export makes (visualize/vis_utils.py:35-41): jointstype='vertices' -> [B, V, 3, T]."""
    return joint_positions(model, args, sample, y, jointstype="vertices", betas=betas)


def mesh_results(model, args, all_vertices, lengths):
    """The 'vertices' / 'faces' entries of results.npy; --obj_dir: the OBJ sequences beside them; --render_dir: the rendered frames."""
    from ..utils.mesh_io import write_obj_sequences, write_png_sequences
    verts, faces = np.concatenate(all_vertices), model.rot2xyz.mesh["faces"]
    if args.obj_dir:
        n = write_obj_sequences(args.obj_dir, verts, faces, lengths)
        print(f"wrote {n} OBJ files under [{os.path.abspath(args.obj_dir)}]")
    if getattr(args, "render_dir", ""):                 # one motion at a time: a motion's frames are 3 W H T bytes
        from ..utils.render import MeshRenderer
        renderer, n = MeshRenderer(faces, next(model.parameters()).device), 0
        for i in range(len(verts)):
            frames = renderer.render(torch.from_numpy(verts[i:i + 1]), width=args.render_size, height=args.render_size)
            n += write_png_sequences(args.render_dir, frames.cpu().numpy(), lengths[i:i + 1], first=i)
        renderer.close()
        print(f"wrote {n} PNG files under [{os.path.abspath(args.render_dir)}]")
    return {"vertices": verts, "faces": faces}


def main(argv=None):
    """Single process: one GPU samples `num_samples` motions per repetition. Under torchrun
    (`python -m torch.distributed.run --nproc-per-node N -m regennet_amd.sample.cgenerate ...`): the `num_samples` of every
    repetition are sharded over the N ranks (contiguous shards, `dist_util.shard_bounds`), rank 0's checkpoint is
    broadcast once over RCCL (`dist_util.sync_model_weights`: one flat fp32 buffer), every rank samples its shard with the Philox stream keyed by the GLOBAL sample index (so the
    result does not depend on N), and rank 0 gathers and saves. No collective inside the sampling loop."""
    args = cgenerate_args(argv)
    fixseed(args.seed)
    hml = args.dataset in HML_DATASETS
    max_frames = HML_MAX_FRAMES if hml else 150 if args.dataset == "chi3d" else 60
    n_frames = min(max_frames, int(args.motion_length))
    hml_mean, hml_std = hml_statistics(args) if hml else (None, None)
    dev = dist_util.setup_dist()
    rank, world = dist_util.world()
    assert args.num_samples <= args.batch_size, \
        f"Please either increase batch_size({args.batch_size}) or reduce num_samples({args.num_samples})"
    args.batch_size = args.num_samples
    cfg = dataset_config(args)
    data = types.SimpleNamespace(dataset=types.SimpleNamespace(num_actions=cfg["num_actions"], num_person=2))
    if rank == 0:
        print("Creating model and diffusion...")
    if args.arch == "gru":     # (--gru_scan reaches the model through get_model_args)
        model, diffusion = create_model_and_diffusion(args, data, allow_gru=True)
    else:
        model, diffusion = create_model_and_diffusion(args, data, allow_mlp=True)
    model.precision = args.precision
    if args.synthetic or not args.model_path:
        # rank 0 owns "the checkpoint"; other ranks start from different values and receive rank 0's through the start-up broadcast
        sd = {k: torch.from_numpy(v) for k, v in
              synth.make_state_dict(model.engine_config() | {"layers": model.num_layers}, seed=0 if rank == 0 else 1000 + rank).items()}
    else:
        if rank == 0:
            print(f"Loading checkpoints from [{args.model_path}]...")
        sd = torch.load(args.model_path, map_location="cpu")
    load_model_wo_clip(model, sd)
    if args.guidance_param != 1:
        model = ClassifierFreeSampleModel(model)
    model.to(dev)
    model.eval()
    dist_util.sync_model_weights(model, 0)                  # THE collective of the run's start-up (none in a single process)
    clips, actions = _load_clips(args, cfg, args.num_samples)
    assert clips.shape[1:3] == (cfg["njoints"], cfg["nfeats"]) and clips.shape[3] >= n_frames, \
        f"actor clips {clips.shape} do not cover [N, {cfg['njoints']}, {cfg['nfeats']}, {n_frames}]"
    clips = clips[..., :n_frames]                           # --motion_length shorter than the dataset length (cgenerate.py:40,126)
    B = args.batch_size
    lo, hi = dist_util.shard_bounds(B)                      # this rank's samples of every repetition
    Bl = hi - lo
    sample_fn = diffusion.p_sample_loop if not args.use_ddim else diffusion.ddim_sample_loop
    inner = model.model if isinstance(model, ClassifierFreeSampleModel) else model
    eng, _ = inner._get_engine(max(Bl, 1), n_frames)
    with_motion = hml or set_skeleton(inner, args)
    with_vertices = with_motion and args.vertices
    texts = load_text_features(args, args.num_samples, inner.clip_dim) if inner.cond_mode == "text" else None
    if hml:
        from ..utils.hml import hml_to_joints, joints_of
    nverts = inner.rot2xyz.mesh["v_template"].shape[0] if with_vertices else 0
    shapes = load_betas(args, args.num_samples, inner.rot2xyz.num_betas if with_motion and not hml else 0)     # [N, nb] | None: cycled like the actor clips
    all_outputs, all_cmotions, all_motions, all_vertices, all_betas, time_all = [], [], [], [], [], 0.0
    shape = (Bl, inner.njoints, inner.nfeats, n_frames)

    def make_y(rep_i):
        idx = (np.arange(lo, hi) + rep_i * B) % len(clips)
        y = {"cmotion": torch.from_numpy(np.ascontiguousarray(clips[idx])).to(dev), "lengths": torch.full((Bl,), n_frames),
             "mask": torch.ones(Bl, 1, 1, n_frames, dtype=torch.bool)}
        if inner.cond_mode == "action":
            y["action"] = torch.from_numpy(actions[idx]).to(dev)
        if inner.cond_mode == "text":
            y["text_features"] = torch.from_numpy(np.ascontiguousarray(texts[(np.arange(lo, hi) + rep_i * B) % len(texts)])).to(dev)
        if args.guidance_param != 1:
            y["scale"] = torch.ones(Bl, device=dev) * args.guidance_param
        return y

    if world > 1:
        # one precision-schedule switch point for all ranks (x3_tail="auto": measured on the loaded checkpoint), agreed HERE, where every
        # rank passes whatever its shard - a rank with no samples contributes 0 and still takes part in the all-reduce
        diffusion.agree_x3_tail(model, shape, {"y": make_y(0)} if Bl > 0 else None, sampler="ddim" if args.use_ddim else "ddpm")
    for rep_i in range(args.num_repetitions):
        if rank == 0:
            print(f"### Sampling [repetitions #{rep_i}]")
        y = make_y(rep_i)
        dist_util.synchronize()
        t_start = time.time()
        if Bl > 0:
            sample = sample_fn(model, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=0, init_image=None,
                               progress=(rank == 0), dump_steps=None, noise=None, const_noise=False,
                               seed=args.seed * 1000003 + rep_i, sample_offset=rep_i * B + lo)
            smooth = torch.empty_like(sample)      # scipy.ndimage.gaussian_filter1d(sigma=1, axis=-1) on the device (cgenerate.py:142)
            eng.gaussian_filter1d(sample.contiguous(), smooth, sample.numel() // n_frames, n_frames, 1.0, dist_util.stream_handle(dev))
        else:
            smooth = torch.empty(shape, device=dev)
        dist_util.synchronize()
        t_end = time.time()
        if rep_i >= 1:
            time_all += (t_end - t_start) * 1000
        if rank == 0:
            print("Generating time consumption: %s ms" % ((t_end - t_start) * 1000))
        all_outputs.append(dist_util.all_gather_samples(smooth, B).cpu().numpy())
        all_cmotions.append(dist_util.all_gather_samples(y["cmotion"], B).cpu().numpy())
        betas = None
        if shapes is not None:                     # sample i of this repetition wears shape (i + rep_i B) mod N
            all_betas.append(shapes[(np.arange(B) + rep_i * B) % len(shapes)])
            betas = all_betas[-1][lo:hi]
        if hml:                                    # cgenerate.py:147-152: inv_transform + recover_from_ric of the smoothed sample, one launch
            motion = hml_to_joints(smooth, hml_mean, hml_std, engine=eng) if Bl > 0 else torch.empty((0, joints_of(inner.njoints), 3, n_frames), device=dev)
            all_motions.append(dist_util.all_gather_samples(motion, B).cpu().numpy())
        elif with_motion:                          # after the timed region, from the smoothed sample, like the reference (cgenerate.py:142-163)
            motion = joint_positions(inner, args, smooth, y, betas=betas) if Bl > 0 else torch.empty((0, motion_rows(inner, args), 3, n_frames), device=dev)
            all_motions.append(dist_util.all_gather_samples(motion, B).cpu().numpy())
        if with_vertices:
            verts = vertex_positions(inner, args, smooth, y, betas=betas) if Bl > 0 else torch.empty((0, nverts, 3, n_frames), device=dev)
            all_vertices.append(dist_util.all_gather_samples(verts, B).cpu().numpy())
        if rank == 0:
            print(f"created {len(all_outputs) * B} samples")
    npy_path = None
    if rank == 0:
        if args.num_repetitions != 1:
            print("Average Time Consumption: %s ms" % (time_all / (args.num_repetitions - 1)))
        out_path = args.output_dir or os.path.join(os.path.dirname(args.model_path) or ".", f"samples_seed{args.seed}")
        os.makedirs(out_path, exist_ok=True)
        npy_path = os.path.join(out_path, "results.npy")
        print(f"saving results file to [{npy_path}]")
        np.save(npy_path, {**({"motion": np.concatenate(all_motions)} if with_motion else {}),
                           **({"betas": np.concatenate(all_betas)} if all_betas else {}),
                           **(mesh_results(inner, args, all_vertices, np.full((len(all_outputs) * B,), n_frames)) if with_vertices else {}),
                           "output": np.concatenate(all_outputs), "cmotion": np.concatenate(all_cmotions),
                           "lengths": np.full((len(all_outputs) * B,), n_frames), "num_samples": args.num_samples,
                           "num_repetitions": args.num_repetitions, "world_size": world})
        print(f"[Done] Results are at [{os.path.abspath(out_path)}]")
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    return npy_path


if __name__ == "__main__":
    main()
