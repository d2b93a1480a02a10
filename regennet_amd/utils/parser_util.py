"""Flag subset of the reference's `utils/parser_util.py` that the sampling hot path reads:
base (:90-98), diffusion (:100-106), model (:109-139), dataset (:142-153), sampling (:190-204), generate
(:207-220). As in the reference, for sampling the `model`/`diffusion` groups are overwritten from `args.json`
beside the checkpoint (parse_and_load_from_model_wo_data :40-70) and guidance is disabled when the model was
trained without condition masking (:68-69). `type=bool` flags keep the reference's (quirky) semantics: any
non-empty string is True."""
import argparse
import json
import os


def add_base_options(p):
    g = p.add_argument_group("base")
    g.add_argument("--cuda", default=True, type=bool)
    g.add_argument("--device", default=0, type=int)
    g.add_argument("--seed", default=10, type=int)
    g.add_argument("--batch_size", default=64, type=int)
    g.add_argument("--use_ddim", action="store_true")
    g.add_argument("--timestep_respacing", default="", type=str)


def add_diffusion_options(p):
    g = p.add_argument_group("diffusion")
    g.add_argument("--noise_schedule", default="cosine", choices=["linear", "cosine"], type=str)
    g.add_argument("--diffusion_steps", default=1000, type=int)   # ignored, like the reference (model_util.py:78)
    g.add_argument("--sigma_small", default=True, type=bool)


def add_model_options(p):
    g = p.add_argument_group("model")
    g.add_argument("--setting", default="cmdm", choices=["mdm", "cmdm"], type=str)
    g.add_argument("--arch", default="online", choices=["trans_enc", "trans_dec", "gru", "mlp", "online", "offline"], type=str)
    g.add_argument("--gru_scan", default="batch", choices=["batch", "frames"], type=str,
                   help="arch='gru' only: the axis the GRU scans. batch (default) is the reference's own recurrence over the samples of a call, so a "
                        "motion depends on the samples before it in its batch; frames is a recurrence over each motion's frames.")
    g.add_argument("--emb_trans_dec", default=False, type=bool)
    g.add_argument("--wo_pos_emb", action="store_true")
    g.add_argument("--cm_mode", default="concat", choices=["concat", "add"], type=str)
    g.add_argument("--layers", default=8, type=int)
    g.add_argument("--latent_dim", default=512, type=int)
    g.add_argument("--cond_mask_prob", default=0.1, type=float)
    g.add_argument("--unconstrained", action="store_true")
    for name in ("lambda_rcxyz", "lambda_vel", "lambda_fc", "lambda_orient", "lambda_body", "lambda_transl"):
        g.add_argument("--" + name, default=0.0, type=float)
    g.add_argument("--vel_threshold", default=0.01, type=float)


def add_data_options(p):
    g = p.add_argument_group("dataset")
    g.add_argument("--dataset", default="ntu", choices=["ntu", "chi3d", "humanml", "kit"], type=str,
                   help="humanml / kit: the 263 / 251-row feature vector (data_rep='hml_vec', text-conditioned, up to 196 frames); 'motion' is "
                        "recover_from_ric of the sample")
    g.add_argument("--hml_stats", default="", type=str,
                   help="humanml / kit: the dataset's Mean / Std - an npz with 'mean' and 'std' [D], or a directory holding Mean.npy / Std.npy; "
                        "without it the features are taken as already de-normalised")
    g.add_argument("--data_path", default="", type=str)
    g.add_argument("--num_person", default=2, type=int)
    g.add_argument("--pose_rep", default="rot6d", type=str)
    g.add_argument("--body_model", default="smplx", type=str)


def add_sampling_options(p):
    g = p.add_argument_group("sampling")
    g.add_argument("--model_path", default="", type=str, help="model####.pt (args.json is read from the same directory)")
    g.add_argument("--output_dir", default="", type=str)
    g.add_argument("--num_samples", default=10, type=int)
    g.add_argument("--num_repetitions", default=3, type=int)
    g.add_argument("--guidance_param", default=2.5, type=float)


def add_generate_options(p):
    g = p.add_argument_group("generate")
    g.add_argument("--motion_length", default=60, type=float)
    g.add_argument("--action_file", default="", type=str)
    g.add_argument("--action_name", default="", type=str)
    # inputs the reference takes from its (licence-restricted) h5 datasets; here an .npz or synthetic data
    g.add_argument("--cmotion_npz", default="", type=str, help="npz with 'cmotion' [N,56,6,T] (+ 'action' [N]) actor clips")
    g.add_argument("--synthetic", action="store_true", help="synthetic checkpoint + actor motions (+ text features) (no assets needed)")
    g.add_argument("--text_features", default="", type=str,
                   help="text-conditioned models: npy [N, clip_dim] of text features for y['text_features'] (the CLIP tower is out of scope), cycled "
                        "over repetitions like the actor clips")
    g.add_argument("--skeleton", default="", type=str,
                   help="skeleton npz (tools/make_skeleton.py) or 'synthetic': also store 'motion', the joint positions model.rot2xyz gives")
    g.add_argument("--vertices", action="store_true",
                   help="also store 'vertices' [N,V,3,T] and 'faces': needs a --skeleton with mesh arrays (tools/make_skeleton.py --mesh; 'synthetic': synth.make_body)")
    g.add_argument("--jointstype", default="", choices=["", "vibe", "a2m", "a2mpl"], type=str,
                   help="'motion' holds this joint type (regressed from the mesh) instead of the skeleton's joints: needs a --skeleton body file with "
                        "vertex_joints / J_regressor_extra and the type's map (tools/make_skeleton.py --mesh --joint_maps ...; 'synthetic': "
                        "synth.make_joint_regressors)")
    g.add_argument("--betas_npz", default="", type=str,
                   help="with --skeleton: npz with 'betas' [N,nb], the reactor's body shape per generated sample (cycled over repetitions like the actor "
                        "clips), for 'motion' and 'vertices'; 'synthetic': seeded N(0,1) shapes; results.npy stores 'betas'")
    g.add_argument("--obj_dir", default="", type=str, help="with --vertices: write DIR/sample{i:02d}/frame{t:03d}.obj")
    g.add_argument("--render_dir", default="", type=str, help="with --vertices: render the meshes on the device and write DIR/sample{i:02d}/frame{t:03d}.png")
    g.add_argument("--render_size", default=1024, type=int, help="with --render_dir: width and height of the frames (render/crendermotion.py:109-110: 1024)")
    g.add_argument("--precision", default="bf16_x3tail", choices=["f32", "bf16x3", "bf16", "bf16_x3tail"], type=str)


def add_edit_options(p):
    """parser_util.py:223-237 (names and defaults), with 'rows' / --keep_rows in place of the HumanML3D-only 'upper_body' and the
    inputs this CLI takes instead of a dataset."""
    g = p.add_argument_group("edit")
    g.add_argument("--edit_mode", default="in_between", choices=["in_between", "upper_body", "rows"], type=str,
                   help="in_between: keep the frames outside [prefix_end, suffix_start); rows: keep the pose rows of --keep_rows in every frame; "
                        "upper_body (--dataset humanml): keep the lower-body rows of the feature vector, generate the upper body")
    g.add_argument("--prefix_end", default=0.25, type=float, help="in_between: end of the kept prefix, as a fraction of the length")
    g.add_argument("--suffix_start", default=0.75, type=float, help="in_between: start of the kept suffix, as a fraction of the length")
    g.add_argument("--keep_rows", default="", type=str, help="rows: pose rows to keep, e.g. 0-21,55")
    g.add_argument("--input_motions", default="", type=str, help=".npy [N, njoints, nfeats, T]: the motions to edit (--synthetic: synthetic ones)")


def add_score_options(p):
    """regennet_amd.eval.score: the grid of timesteps and where the table goes (the weights are the model group's lambda_* / --vel_threshold)."""
    g = p.add_argument_group("score")
    g.add_argument("--t_grid", default=10, type=int, help="score every motion at this many evenly spaced timesteps of the (respaced) schedule")
    g.add_argument("--bpd", action="store_true",
                   help="score with the variational bound in bits per dimension over the WHOLE (respaced) schedule (diffusion.calc_bpd_loop) instead of "
                        "the training terms; the table shows --t_grid of its timesteps, scores.npy holds all of them. Needs no skeleton.")


def _group_keys(parser, args, title):
    for grp in parser._action_groups:
        if grp.title == title:
            return [a.dest for a in grp._group_actions]
    raise ValueError("group_name was not found.")


def cgenerate_args(argv=None, edit=False, score=False):
    p = argparse.ArgumentParser()
    add_base_options(p)
    add_data_options(p)
    add_sampling_options(p)
    add_generate_options(p)
    add_model_options(p)
    add_diffusion_options(p)
    if edit:
        add_edit_options(p)
    if score:
        add_score_options(p)
    args = p.parse_args(argv)
    if args.model_path:
        args_path = os.path.join(os.path.dirname(args.model_path), "args.json")
        assert os.path.exists(args_path), "Arguments json file was not found!"
        with open(args_path) as fr:
            model_args = json.load(fr)
        for key in _group_keys(p, args, "model") + _group_keys(p, args, "diffusion"):
            if key in model_args:
                setattr(args, key, model_args[key])
            elif "cond_mode" in model_args:
                setattr(args, "unconstrained", model_args["cond_mode"] == "no_cond")
            else:
                print(f"Warning: was not able to load [{key}], using default value [{getattr(args, key)}] instead.")
    if args.cond_mask_prob == 0:
        args.guidance_param = 1
    return args


def edit_args(argv=None):
    """The reference's edit_args (parser_util.py:259-264) on this CLI's flag set: cgenerate's groups + the edit group."""
    return cgenerate_args(argv, edit=True)


LOSS_FLAGS = ("lambda_rcxyz", "lambda_vel", "lambda_fc", "lambda_orient", "lambda_body", "lambda_transl", "vel_threshold")


def score_args(argv=None):
    """cgenerate's flag set + the score group. The weights of the objective come from args.json beside --model_path (what the checkpoint was
    trained with); without one orient, body and transl stand at 1 like the reference's training defaults (parser_util.py:131-136). A weight
    given on the command line wins over both."""
    args = cgenerate_args(argv, score=True)
    if not args.model_path:
        args.lambda_orient = args.lambda_body = args.lambda_transl = 1.0
    given = argparse.ArgumentParser(add_help=False, argument_default=argparse.SUPPRESS)
    for name in LOSS_FLAGS:
        given.add_argument("--" + name, type=float)
    for k, v in vars(given.parse_known_args(argv)[0]).items():
        setattr(args, k, v)
    if args.t_grid < 1:
        raise SystemExit("--t_grid must be at least 1")
    return args
