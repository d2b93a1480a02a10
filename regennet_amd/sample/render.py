"""`python -m regennet_amd.sample.render` - counterpart of the reference's `python -m render.crendermotion --data_path results.npy --num_person 2
--setting cmdm --body_model smplx` (render/crendermotion.py:52-128): read a results file, put actor and reactor side by side (:78), smooth with the
sigma = 3 temporal Gaussian (:79), pose the meshes (jointstype='vertices', num_person persons, vertstrans; :61-68, :87), centre on the first
frame and render every frame (:20-31), crop the motion's frames to their content (:33-41) and write them out.

Everything between the file and the PNGs runs on the device: rgn_gaussian_filter1d, rgn_rot2verts, rgn_render. The reference takes the body from
its licensed SMPL / SMPL-X files; here `--skeleton BODY.npz` is a body file of tools/make_skeleton.py --mesh (`synthetic`: synth.make_body, not
a body model). Frames are written as OUT/sample{i:02d}/frame{t:03d}.png; OUT/sample{i:02d}.mp4 is written as well where `imageio` can be
imported (the reference's only output, :21, 40-42)."""
import argparse
import os

import numpy as np
import torch

from .. import synth
from ..model.rotation2xyz import Rotation2xyz, load_skeleton_or_body
from ..utils import dist_util
from ..utils.mesh_io import write_png_sequences
from ..utils.render import DEFAULT_CAM, MeshRenderer, crop_to_content


def load_results(path, num_person):
    """The dict `cgenerate` saves (and the layout crendermotion.py:74-78 reads: 'cmotion', 'output', optional 'text') -> (x fp32
    [N, rows, feats * num_person, T], texts)."""
    d = np.load(path, allow_pickle=True)
    d = d.item() if d.dtype == object else {"output": d}
    out = np.asarray(d["output"], dtype=np.float32)
    if num_person == 2:
        if "cmotion" not in d:
            raise SystemExit(f"--num_person 2 needs 'cmotion' beside 'output' in {path}")
        out = np.concatenate((np.asarray(d["cmotion"], dtype=np.float32), out), axis=2)          # actor first (:78)
    elif num_person != 1:
        raise SystemExit("--num_person: 1 (the reactor alone) or 2 (actor and reactor)")
    texts = [str(t) for t in d["text"]] if "text" in d else [""] * len(out)
    return out, texts


def load_betas(spec, n, nb, num_person, seed=0):
    """--betas_npz FILE | synthetic -> fp32 [N, num_person, nb'] (None without the option). The file's 'betas' is [N, 2, nb], actor then reactor;
    one person is the reactor alone, like 'output'. `synthetic`: `n` seeded N(0, 1) pairs over the body's `nb` directions."""
    if not spec:
        return None
    if spec == "synthetic":
        betas = np.random.Generator(np.random.PCG64(seed)).standard_normal((n, 2, nb)).astype(np.float32)
    else:
        with np.load(spec, allow_pickle=False) as z:
            if "betas" not in z.files:
                raise SystemExit(f"--betas_npz: {spec} holds no 'betas'")
            betas = np.ascontiguousarray(z["betas"], dtype=np.float32)
        if betas.ndim != 3 or not len(betas) or betas.shape[1] != 2 or not 1 <= betas.shape[2] <= nb:
            raise SystemExit(f"--betas_npz: 'betas' {betas.shape} is not [N, 2, nb] (actor, reactor) with 1 <= nb <= {nb} (the body file's shape directions)")
    return np.ascontiguousarray(betas[:, 2 - num_person:])


def write_mp4(path, frames, fps=30):
    """Only where imageio is there (crendermotion.py:21, 40-42); returns whether it wrote."""
    try:
        import imageio
    except ImportError:
        return False
    with imageio.get_writer(path, fps=fps) as w:
        for f in frames:
            w.append_data(f)
    return True


def postprocessing_engine(dev):
    """(model, engine) for the two post-processing entry points this script needs and no denoiser: rgn_gaussian_filter1d takes an rgn_handle
    with finalized weights, and Rotation2xyz takes its device from a model. Neither reads the weights, so the smallest synthetic configuration
    is built for them, here and nowhere else (the coupling, and what would remove it)."""
    cfg = synth.get_config("tiny")
    model, _ = synth.build_model(cfg, synth.make_state_dict(cfg, seed=0), resp="10", precision="f32", device=str(dev))
    eng, _ = model._get_engine(1, cfg["num_frames"])
    return model, eng


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--data_path", required=True, help="results.npy of cgenerate (or a dict with 'cmotion', 'output', 'text' as the reference saves it)")
    p.add_argument("--skeleton", required=True, help="body file (tools/make_skeleton.py --mesh) or 'synthetic'")
    p.add_argument("--num_person", default=2, type=int)
    p.add_argument("--setting", default="mdm", choices=["mdm", "cmdm"], help="cmdm: the second person in grey (renderer.py:86-89)")
    p.add_argument("--out", default="", help="default: 'rendered' beside the data file (crendermotion.py:115)")
    p.add_argument("--size", default=1024, type=int, help="width and height (crendermotion.py:109-110)")
    p.add_argument("--sigma", default=3.0, type=float, help="temporal smoothing (crendermotion.py:79); 0: none")
    p.add_argument("--betas_npz", default="", help="npz with 'betas' [N, 2, nb]: the body shape of actor and reactor per sample (cycled); "
                                                   "'synthetic': seeded N(0, 1) shapes")
    p.add_argument("--no_crop", action="store_true")
    p.add_argument("--device", default=0, type=int)
    args = p.parse_args(argv)
    dev = torch.device("cuda", args.device)
    x, texts = load_results(args.data_path, args.num_person)
    N, R, _, T = x.shape
    body = synth.make_body(R - 1) if args.skeleton == "synthetic" else load_skeleton_or_body(args.skeleton)
    if body.get("mesh", None) is None:
        raise SystemExit(f"{args.skeleton} is a skeleton file without mesh arrays (write a body file with tools/make_skeleton.py --mesh)")
    model, eng = postprocessing_engine(dev)
    rot2xyz = Rotation2xyz(body, model)
    betas = load_betas(args.betas_npz, N, rot2xyz.num_betas, args.num_person)
    renderer = MeshRenderer(body["mesh"]["faces"], dev)
    out_dir = args.out or os.path.join(os.path.dirname(os.path.abspath(args.data_path)), "rendered")
    n_png = n_mp4 = 0
    for i in range(N):
        xi = torch.from_numpy(np.ascontiguousarray(x[i:i + 1])).to(dev)
        if args.sigma > 0:
            sm = torch.empty_like(xi)
            eng.gaussian_filter1d(xi, sm, xi.numel() // T, T, float(args.sigma), dist_util.stream_handle(dev))
            xi = sm
        verts = rot2xyz(xi, torch.ones((1, T), dtype=torch.bool), pose_rep="rot6d", translation=True, glob=True, jointstype="vertices", vertstrans=True,
                        num_person=args.num_person, glob_rot=[3.141592653589793, 0, 0],
                        **({} if betas is None else {"betas_per_motion": torch.from_numpy(betas[i % len(betas)][None])}))
        frames = renderer.render(verts, width=args.size, height=args.size, cam=DEFAULT_CAM, setting=args.setting, center=True)[0]
        box = None if args.no_crop else crop_to_content(frames)
        if box is not None:
            frames = frames[:, box[0]:box[2], box[1]:box[3]]
        frames = frames.cpu().numpy()
        n_png += write_png_sequences(out_dir, frames[None], first=i)
        n_mp4 += write_mp4(os.path.join(out_dir, "sample%02d.mp4" % i), frames)
        print(f"sample {i}{' (' + texts[i] + ')' if texts[i] else ''}: {len(frames)} frames of {frames.shape[2]} x {frames.shape[1]}")
    renderer.close()
    print(f"wrote {n_png} PNG files" + (f" and {n_mp4} mp4 files" if n_mp4 else "") + f" under [{out_dir}]")
    return out_dir


if __name__ == "__main__":
    main()
