"""`python -m regennet_amd.sample.hml_joints --data_path results.npy [--hml_stats PATH] --out FILE.npy` - joint positions of stored HumanML3D / KIT
samples without a checkpoint: reads 'output' [N, 263 | 251, 1, T] of a results file (cgenerate / edit with --dataset humanml | kit, or a bare array),
de-normalises it with the dataset's Mean / Std when --hml_stats is given, and writes what the reference's cgenerate.py:147-152 forms, fp32
[N, 22 | 21, 3, T] - one launch of rgn_hml_to_joints per `--batch_size` motions, on the handle sample/render.py's postprocessing_engine provides."""
import argparse
import os

import numpy as np
import torch

from ..utils.hml import hml_to_joints, joints_of, load_hml_stats
from .render import postprocessing_engine


def load_output(path):
    d = np.load(path, allow_pickle=True)
    d = d.item() if d.dtype == object else {"output": d}
    if "output" not in d:
        raise SystemExit(f"{path} holds no 'output'")
    out = np.ascontiguousarray(d["output"], dtype=np.float32)
    if out.ndim != 4 or out.shape[2] != 1:
        raise SystemExit(f"'output' {out.shape} of {path} is not [N, D, 1, T], the layout of a data_rep='hml_vec' model")
    try:
        joints_of(out.shape[1])
    except ValueError as e:
        raise SystemExit(f"{path}: {e}")
    return out


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--data_path", required=True, help="results.npy of cgenerate / edit --dataset humanml | kit (or an array [N, D, 1, T])")
    p.add_argument("--hml_stats", default="", help="npz with 'mean' and 'std' [D], or a directory holding Mean.npy / Std.npy; without it the "
                                                   "features are taken as already de-normalised")
    p.add_argument("--out", default="", help="default: hml_joints.npy beside the data file")
    p.add_argument("--batch_size", default=256, type=int)
    p.add_argument("--device", default=0, type=int)
    args = p.parse_args(argv)
    x = load_output(args.data_path)
    mean = std = None
    if args.hml_stats:
        mean, std = load_hml_stats(args.hml_stats)
        if len(mean) != x.shape[1]:
            raise SystemExit(f"--hml_stats: {args.hml_stats} holds {len(mean)} rows, 'output' has {x.shape[1]}")
    else:
        print("no --hml_stats: the features are taken as already de-normalised (the dataset's Mean / Std are not applied)")
    dev = torch.device("cuda", args.device)
    model, eng = postprocessing_engine(dev)
    step = max(1, args.batch_size)
    xyz = [hml_to_joints(torch.from_numpy(x[i:i + step]).to(dev), mean, std, engine=eng).cpu().numpy() for i in range(0, len(x), step)]
    xyz = np.concatenate(xyz) if xyz else np.zeros((0, joints_of(x.shape[1]), 3, x.shape[3]), np.float32)
    out = args.out or os.path.join(os.path.dirname(os.path.abspath(args.data_path)), "hml_joints.npy")
    np.save(out, xyz)
    print(f"wrote joint positions {xyz.shape} to [{out}]")
    return out


if __name__ == "__main__":
    main()
