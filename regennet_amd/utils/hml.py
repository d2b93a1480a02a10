"""Joint positions of HumanML3D / KIT feature vectors on the device: the reference's closing step for data_rep='hml_vec' models
(sample/cgenerate.py:147-152: t2m_dataset.inv_transform, then data_loaders/humanml/scripts/motion_process.py recover_from_ric), one launch of
rgn_hml_to_joints (csrc/rgn_hml.hip) on the sample's own layout.

  hml_to_joints(sample, mean, std, engine)    [B, D, 1, T] in the model's layout -> [B, J, 3, T]
  recover_from_ric(data, joints_num)          the reference's signature and layouts: [..., T, D] -> [..., T, J, 3]
  load_hml_stats(path)                        Mean / Std of the dataset, from an .npz or the dataset's own directory

No CPU fallback: tensors on another device are refused. tests/hml_ref.py restates the arithmetic in fp64."""
import os

import numpy as np
import torch

from . import dist_util

_ENGINES = {}          # device -> (model, engine) of sample.render.postprocessing_engine, for callers that hold no engine of their own


def joints_of(D):
    """Joints of a feature vector of D = 12 J - 1 rows: 22 for HumanML3D's 263, 21 for KIT's 251 (cgenerate.py:149)."""
    D = int(D)
    if D < 23 or (D + 1) % 12:
        raise ValueError(f"{D} rows are no HumanML3D / KIT feature vector (12 J - 1 rows: 263 for 22 joints, 251 for 21)")
    return (D + 1) // 12


def default_engine(device):
    """The handle sample/render.py's postprocessing_engine provides for entry points that read no weights; one per device, kept."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _ENGINES:
        from ..sample.render import postprocessing_engine
        _ENGINES[key] = postprocessing_engine(torch.device(*key))
    return _ENGINES[key][1]


def hml_to_joints(sample, mean=None, std=None, engine=None):
    """sample fp32 [B, D, 1, T] on the device (the model's layout, as the sampling loop returns it), mean / std [D] (tensors or arrays; both or
    neither: without them the features are taken as already de-normalised) -> joint positions fp32 [B, J, 3, T] on the device, what
    cgenerate.py:150-152 forms. engine: any engine of this device (a model's, or default_engine's when None)."""
    if not isinstance(sample, torch.Tensor) or sample.device.type != "cuda":
        raise RuntimeError("hml_to_joints runs on an AMD GPU only: pass a tensor on the device (there is no CPU fallback; tests/hml_ref.py restates it)")
    if sample.dim() != 4 or sample.shape[2] != 1:
        raise ValueError(f"sample {tuple(sample.shape)} is not [B, D, 1, T], the layout of a data_rep='hml_vec' model")
    if (mean is None) != (std is None):
        raise ValueError("mean and std go together: both given or both None")
    B, D, _, T = sample.shape
    J = joints_of(D)
    dev = sample.device
    x = sample.detach().to(torch.float32).contiguous()
    stats = [None if s is None else torch.as_tensor(np.asarray(s) if not isinstance(s, torch.Tensor) else s).to(dev, torch.float32).reshape(-1).contiguous()
             for s in (mean, std)]
    if stats[0] is not None and (stats[0].numel() != D or stats[1].numel() != D):
        raise ValueError(f"mean / std of {stats[0].numel()} / {stats[1].numel()} entries for a sample of {D} rows")
    xyz = torch.empty((B, J, 3, T), dtype=torch.float32, device=dev)
    (engine or default_engine(dev)).hml_to_joints(x, stats[0], stats[1], J, xyz, dist_util.stream_handle(dev))
    return xyz


def recover_from_ric(data, joints_num, engine=None):
    """The reference's recover_from_ric (motion_process.py:415-430) with its signature and layouts: data [..., T, D] of de-normalised features on the
    device, any leading dimensions -> positions [..., T, joints_num, 3]."""
    if data.dim() < 2:
        raise ValueError(f"data {tuple(data.shape)} is not [..., T, D]")
    T, D = data.shape[-2:]
    if joints_of(D) != int(joints_num):
        raise ValueError(f"joints_num = {joints_num} for {D} rows: 12 J - 1 rows hold J = {joints_of(D)} joints")
    lead = tuple(data.shape[:-2])
    x = data.reshape(-1, T, D).permute(0, 2, 1).unsqueeze(2).contiguous()            # [N, D, 1, T]
    if x.shape[0] == 0:
        return data.new_empty(lead + (T, int(joints_num), 3))
    xyz = hml_to_joints(x, engine=engine)                                             # [N, J, 3, T]
    return xyz.permute(0, 3, 1, 2).reshape(lead + (T, int(joints_num), 3))


def load_hml_stats(path):
    """(mean, std) fp32 [D] from an .npz with 'mean' and 'std', or from a directory holding Mean.npy / Std.npy as the dataset ships them."""
    if os.path.isdir(path):
        mean, std = (np.load(os.path.join(path, n), allow_pickle=False) for n in ("Mean.npy", "Std.npy"))
    else:
        with np.load(path, allow_pickle=False) as z:
            if "mean" not in z.files or "std" not in z.files:
                raise ValueError(f"{path} holds no 'mean' and 'std'")
            mean, std = z["mean"], z["std"]
    mean, std = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (mean, std))
    if mean.shape != std.shape:
        raise ValueError(f"{path}: mean {mean.shape} and std {std.shape} differ")
    joints_of(len(mean))
    return mean, std
