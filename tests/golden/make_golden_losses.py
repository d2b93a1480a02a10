"""Fixtures of the training-loss terms, recorded by RUNNING THE REFERENCE (CPU, fp64) in the build container.

    python tests/golden/make_golden_losses.py

`GaussianDiffusion.training_losses` (diffusion/gaussian_diffusion.py:1239-1403) is run as it stands, through `SpacedDiffusion.training_losses`
(diffusion/respace.py:94-97): masked_l2, the three rot2xyz passes, the rotation conversions of utils/rotation_conversions.py and the weighting
are the reference's own code. The body layer its rot2xyz calls is the stand-in of make_golden_rot2xyz.py (posed skeleton joints of
regennet_amd.synth.make_skeleton(), fp64 from fp32 rest joints).

  kernel cases      the "model" is a stub that returns a prescribed output, so the terms depend on the stored tensors alone
                    (inputs: tests/loss_cases.py, no undecided foot frame, root orientations within 3 rad)
  end-to-end cases  the reference's own CMDM(arch='online') on a synthetic checkpoint, fp32 as it runs in practice; the terms are then formed in
                    fp64 from its recorded output. `sens` is, per term, the largest change when that output moves by +-1e-3 (the project's
                    documented output bound) with random signs, three draws.

Only DATA is written: tests/golden/losses_<case>.npz."""
import os
import sys
import types
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
import make_golden_rot2xyz as r2x  # noqa: E402
from regennet_amd import synth  # noqa: E402
from tests import loss_cases  # noqa: E402

TERMS = ("rot_mse", "rcxyz_mse", "vel_mse", "fc", "orient", "body", "transl")
LAMBDAS = dict(lambda_rcxyz=1.0, lambda_vel=1.0, lambda_fc=1.0, lambda_orient=1.0, lambda_body=1.0, lambda_transl=1.0)
NTU = types.SimpleNamespace(dataname="ntu")
_zeros = lambda *a, **k: np.zeros((9, 1), np.float32)       # noqa: E731  J_regressor_extra (model/smpl.py:76), unused by 'smplx'


def ref_diffusion(vel_threshold, resp=""):
    from diffusion import gaussian_diffusion as gd
    from diffusion.respace import SpacedDiffusion, space_timesteps
    return SpacedDiffusion(use_timesteps=space_timesteps(1000, resp or [1000]), betas=gd.get_named_beta_schedule("cosine", 1000, 1.0),
                           model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE,
                           rescale_timesteps=False, data_rep="rot6d", num_person=1, body_model="smplx", vel_threshold=vel_threshold, **LAMBDAS)


class _Stub:
    """What training_losses sees of a model: `.module` with rot2xyz and its settings, and a call that returns the prescribed output."""

    def __init__(self, enc, output):
        self.module, self.output = enc, output

    def __call__(self, x, ts, **kw):
        return self.output


class _Wrapper:
    """Stands where DistributedDataParallel stands in training: `.module` and a call."""

    def __init__(self, module):
        self.module = module

    def __call__(self, x, ts, **kw):
        return self.module(x, ts, **kw)


def ref_terms(diffusion, enc, target, output, cmotion, mask, t=None, noise=None):
    """The reference's terms in fp64 for a prescribed model output -> [B, 7] and the weighted loss [B]."""
    B, T = mask.shape
    y = {"mask": torch.from_numpy(mask).reshape(B, 1, 1, T), "cmotion": torch.from_numpy(cmotion).double()}
    x0 = torch.from_numpy(target).double()
    out = diffusion.training_losses(_Stub(enc, torch.from_numpy(np.asarray(output)).double()), x0, torch.zeros(B, dtype=torch.long) if t is None else t,
                                    model_kwargs={"y": y}, noise=torch.zeros_like(x0) if noise is None else noise, dataset=NTU)
    assert set(out) == set(TERMS) | {"loss"} and all(v.dtype == torch.float64 and tuple(v.shape) == (B,) for v in out.values())
    return np.stack([out[k].numpy() for k in TERMS], 1), out["loss"].numpy()


def kernel_cases(enc, sk):
    for name, (B, T, mk, drift, thr, seed) in {"k_b3t7": (3, 7, "ragged", 0.01, 0.03, 1), "k_b2t33": (2, 33, "full", 0.004, 0.01, 2)}.items():
        inp, cond, used = loss_cases.find_inputs(B, T, "tree55", drift, thr, seed, max_undecided=0)
        mask = loss_cases.make_mask(mk, B, T, seed)
        terms, loss = ref_terms(ref_diffusion(thr), enc, inp["target"], inp["output"], inp["cmotion"], mask)
        path = os.path.join(HERE, f"losses_{name}.npz")
        np.savez_compressed(path, mask=mask, rest_joints=sk["rest_joints"], parents=sk["parents"], vel_threshold=np.array(thr), seed=np.array(used),
                            foot_joints=np.array([7, 10, 8, 11], np.int32), transl_row=np.array(55), expected=terms, loss=loss, **inp)
        print(f"{name}: seed {used}  max angle {cond['max_angle'].max():.3f}  smallest gap {cond['gap'].min():.2e} (16 d = {16 * cond['d'].max():.2e})  "
              f"contact {cond['contact']:.2f}  {os.path.getsize(path)} B\n    " + "  ".join(f"{k} {v:.3e}" for k, v in zip(TERMS, terms[0])))


def e2e_cases(sk):
    for name, (cfg_name, over, B, resp) in {"e2e_tiny": ("tiny", {"njoints": 56}, 3, ""), "e2e_tiny_r50": ("tiny", {"njoints": 56}, 3, "50"),
                                            "e2e_ntu_action": ("ntu_action", {}, 2, "")}.items():
        cfg = synth.get_config(cfg_name, **over)
        sd = synth.make_state_dict(cfg, seed=0)
        with mock.patch("numpy.load", _zeros):
            model, _ = _ref_import.build_reference(cfg, sd, resp)
        T, thr = cfg["num_frames"], 0.03
        diffusion = ref_diffusion(thr, resp)
        S = diffusion.num_timesteps
        inp, cond, used = loss_cases.find_inputs(B, T, "tree55", 0.01, thr, 7, max_undecided=0)
        mask = loss_cases.make_mask("ragged", B, T, 3)
        rng = np.random.Generator(np.random.PCG64(17))
        t = torch.tensor([S // 10, S // 2, S - 1][:B], dtype=torch.long)
        noise = rng.standard_normal(inp["target"].shape).astype(np.float32)
        y = {"mask": torch.from_numpy(mask).reshape(B, 1, 1, T), "cmotion": torch.from_numpy(inp["cmotion"])}
        if "action" in cfg["cond_mode"]:
            y["action"] = torch.from_numpy(synth.make_actions(cfg, B))
        # the reference run as a user makes it: fp32 model, its own call chain; the wrapped model's call is logged for x_t and the mapped timesteps
        log = []
        fwd = model.forward
        model.forward = lambda x, ts, **kw: (log.append((x.clone(), ts.clone())), fwd(x, ts, **kw))[1]
        with torch.no_grad():
            out32 = diffusion.training_losses(_Wrapper(model), torch.from_numpy(inp["target"]), t, model_kwargs={"y": y}, noise=torch.from_numpy(noise),
                                              dataset=NTU)
        model.forward = fwd
        (x_t, t_model), = log
        with torch.no_grad():
            model_output = model(x_t, t_model, y=y).numpy()
        # the terms in fp64 from the recorded output, and their sensitivity to the output bound
        enc = types.SimpleNamespace(rot2xyz=model.rot2xyz, pose_rep="rot6d", translation=True, glob=True)
        terms, loss = ref_terms(diffusion, enc, inp["target"], model_output, inp["cmotion"], mask, t=t, noise=torch.from_numpy(noise).double())
        terms32 = np.stack([out32[k].double().numpy() for k in TERMS], 1)
        sens = np.zeros_like(terms)
        for _ in range(3):
            moved = model_output.astype(np.float64) + 1e-3 * rng.choice([-1.0, 1.0], model_output.shape)
            sens = np.maximum(sens, np.abs(ref_terms(diffusion, enc, inp["target"], moved, inp["cmotion"], mask, t=t)[0] - terms))
        path = os.path.join(HERE, f"losses_{name}.npz")
        np.savez_compressed(path, cfg_name=np.array(cfg_name), over=np.array(repr(over)), resp=np.array(resp), B=np.array(B), t=t.numpy(),
                            t_model=t_model.numpy(), noise=noise, mask=mask, model_output=model_output, expected=terms, loss=loss,
                            sens=sens, rest_joints=sk["rest_joints"], parents=sk["parents"], vel_threshold=np.array(thr), seed=np.array(used),
                            **({"action": y["action"].numpy()} if "action" in y else {}), target=inp["target"], cmotion=inp["cmotion"])
        print(f"{name}: t {t.tolist()} -> {t_model.tolist()}  fp32 run vs fp64 terms, max rel {np.nanmax(np.abs(terms32 - terms) / np.abs(terms)):.2e}  "
              f"{os.path.getsize(path)} B\n    " + "  ".join(f"{k} {v:.3e} (sens {s:.1e})" for k, v, s in zip(TERMS, terms[0], sens[0])))


def main():
    _, Rotation2xyz_x = r2x.reference_wrappers()
    posed = r2x._SkeletonLayer.posed        # the stand-in answers in fp64 whatever it is asked in; the fp32 end-to-end run needs its input's dtype back

    def posed_like_input(self, rot, betas):
        out = posed(self, rot, betas)
        return types.SimpleNamespace(joints=out.joints.to(rot.dtype), vertices=out.vertices.to(rot.dtype))

    r2x._SkeletonLayer.posed = posed_like_input
    sk = synth.make_skeleton()
    r2x._SkeletonLayer.skeleton = sk
    with mock.patch("numpy.load", _zeros):
        enc = types.SimpleNamespace(rot2xyz=Rotation2xyz_x("cpu"), pose_rep="rot6d", translation=True, glob=True)
    kernel_cases(enc, sk)
    e2e_cases(sk)


if __name__ == "__main__":
    main()
