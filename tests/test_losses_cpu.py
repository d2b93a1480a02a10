"""CPU: the loss-term restatement (tests/losses_ref.py) is pinned to fixtures recorded from the reference's own training_losses
(tests/golden/make_golden_losses.py), and the host side of the feature - the C entry point's argument checks, the Python surface's signature
and key rules, masked_l2, the input generator's conditions, the CLI's flags - behaves as specified. The kernel itself is tested in
tests/test_losses_gpu.py."""
import ctypes
import glob
import inspect
import os
import re

import numpy as np
import pytest
import torch

from regennet_amd import synth
from regennet_amd.diffusion import gaussian_diffusion as gd
from regennet_amd.diffusion.respace import SpacedDiffusion, space_timesteps
from tests import loss_cases
from tests.losses_ref import FOOT_JOINTS, TERMS, joints_of, loss_terms_ref, masked_l2, stack_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "losses_*.npz")))


def fixture_terms(g, dtype):
    sk = {"rest_joints": g["rest_joints"], "parents": g["parents"]}
    output = g["output"] if "output" in g else g["model_output"]
    return stack_terms(loss_terms_ref(g["target"], output, g["cmotion"], g["mask"], sk, float(g["vel_threshold"]), dtype=dtype))


def diffusion_with(resp="", **kw):
    return SpacedDiffusion(use_timesteps=space_timesteps(1000, resp or [1000]), betas=gd.get_named_beta_schedule("cosine", 1000),
                           model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE, **kw)


def test_the_recorded_cases_are_all_there():
    assert {n[len("losses_"):] for n in FIXTURES} == {"k_b3t7", "k_b2t33", "e2e_tiny", "e2e_tiny_r50", "e2e_ntu_action"}


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference(golden, name):
    """fp64: the same arithmetic as the recorded run up to the association of sums and of the chain's products: 1e-12 relative on every term."""
    g = golden(name)
    exp = g["expected"]
    assert exp.dtype == np.float64 and exp.shape == (g["target"].shape[0], 7) and np.isfinite(exp).all()
    rel = np.abs(fixture_terms(g, torch.float64) - exp) / np.abs(exp)
    rel32 = np.abs(fixture_terms(g, torch.float32) - exp) / np.abs(exp)
    print(name, "fp64", " ".join(f"{v:.1e}" for v in rel.max(0)), "| fp32", " ".join(f"{v:.1e}" for v in rel32.max(0)))
    assert float(rel.max()) < 1e-12, rel.max(0)


def test_kernel_fixtures_hold_no_undecided_foot_frame_and_no_orientation_near_pi(golden):
    contact = []
    for name in ("losses_k_b3t7", "losses_k_b2t33"):
        g = golden(name)
        cond = loss_cases.conditions({k: g[k] for k in ("target", "output", "cmotion")}, {"rest_joints": g["rest_joints"], "parents": g["parents"]},
                                     FOOT_JOINTS, float(g["vel_threshold"]))
        assert not cond["undecided"].any() and float(cond["max_angle"].max()) <= loss_cases.MAX_ANGLE
        contact.append(cond["contact"])
        assert list(g["foot_joints"]) == list(FOOT_JOINTS) and int(g["transl_row"]) == 55
    assert min(contact) > 0.5 and min(contact) < 0.95                 # both sides of the threshold occur


def test_generator_enforces_its_conditions_by_a_seed_search():
    """Every grid case is reproducible, holds at most one undecided motion and no root orientation beyond 3 rad. The search is not vacuous: at
    least one case's first seed is refused, and at least one case keeps an undecided motion (so the fc comparison's skip is exercised)."""
    moved, undecided = 0, 0
    for B, T, skel, mk, drift, thr, seed in loss_cases.GRID:
        inp, cond, used = loss_cases.find_inputs(B, T, skel, drift, thr, seed)
        assert int(cond["undecided"].sum()) <= 1 and float(cond["max_angle"].max()) <= loss_cases.MAX_ANGLE
        again, _, used2 = loss_cases.find_inputs(B, T, skel, drift, thr, seed)
        assert used2 == used and all(np.array_equal(inp[k], again[k]) for k in inp)
        moved += used != seed
        undecided += int(cond["undecided"].sum())
        assert loss_cases.make_mask(mk, B, T, seed).shape == (B, T)
    print("seeds moved by the search:", moved, " undecided motions kept:", undecided)
    assert moved >= 1 and undecided >= 1
    m = loss_cases.make_mask("ragged", 3, 7, 1)
    assert not m[0, 0] and m[0, 1] and not m.all(1).all() and (m.sum(1) >= 2).all()


def test_rgn_loss_terms_is_declared_bound_and_exported():
    from regennet_amd import _lib
    header = open(os.path.join(ROOT, "include", "regennet_hip.h")).read()
    assert re.search(r"RGN_API int rgn_loss_terms\(rgn_handle h, const float\* target_dev", header) and "gaussian_diffusion.py:1313-1391" in header
    assert "rgn_loss_terms" in _lib.SYMBOLS and len(_lib.SYMBOLS["rgn_loss_terms"][1]) == 17
    assert _lib.LOSS_TERMS == TERMS
    lib = _lib.load()
    assert hasattr(lib, "rgn_loss_terms")
    assert "rgn_loss.hip" in __import__("__graft_entry__").SOURCES


def test_rgn_loss_terms_argument_checks_need_no_device():
    """Each bad argument is RGN_ERR_INVALID_ARG with its text, before the handle or the device is looked at: the calls below pass a NULL handle and
    non-null dummy 'device' pointers that are never dereferenced."""
    from regennet_amd import _lib
    lib = _lib.load()
    vp = ctypes.c_void_p
    dummy = (ctypes.c_float * 4)()
    dev = ctypes.cast(dummy, vp)
    rest = np.zeros((65, 3), np.float32)
    par = np.arange(-1, 64, dtype=np.int32)
    foot = np.array([0, 1, 2, 1], np.int32)

    def call(target=dev, output=dev, cmotion=dev, mask=dev, terms=dev, rest_=rest, par_=par, foot_=foot, B=1, T=2, R=4, J=3, row=3, flags=1):
        p = lambda a: None if a is None else a.ctypes.data_as(vp)      # noqa: E731
        rc = lib.rgn_loss_terms(None, target, output, cmotion, mask, B, T, R, J, p(rest_), p(par_), p(foot_), row, 0.01, flags, terms, None)
        return rc, (lib.rgn_last_error(None) or b"").decode()

    rc, err = call()
    assert rc == -1 and "null handle" in err          # everything else passed
    cases = [(dict(target=None), "null"), (dict(output=None), "null"), (dict(cmotion=None), "null"), (dict(mask=None), "null"), (dict(terms=None), "null"),
             (dict(rest_=None), "null"), (dict(par_=None), "null"), (dict(foot_=None), "null"), (dict(B=0), "B < 1"), (dict(T=0), "T < 1"),
             (dict(J=0, R=1), "J outside [1, 64]"), (dict(J=65, R=66), "J outside [1, 64]"),
             (dict(par_=np.array([0, 0, 1], np.int32)), "parents[0] != -1"), (dict(par_=np.array([-1, 1, 1], np.int32)), "parents[1]"),
             (dict(par_=np.array([-1, 0, 2], np.int32)), "parents[2]"), (dict(par_=np.array([-1, 0, -1], np.int32)), "parents[2]"),
             (dict(R=3), "J + 1 = 4"), (dict(R=5), "J + 1 = 4"), (dict(foot_=np.array([0, 1, 3, 1], np.int32)), "foot_joints[2] = 3"),
             (dict(foot_=np.array([-1, 1, 2, 1], np.int32)), "foot_joints[0] = -1"), (dict(row=4), "transl_row 4"), (dict(row=-1), "transl_row -1"),
             (dict(flags=2), "unknown flag")]
    for kw, text in cases:
        rc, err = call(**kw)
        assert rc == -1 and err.startswith("rgn_loss_terms: ") and text in err, (kw, rc, err)


def test_training_losses_has_the_reference_signature():
    for cls in (gd.GaussianDiffusion, SpacedDiffusion):
        assert hasattr(cls, "training_losses")
    sig = inspect.signature(gd.GaussianDiffusion.training_losses)
    assert list(sig.parameters) == ["self", "model", "x_start", "t", "model_kwargs", "noise", "dataset"]
    assert all(sig.parameters[k].default is None for k in ("model_kwargs", "noise", "dataset"))
    assert list(inspect.signature(gd.GaussianDiffusion.masked_l2).parameters) == ["self", "a", "b", "mask"]
    assert "training_losses" in SpacedDiffusion.__dict__                       # wraps the model like respace.py:94-97


LAMBDA_SETS = {
    "zero": {},
    "defaults": dict(lambda_orient=1.0, lambda_body=1.0, lambda_transl=1.0),
    "all": dict(lambda_rcxyz=0.5, lambda_vel=2.0, lambda_fc=3.0, lambda_orient=1.0, lambda_body=0.25, lambda_transl=4.0),
}


def expected_keys(lam, dataname):
    keys = {"rot_mse", "loss"}
    keys |= {k for k, l in (("rcxyz_mse", "lambda_rcxyz"), ("vel_mse", "lambda_vel"), ("orient", "lambda_orient"), ("body", "lambda_body"),
                            ("transl", "lambda_transl")) if lam.get(l, 0.0) > 0}
    if lam.get("lambda_fc", 0.0) > 0 and dataname in ("humanact12", "uestc", "ntu", "chi3d"):
        keys.add("fc")
    return keys


def weighted(lam, terms, keys):
    """:1393-1399, in the reference's order."""
    c = {k: terms[:, i] for i, k in enumerate(TERMS)}
    g = lambda k: c[k] if k in keys else 0.0                              # noqa: E731
    return c["rot_mse"] + 0.0 + lam.get("lambda_vel", 0.0) * g("vel_mse") + lam.get("lambda_rcxyz", 0.0) * g("rcxyz_mse") + \
        lam.get("lambda_fc", 0.0) * g("fc") + lam.get("lambda_orient", 0.0) * g("orient") + lam.get("lambda_body", 0.0) * g("body") + \
        lam.get("lambda_transl", 0.0) * g("transl")


@pytest.mark.parametrize("lam", list(LAMBDA_SETS))
@pytest.mark.parametrize("dataset", [None, "ntu", "kit", "object:chi3d"])
def test_key_rules_and_weighting_of_the_returned_dict(lam, dataset):
    """rot_mse always, every other term only with a positive weight, fc only for the reference's datasets (given as an object with .dataname or
    as the name), loss = the reference's weighted sum."""
    import types
    lams = LAMBDA_SETS[lam]
    d = diffusion_with(data_rep="rot6d", **lams)
    terms = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).uniform(0.1, 1.0, (4, 7)).astype(np.float32))
    ds = types.SimpleNamespace(dataname=dataset[7:]) if isinstance(dataset, str) and dataset.startswith("object:") else dataset
    name = getattr(ds, "dataname", ds)
    out = d._loss_dict(terms, ds)
    keys = expected_keys(lams, name)
    assert set(out) == keys
    for k in keys - {"loss"}:
        assert torch.equal(out[k], terms[:, TERMS.index(k)]) and tuple(out[k].shape) == (4,)
    assert torch.equal(out["loss"], weighted(lams, terms, keys))
    if lam == "all":
        assert ("fc" in out) == (name in ("ntu", "chi3d"))


def test_training_losses_refuses_what_it_does_not_evaluate():
    x = torch.zeros(2, 56, 6, 8)
    t = torch.zeros(2, dtype=torch.long)
    kw = dict(use_timesteps=space_timesteps(1000, [1000]), betas=gd.get_named_beta_schedule("cosine", 1000), model_mean_type=gd.ModelMeanType.START_X)
    with pytest.raises(NotImplementedError, match="MSE"):
        SpacedDiffusion(model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.KL, **kw).training_losses(None, x, t)
    with pytest.raises(NotImplementedError, match="MSE"):
        SpacedDiffusion(model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.RESCALED_MSE, **kw).training_losses(None, x, t)
    with pytest.raises(NotImplementedError, match="learned variances"):
        SpacedDiffusion(model_var_type=gd.ModelVarType.LEARNED_RANGE, loss_type=gd.LossType.MSE, **kw).training_losses(None, x, t)
    with pytest.raises(NotImplementedError, match="lambda_vel_rcxyz"):
        diffusion_with(lambda_vel_rcxyz=1.0).training_losses(None, x, t)
    with pytest.raises(TypeError, match="HIP denoiser"):
        diffusion_with().training_losses(lambda *a, **k: x, x, t, model_kwargs={"y": {}})


def _model(njoints):
    from regennet_amd.model.cmdm import CMDM
    cfg = synth.get_config("tiny", njoints=njoints)
    return CMDM("", cfg["njoints"], cfg["nfeats"], cfg["num_actions"], True, "rot6d", True, True, num_frames=cfg["num_frames"],
                latent_dim=cfg["latent_dim"], ff_size=cfg["ff_size"], num_layers=cfg["layers"], num_heads=cfg["num_heads"], arch="online",
                cm_mode=cfg["cm_mode"], body_model="smplx", cond_mode=cfg["cond_mode"], cond_mask_prob=cfg["cond_mask_prob"], dataset="ntu").eval()


def test_training_losses_names_the_hard_coded_rows_and_needs_a_skeleton():
    t = torch.zeros(2, dtype=torch.long)
    y = {"mask": torch.ones(2, 1, 1, 8, dtype=torch.bool), "cmotion": torch.zeros(2, 5, 6, 8)}
    with pytest.raises(ValueError, match=r"row 55 .* joints 7, 8, 10 and 11"):
        diffusion_with().training_losses(_model(5), torch.zeros(2, 5, 6, 8), t, model_kwargs={"y": y})
    y56 = {"mask": torch.ones(2, 1, 1, 8, dtype=torch.bool), "cmotion": torch.zeros(2, 56, 6, 8)}
    import types
    for wrap in (lambda m: m, lambda m: types.SimpleNamespace(module=m)):      # bare, and as the `.module` of a wrapper
        with pytest.raises(NotImplementedError, match="skeleton"):
            diffusion_with().training_losses(wrap(_model(56)), torch.zeros(2, 56, 6, 8), t, model_kwargs={"y": y56})
    with pytest.raises(KeyError):
        diffusion_with().training_losses(_model(56), torch.zeros(2, 56, 6, 8), t)


@pytest.mark.parametrize("shape", ["BJ3T", "B1T", "BJT"])
def test_masked_l2_matches_the_restatement(shape):
    """[B,J,3,T] with the [B,1,1,T] mask, and the 3-D inputs of orient / transl ([B,1,T]) and body ([B,J,T]) with mask.squeeze(1): the divisor
    carries a.shape[1] * a.shape[2], whatever those axes mean; an empty mask gives NaN."""
    rng = np.random.Generator(np.random.PCG64(5))
    B, J, T = 3, 5, 7
    dims = {"BJ3T": (B, J, 3, T), "B1T": (B, 1, T), "BJT": (B, J, T)}[shape]
    a, b = (torch.from_numpy(rng.standard_normal(dims)) for _ in range(2))
    m = torch.from_numpy(rng.uniform(size=(B, 1, 1, T)) < 0.6)
    m[2] = False
    mask = m if len(dims) == 4 else m.squeeze(1)
    got = diffusion_with().masked_l2(a, b, mask)
    want = masked_l2(a, b, mask)
    by_hand = np.array([((a[i] - b[i]) ** 2 * mask[i].double()).sum().item() / (int(m[i].sum()) * dims[1] * dims[2]) if int(m[i].sum()) else np.nan
                        for i in range(B)])
    assert tuple(got.shape) == (B,) and torch.isnan(got[2]) and torch.isnan(want[2])
    assert torch.equal(got[:2], want[:2]) and np.allclose(got[:2].numpy(), by_hand[:2], rtol=1e-14, atol=0)
    if shape != "BJ3T":
        assert dims[1] * dims[2] == (T if shape == "B1T" else J * T)               # the extra 1 / T of the three interaction terms


def test_restatement_joints_are_rot2xyz_without_mask_and_translation_term(golden):
    g = golden("losses_k_b3t7")
    xyz = joints_of(g["target"], {"rest_joints": g["rest_joints"], "parents": g["parents"]}, torch.float64)
    assert tuple(xyz.shape) == (3, 55, 3, 7) and float(xyz[:, 0].abs().max()) == 0.0 and float(xyz[:, 1:].abs().min()) > 0.0


def test_score_cli_flags():
    from regennet_amd.eval import score
    from regennet_amd.utils.parser_util import score_args
    a = score_args(["--synthetic", "--skeleton", "synthetic", "--num_samples", "8", "--t_grid", "5"])
    assert (a.t_grid, a.num_samples, a.skeleton, a.synthetic) == (5, 8, "synthetic", True)
    assert (a.lambda_orient, a.lambda_body, a.lambda_transl, a.lambda_rcxyz, a.lambda_vel, a.lambda_fc, a.vel_threshold) == (1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.01)
    b = score_args(["--synthetic", "--lambda_fc", "2", "--lambda_orient", "0", "--vel_threshold", "0.03", "--data_path", "x.npy"])
    assert (b.lambda_fc, b.lambda_orient, b.lambda_body, b.vel_threshold, b.data_path, b.t_grid) == (2.0, 0.0, 1.0, 0.03, "x.npy", 10)
    with pytest.raises(SystemExit):
        score_args(["--synthetic", "--t_grid", "0"])
    assert score.timestep_grid(1000, 5) == [0, 250, 500, 749, 999] and score.timestep_grid(50, 1) == [25] and score.timestep_grid(3, 10) == [0, 1, 2]
    table = score.format_table([0, 999], {"rot_mse": np.array([[1.0, 3.0], [2.0, np.nan]]), "loss": np.array([[1.0, 1.0], [4.0, 4.0]])})
    assert table.splitlines()[0].split() == ["t", "rot_mse", "loss"] and table.splitlines()[2].split() == ["999", "2.00000e+00", "4.00000e+00"]
