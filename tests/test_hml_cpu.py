"""The hml_vec post-processing without a GPU: the fp64 restatement (tests/hml_ref.py) against what the reference's own fp32 run returned
(tests/golden/hml_*.npz, recorded by tests/golden/make_golden_hml.py), the structural mutants, the masks, the argument checks of rgn_hml_to_joints,
and the wiring of the humanml / kit datasets through the factory, the parser and the edit mask.

THE BOUNDS (derived in tests/hml_ref.py's module text): the reference's fp32 run lies within gamma_T(2^-24) A of the exact value, element for element,
with A the absolute-sum companion of the same recurrences and gamma_T = T 2^-24 / (1 - T 2^-24). Measured when the fixtures were recorded: the
largest |restatement - fixture| / (gamma_T A) is 0.0027 (hml_t196), 0.0097 (hml_kit_t65), 0 (hml_t1), 0.48 (hml_t2), 0.010 (hml_raw_t64); as
orientation, the fp32 run lies within 4.8e-7 of an fp64 run at T = 196 and |xyz| up to 1.9. Every structural mutant misses every fixture it
applies to by at least 100 x that bound; the smallest ratio is 1538 (velocity_under_its_own_angle on hml_t196)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import hml_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = {"hml_t196": (1, 263, 196), "hml_kit_t65": (3, 251, 65), "hml_t1": (2, 263, 1), "hml_t2": (2, 263, 2), "hml_raw_t64": (2, 263, 64)}


def load_case(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as f:
        z = {k: f[k] for k in f.files}
    raw = bool(z["raw"])
    return z["x"], (None if raw else z["mean"]), (None if raw else z["std"]), z["expected"], z


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_is_what_the_issue_asks_for(name):
    x, mean, std, expected, z = load_case(name)
    B, D, T = CASES[name]
    assert x.shape == (B, D, 1, T) and x.dtype == np.float32 and expected.dtype == np.float32 and expected.shape == (B, hml_ref.joints_of(D), 3, T)
    assert z["mean"].shape == z["std"].shape == (D,) and os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= 400 * 1024
    if name == "hml_raw_t64":
        assert mean is None and not z["mean"].any() and (z["std"] == 1).all()
    if name == "hml_t196":       # |a| passes pi: a wrong angle convention cannot hide
        assert np.abs(np.cumsum(hml_ref.inv_transform(x, mean, std)[:, 0, :, 0], axis=1)).max() > np.pi


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_reference_run_within_its_fp32_model(name):
    x, mean, std, expected, z = load_case(name)
    T = x.shape[-1]
    ref = hml_ref.hml_joints_ref(x, mean, std)
    bound = hml_ref.gamma32(T) * hml_ref.error_model(x, mean, std)
    err = np.abs(ref - expected)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)
    print(f"{name}: max |restatement - fixture| {err.max():.3e}, / bound {ratio.max():.4f}, fp32 run vs fp64 run {float(z['ref64_gap']):.2e}")
    assert (err <= bound).all(), (name, float(ratio.max()))


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_mutant_misses_by_100_bounds(name):
    x, mean, std, expected, _ = load_case(name)
    B, D, _1, T = x.shape
    bound = hml_ref.gamma32(T) * hml_ref.error_model(x, mean, std)
    assert (bound > 0).all()
    applied = 0
    for mutant, applies in hml_ref.MUTANTS.items():
        if not applies(B, D, T, mean is not None):
            continue
        ratio = hml_ref.miss_ratio(hml_ref.hml_joints_ref(x, mean, std, mutant=mutant), expected.astype(np.float64), bound)
        print(f"{name}: {mutant} misses by {ratio:.0f} bounds")
        assert ratio >= 100, (name, mutant, ratio)
        applied += 1
    assert applied >= 3


def test_every_mutant_applies_somewhere():
    for mutant, applies in hml_ref.MUTANTS.items():
        assert any(applies(B, D, T, name != "hml_raw_t64") for name, (B, D, T) in CASES.items()), mutant


def test_masks_and_names_equal_the_reference():
    from regennet_amd.data_loaders import humanml_utils as hu
    with np.load(os.path.join(GOLDEN, "hml_masks.npz"), allow_pickle=False) as z:
        for k in ("HML_ROOT_MASK", "HML_LOWER_BODY_MASK", "HML_UPPER_BODY_MASK"):
            got = getattr(hu, k)
            assert got.dtype == bool and got.shape == (263,) and np.array_equal(got, z[k]), k
        assert hu.HML_JOINT_NAMES == [str(n) for n in z["HML_JOINT_NAMES"]] and hu.NUM_HML_JOINTS == 22
    assert hu.HML_ROOT_MASK.sum() == 7 and not (hu.HML_UPPER_BODY_MASK & hu.HML_LOWER_BODY_MASK).any()


def test_argument_refusals_answer_with_their_text_without_a_device():
    from regennet_amd import _lib
    lib = _lib.load()
    dev = C.c_void_p(64)          # stands for device memory: never dereferenced

    def call(x=dev, mean=dev, std=dev, B=2, T=5, D=263, J=22, xyz=dev):
        rc = lib.rgn_hml_to_joints(None, x, mean, std, B, T, D, J, xyz, None)
        return rc, (lib.rgn_last_error(None) or b"").decode()

    for kw in ({}, dict(mean=None, std=None), dict(D=251, J=21), dict(T=4096), dict(T=1), dict(D=23, J=2), dict(D=767, J=64), dict(B=2 ** 31 - 1)):
        rc, err = call(**kw)
        assert rc == -1 and err == "rgn_hml_to_joints: null handle", (kw, err)       # everything else passed
    for kw, text in [(dict(x=None), "null x or xyz"), (dict(xyz=None), "null x or xyz"), (dict(mean=None), "mean and std go together"),
                     (dict(std=None), "mean and std go together"), (dict(B=0), "B < 1"), (dict(B=-1), "B < 1"), (dict(T=0), "T = 0 outside [1, 4096]"),
                     (dict(T=4097), "T = 4097 outside [1, 4096]"), (dict(J=1, D=11), "J = 1 outside [2, 64]"), (dict(J=65, D=779), "J = 65 outside [2, 64]"),
                     (dict(D=251), "D = 251 rows, 12 J - 1 = 263 expected"), (dict(D=263, J=21), "D = 263 rows, 12 J - 1 = 251 expected"),
                     (dict(D=264), "D = 264 rows")]:
        rc, err = call(**kw)
        assert rc == -1 and err.startswith("rgn_hml_to_joints: ") and text in err, (kw, err)


def test_the_entry_point_is_declared_bound_exported_and_built():
    from regennet_amd import _lib
    header = open(os.path.join(ROOT, "include", "regennet_hip.h")).read()
    assert re.search(r"RGN_API int rgn_hml_to_joints\(rgn_handle h, const float\* x_dev, const float\* mean_dev", header)
    for cite in ("sample/cgenerate.py:147-152", "sample/edit.py:117-120", "sample/predict.py:114-117", "data_loaders/humanml/data/dataset.py:132",
                 "motion_process.py:362-381", "must NOT overlap"):
        assert cite in header, cite
    assert len(_lib.SYMBOLS["rgn_hml_to_joints"][1]) == 10
    assert hasattr(_lib.load(), "rgn_hml_to_joints") and hasattr(_lib.Engine, "hml_to_joints")
    assert "rgn_hml.hip" in __import__("__graft_entry__").SOURCES
    check = open(os.path.join(ROOT, "regennet_amd", "csrc", "rgn_hml_check.h")).read()
    assert "hip_runtime" not in check and "__global__" not in check and "__device__" not in check      # host only, for tools/hml_args_check.cpp
    assert os.path.exists(os.path.join(ROOT, "tools", "hml_args_check.cpp"))


@pytest.mark.parametrize("dataset,rows", [("humanml", 263), ("kit", 251)])
def test_the_factory_builds_the_hml_geometries(dataset, rows):
    import types

    from regennet_amd.utils.model_util import create_model_and_diffusion, get_model_args
    from regennet_amd.utils.parser_util import cgenerate_args
    args = cgenerate_args(["--dataset", dataset, "--layers", "1", "--latent_dim", "64"])
    data = types.SimpleNamespace(dataset=types.SimpleNamespace(num_actions=1, num_person=2))
    kw = get_model_args(args, data)
    assert (kw["njoints"], kw["nfeats"], kw["data_rep"], kw["cond_mode"], kw["num_frames"]) == (rows, 1, "hml_vec", "text", 196)
    model, _ = create_model_and_diffusion(args, data)
    assert (model.njoints, model.nfeats, model.data_rep, model.cond_mode, model.num_frames) == (rows, 1, "hml_vec", "text", 196)
    assert tuple(model.input_process.poseEmbedding.weight.shape) == (64, rows)


def test_build_mask_serves_upper_body_at_263_only():
    from regennet_amd.data_loaders.humanml_utils import HML_LOWER_BODY_MASK
    from regennet_amd.sample.edit import build_mask
    from regennet_amd.utils.parser_util import edit_args
    a = edit_args(["--edit_mode", "upper_body", "--dataset", "humanml"])
    m = build_mask(a, (3, 263, 1, 7))
    assert m.dtype == bool and m.shape == (3, 263, 1, 7) and m.flags["C_CONTIGUOUS"]
    assert all(np.array_equal(m[b, :, 0, t], HML_LOWER_BODY_MASK) for b in range(3) for t in range(7))      # True = keep the input (edit.py:84-88)
    for shape in ((1, 56, 6, 60), (1, 251, 1, 60)):
        with pytest.raises(NotImplementedError, match="HumanML3D"):
            build_mask(a, shape)


def test_the_parser_offers_the_datasets_and_their_options(tmp_path):
    from regennet_amd.utils.parser_util import cgenerate_args, edit_args
    a = cgenerate_args(["--dataset", "humanml"])
    assert a.dataset == "humanml" and a.hml_stats == "" and a.text_features == ""
    a = edit_args(["--dataset", "kit", "--hml_stats", "stats.npz", "--text_features", "f.npy", "--synthetic"])
    assert (a.dataset, a.hml_stats, a.text_features, a.synthetic) == ("kit", "stats.npz", "f.npy", True)
    assert cgenerate_args([]).dataset == "ntu"


def test_load_hml_stats_reads_both_forms(tmp_path):
    from regennet_amd.utils.hml import joints_of, load_hml_stats
    mean, std = hml_ref.make_stats(251, 5)
    np.savez(tmp_path / "stats.npz", mean=mean.astype(np.float64), std=std)
    np.save(tmp_path / "Mean.npy", mean)
    np.save(tmp_path / "Std.npy", std)
    for path in (tmp_path / "stats.npz", tmp_path):
        m, s = load_hml_stats(str(path))
        assert m.dtype == s.dtype == np.float32 and np.array_equal(m, mean) and np.array_equal(s, std)
    np.savez(tmp_path / "bad.npz", mean=mean[:250], std=std[:250])
    with pytest.raises(ValueError, match="12 J - 1"):
        load_hml_stats(str(tmp_path / "bad.npz"))
    assert joints_of(263) == 22 and joints_of(251) == 21


def test_the_clis_refuse_what_needs_a_body_and_cpu_tensors():
    import torch

    from regennet_amd.sample.cgenerate import hml_statistics
    from regennet_amd.utils.hml import hml_to_joints
    from regennet_amd.utils.parser_util import cgenerate_args
    for flags in (["--vertices"], ["--jointstype", "vibe"], ["--betas_npz", "synthetic"], ["--skeleton", "synthetic"]):
        with pytest.raises(SystemExit, match="no body"):
            hml_statistics(cgenerate_args(["--dataset", "humanml"] + flags))
    assert hml_statistics(cgenerate_args(["--dataset", "humanml"])) == (None, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hml_to_joints(torch.zeros(1, 263, 1, 4))
