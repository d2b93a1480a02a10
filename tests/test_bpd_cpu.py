"""CPU: the restatement of the likelihood evaluation (tests/bpd_ref.py) is pinned to fixtures recorded from the reference's own calc_bpd_loop and
_vb_terms_bpd (tests/golden/make_golden_bpd.py), and the host side of the feature - the torch expressions _prior_bpd, q_mean_variance and
q_posterior_mean_variance, the row bookkeeping of calc_bpd_loop (on a stand-in engine that answers with the restatement), the two entry points'
argument checks, the constructed inputs, the CLI's flag - behaves as specified. The kernels themselves are tested in tests/test_bpd_gpu.py."""
import ctypes
import glob
import inspect
import os
import re

import numpy as np
import pytest
import torch

from regennet_amd.diffusion import gaussian_diffusion as gd
from regennet_amd.diffusion.respace import SpacedDiffusion, space_timesteps
from tests import bpd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "bpd_*.npz")))
LOOP_CASES = ("bpd_k_n105_r4", "bpd_k_n240_large_r5")
KEYS = {"total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"}


def fixture_diffusion(g):
    return SpacedDiffusion(use_timesteps=space_timesteps(1000, str(g["resp"]) or [1000]), betas=gd.get_named_beta_schedule(str(g["schedule"]), 1000),
                           model_mean_type=gd.ModelMeanType.START_X,
                           model_var_type=gd.ModelVarType.FIXED_LARGE if bool(g["large"]) else gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)


def spacing32(v):
    return np.spacing(np.abs(np.asarray(v)).astype(np.float32)).astype(np.float64)


def test_the_recorded_cases_are_all_there():
    assert {n[len("bpd_"):] for n in FIXTURES} == {"k_n105_r4", "k_n240_large_r5", "k_rows_cos1000", "e2e_tiny_r10", "e2e_tiny_cos1000", "e2e_ntu_action_r4"}
    assert all(os.path.getsize(os.path.join(ROOT, "tests", "golden", n + ".npz")) < 1000000 for n in FIXTURES)


@pytest.mark.parametrize("name", [n for n in FIXTURES if n.startswith("bpd_k_")])
def test_restatement_reproduces_the_reference(golden, name):
    """fp64 from the fp32 tensors and fp32 coefficients: 1e-12 relative on every recorded number of the kernel cases."""
    g = golden(name)
    d = fixture_diffusion(g)
    args = (g["x_start"], g["x_t"], g["output"], g["noise"], g["t"], bpd_ref.coef_rows(d, g["t"]), bool(g["clip"]))
    r64, r32 = bpd_ref.vb_terms_ref(*args, dtype=torch.float64), bpd_ref.vb_terms_ref(*args, dtype=torch.float32)
    assert np.array_equal(g["x_t"], bpd_ref.q_sample_rows_ref(g["x_start"], g["noise"], bpd_ref.q_coef_rows(d, g["t"])))
    assert (g["t"] == 0).any() and (g["t"] != 0).any()
    if "expected" in g:
        exp = g["expected"]
        assert exp.dtype == np.float64 and exp.shape == (len(g["t"]), 3) and np.isfinite(exp).all()
        prior = bpd_ref.prior_bpd_ref(d, g["x_start"])
        assert float((np.abs(prior - g["prior_bpd"]) / np.abs(g["prior_bpd"])).max()) < 1e-12
        assert float(np.abs(g["vb"].sum(1) + g["prior_bpd"] - g["total_bpd"]).max()) <= 1e-12 * float(np.abs(g["total_bpd"]).max())
    else:
        exp, r64, r32 = g["expected_vb"][:, None], r64[:, :1], r32[:, :1]
    rel, rel32 = np.abs(r64 - exp) / np.abs(exp), np.abs(r32 - exp) / np.abs(exp)
    print(name, "fp64", " ".join(f"{v:.1e}" for v in rel.max(0)), "| fp32", " ".join(f"{v:.1e}" for v in rel32.max(0)))
    assert float(rel.max()) < 1e-12, rel.max(0)


def test_inputs_are_constructed_so_that_no_branch_hangs_on_rounding(golden):
    """x_start holds elements below -0.999, above 0.999 and between, none within 1e-4 of either threshold - in the fixtures and in every grid
    case of the GPU test; outputs leave [-1, 1], so the clamp does something."""
    for name in FIXTURES:
        if name.startswith("bpd_k_"):
            g = golden(name)
            assert bpd_ref.inputs_are_decided(g["x_start"]) and float(np.abs(g["output"]).max()) > 1.0, name
    for row in bpd_ref.GRID:
        c = bpd_ref.grid_case(row[0])
        again = bpd_ref.grid_case(row[0])
        assert bpd_ref.inputs_are_decided(c["x_start"]) and float(np.abs(c["output"]).max()) > 1.0, row[0]
        assert all(np.array_equal(c[k], again[k]) for k in ("x_start", "x_t", "output", "noise", "coef", "t"))
        assert c["N"] % c["B"] == 0 and (c["t"] == 0).any() and c["x_t"].dtype == np.float32
    assert any((bpd_ref.grid_case(r[0])["t"] != 0).any() for r in bpd_ref.GRID)
    x0 = np.array([-1.1, 0.0, 0.99905, 1.1], np.float32)
    assert not bpd_ref.inputs_are_decided(x0) and bpd_ref.inputs_are_decided(np.array([-1.1, 0.0, 1.1], np.float32))


@pytest.mark.parametrize("name", LOOP_CASES)
def test_torch_expressions_agree_with_the_reference(golden, name):
    """_prior_bpd, q_mean_variance and q_posterior_mean_variance on CPU tensors, fp32 as the reference computes them, against the values the
    reference gave in fp64: within 4 x |fp32 restatement - fp64 restatement|, with one fp32 spacing of the value as floor."""
    g = golden(name)
    d = fixture_diffusion(g)
    x0, B = torch.from_numpy(g["x_start"]), int(g["B"])
    tq = torch.from_numpy(g["tq"])
    x_t = torch.from_numpy(g["x_t"][:B])

    def bound(r32, r64, value):
        return np.maximum(4 * np.abs(np.asarray(r32, dtype=np.float64) - r64), spacing32(value))

    def coef(tab, dtype):
        return torch.from_numpy(tab[g["tq"]].astype(np.float32)).to(dtype).reshape(B, 1, 1, 1)

    got = d._prior_bpd(x0)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B,)
    r64, r32 = bpd_ref.prior_bpd_ref(d, g["x_start"], torch.float64), bpd_ref.prior_bpd_ref(d, g["x_start"], torch.float32)
    assert (np.abs(got.double().numpy() - g["prior_bpd"]) <= bound(r32, r64, g["prior_bpd"])).all(), (got, g["prior_bpd"])

    mean, var, logvar = d.q_mean_variance(x0, tq)
    assert mean.shape == var.shape == logvar.shape == x0.shape and mean.dtype == torch.float32
    m64 = (coef(d.sqrt_alphas_cumprod, torch.float64) * x0.double()).numpy()
    m32 = (coef(d.sqrt_alphas_cumprod, torch.float32) * x0).numpy()
    assert float(np.abs(m64 - g["q_mean"]).max()) == 0.0
    assert (np.abs(mean.double().numpy() - g["q_mean"]) <= bound(m32, m64, g["q_mean"])).all()
    assert (np.abs(var[:, 0, 0, 0].double().numpy() - g["q_variance"]) <= spacing32(g["q_variance"])).all()
    assert (np.abs(logvar[:, 0, 0, 0].double().numpy() - g["q_log_variance"]) <= spacing32(g["q_log_variance"])).all()

    pm, pv, plv = d.q_posterior_mean_variance(x0, x_t, tq)
    p64 = (coef(d.posterior_mean_coef1, torch.float64) * x0.double() + coef(d.posterior_mean_coef2, torch.float64) * x_t.double()).numpy()
    p32 = (coef(d.posterior_mean_coef1, torch.float32) * x0 + coef(d.posterior_mean_coef2, torch.float32) * x_t).numpy()
    assert float((np.abs(p64 - g["qp_mean"]) / np.maximum(np.abs(g["qp_mean"]), 1e-30)).max()) < 1e-12
    assert (np.abs(pm.double().numpy() - g["qp_mean"]) <= bound(p32, p64, g["qp_mean"])).all()
    assert (np.abs(pv[:, 0, 0, 0].double().numpy() - g["qp_variance"]) <= spacing32(g["qp_variance"])).all()
    assert (np.abs(plv[:, 0, 0, 0].double().numpy() - g["qp_log_variance"]) <= spacing32(g["qp_log_variance"])).all()

    eps = d._predict_eps_from_xstart(x_t, tq, x0)
    e64 = ((coef(d.sqrt_recip_alphas_cumprod, torch.float64) * x_t.double() - x0.double()) / coef(d.sqrt_recipm1_alphas_cumprod, torch.float64)).numpy()
    assert eps.dtype == torch.float32 and float((np.abs(eps.double().numpy() - e64) / np.maximum(np.abs(e64), 1.0)).max()) < 1e-4


# ---- calc_bpd_loop's bookkeeping on a stand-in engine ----------------------------------------------------------------------------------------
class _RefEngine:
    """Answers the two kernel calls with the fp64 restatement, on CPU tensors."""

    def __init__(self):
        self.q_calls, self.vb_calls = [], []

    def q_sample_rows(self, x_start, noise, coef, t, seed, sample_offset, x_t, noise_out, stream):
        assert noise is not None, "the stand-in draws nothing"
        self.q_calls.append(t.numpy().copy())
        x_t.copy_(torch.from_numpy(bpd_ref.q_sample_rows_ref(x_start.numpy(), noise.numpy(), coef.numpy())))

    def vb_terms(self, x_start, x_t, output, noise, t, coef, flags, terms, stream):
        self.vb_calls.append((t.numpy().copy(), coef.numpy().copy(), flags))
        terms.copy_(torch.from_numpy(bpd_ref.vb_terms_ref(x_start.numpy(), x_t.numpy(), output.numpy(), None if noise is None else noise.numpy(),
                                                          t.numpy(), coef.numpy(), bool(flags & 1))).float())


class _TableModel:
    """A 'model' that answers row (mapped timestep, motion) with the fixture's prescribed output, whatever the grouping into calls."""

    def __init__(self, g, d):
        S, B = d.num_timesteps, int(g["B"])
        self.out = {(d.timestep_map[int(t)], r % B): g["output"][r] for r, t in enumerate(g["t"])}
        self._engine = _RefEngine()
        self.calls, self.B = [], B

    def _get_engine(self, B, T=None):
        return self._engine, torch.device("cpu")

    def __call__(self, x, ts, y=None):
        assert tuple(y["tag"].shape) == (x.shape[0],) and y["tag"].tolist() == [r % self.B for r in range(x.shape[0])] and y["const"] == "kept"
        self.calls.append((x.clone(), ts.clone()))
        return torch.from_numpy(np.stack([self.out[(int(t), r % self.B)] for r, t in enumerate(ts)]))


@pytest.mark.parametrize("rows", [1, "B", "2B", 256])
@pytest.mark.parametrize("name", LOOP_CASES)
def test_calc_bpd_loop_keys_column_order_and_grouping(golden, name, rows):
    """The dict has the reference's keys; column k holds timestep S - 1 - k; every evaluation holds whole timesteps in (t, b) order, at most
    max_rows_per_call rows and at least one timestep; the model sees mapped timesteps and the per-sample entries of y repeated; the tape's entry
    k is consumed at timestep S - 1 - k."""
    g = golden(name)
    d = fixture_diffusion(g)
    B, S = int(g["B"]), d.num_timesteps
    rows = {"B": B, "2B": 2 * B}.get(rows, rows)
    model = _TableModel(g, d)
    tape = torch.from_numpy(g["noise"].reshape((S, B) + g["noise"].shape[1:]))
    y = {"tag": torch.arange(B), "const": "kept"}
    out = d.calc_bpd_loop(model, torch.from_numpy(g["x_start"]), clip_denoised=bool(g["clip"]), model_kwargs={"y": y}, noise_tape=tape,
                          max_rows_per_call=rows)
    assert set(out) == KEYS == {k for k in g.files if k in KEYS}
    for k in ("vb", "xstart_mse", "mse"):
        assert tuple(out[k].shape) == g[k].shape == (B, S) and out[k].dtype == torch.float32
        assert np.allclose(out[k].double().numpy(), g[k], rtol=1e-6, atol=0), k          # (fp32 roundings of fp64 values: the order is what is tested)
    assert not np.allclose(g["vb"][:, ::-1], g["vb"], rtol=1e-3)                          # ... and the order matters
    assert torch.equal(out["total_bpd"], out["vb"].sum(dim=1) + out["prior_bpd"]) and tuple(out["total_bpd"].shape) == (B,)
    assert np.allclose(out["prior_bpd"].double().numpy(), g["prior_bpd"], rtol=1e-4)
    per = max(1, rows // B)
    assert [len(c[1]) for c in model.calls] == [min(per, S - i) * B for i in range(0, S, per)]
    seen = torch.cat([c[1] for c in model.calls]).tolist()
    assert seen == [d.timestep_map[t] for t in g["t"]] and model.calls[0][1].dtype == torch.long
    assert torch.equal(torch.cat([c[0] for c in model.calls]), torch.from_numpy(g["x_t"]))
    assert all(f == (1 if bool(g["clip"]) else 0) for _, _, f in model._engine.vb_calls)
    assert np.array_equal(np.concatenate([c[1] for c in model._engine.vb_calls]), bpd_ref.coef_rows(d, g["t"]))


def test_the_surface_has_the_reference_names_and_refuses_what_it_does_not_evaluate():
    for name in ("q_mean_variance", "q_posterior_mean_variance", "_predict_eps_from_xstart", "_prior_bpd", "_vb_terms_bpd", "calc_bpd_loop"):
        assert hasattr(gd.GaussianDiffusion, name), name
    sig = inspect.signature(gd.GaussianDiffusion.calc_bpd_loop)
    assert list(sig.parameters)[:5] == ["self", "model", "x_start", "clip_denoised", "model_kwargs"] and sig.parameters["clip_denoised"].default is True
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("noise_tape", "seed", "sample_offset", "max_rows_per_call"))
    assert sig.parameters["max_rows_per_call"].default == 256
    sig = inspect.signature(gd.GaussianDiffusion._vb_terms_bpd)
    assert list(sig.parameters) == ["self", "model", "x_start", "x_t", "t", "clip_denoised", "model_kwargs"]
    kw = dict(use_timesteps=space_timesteps(1000, "4"), betas=gd.get_named_beta_schedule("cosine", 1000), loss_type=gd.LossType.MSE)
    x = torch.zeros(2, 5, 6, 8)
    d = SpacedDiffusion(model_mean_type=gd.ModelMeanType.EPSILON, model_var_type=gd.ModelVarType.FIXED_SMALL, **kw)
    with pytest.raises(NotImplementedError, match="x_start"):
        d.calc_bpd_loop(object(), x, model_kwargs={"y": {}})
    d = SpacedDiffusion(model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.LEARNED_RANGE, **kw)
    with pytest.raises(NotImplementedError, match="learned variances"):
        d.calc_bpd_loop(object(), x, model_kwargs={"y": {}})
    d = SpacedDiffusion(model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL, **kw)
    with pytest.raises(KeyError):
        d.calc_bpd_loop(object(), x)
    with pytest.raises(TypeError, match="HIP denoiser"):
        d.calc_bpd_loop(object(), x, model_kwargs={"y": {}})
    d.loss_type = gd.LossType.KL
    with pytest.raises(NotImplementedError):              # training_losses with a KL loss type stays out
        d.training_losses(object(), x, torch.zeros(2, dtype=torch.long))


def test_expand_y_is_what_it_was():
    """repeat_y was factored out of _expand_y: the per-sample entries repeated, masks and lengths cut, the actor motion revealed frame by frame."""
    from regennet_amd.eval.auto_regressive import _expand_y, repeat_y
    B, T = 2, 6
    cm = torch.arange(B * 3 * 2 * T, dtype=torch.float32).reshape(B, 3, 2, T) + 1
    y = {"cmotion": cm, "action": torch.tensor([[4], [5]]), "mask": torch.ones(B, 1, 1, T, dtype=torch.bool), "lengths": torch.tensor([6, 3]),
         "text": ["a", "b"], "scale": torch.tensor([2.5, 1.0]), "flag": True}
    out = _expand_y(y, B, 1, 4, cm, T_call=4)
    assert out["action"].tolist() == [[4], [5]] * 3 and out["text"] == ["a", "b"] * 3 and out["flag"] is True and out["lengths"].tolist() == [4, 3] * 3
    assert tuple(out["mask"].shape) == (6, 1, 1, 4) and tuple(out["cmotion"].shape) == (6, 3, 2, 4)
    for i, f in enumerate(range(1, 4)):
        want = cm.clone()
        want[..., f + 1:] = 0
        assert torch.equal(out["cmotion"][i * B:(i + 1) * B], want[..., :4])
    rep = repeat_y(y, B, 3, T, skip=())
    assert torch.equal(rep["cmotion"], cm.repeat(3, 1, 1, 1)) and rep["lengths"].tolist() == [6, 3] * 3 and "cmotion" not in repeat_y(y, B, 3, T)


def test_the_two_entry_points_are_declared_bound_and_exported():
    from regennet_amd import _lib
    header = open(os.path.join(ROOT, "include", "regennet_hip.h")).read()
    assert re.search(r"RGN_API int rgn_q_sample_rows\(rgn_handle h, const float\* x_start_dev", header)
    assert re.search(r"RGN_API int rgn_vb_terms\(rgn_handle h, const float\* x_start_dev", header)
    assert "gaussian_diffusion.py:1546-1601" in header and "diffusion/losses.py:42-77" in header
    assert len(_lib.SYMBOLS["rgn_q_sample_rows"][1]) == 14 and len(_lib.SYMBOLS["rgn_vb_terms"][1]) == 14
    assert _lib.VB_TERMS == bpd_ref.TERMS and _lib.VB_CLIP == 1
    lib = _lib.load()
    assert hasattr(lib, "rgn_q_sample_rows") and hasattr(lib, "rgn_vb_terms")
    assert "rgn_vb.hip" in __import__("__graft_entry__").SOURCES


def test_argument_checks_need_no_device():
    """Each bad argument is RGN_ERR_INVALID_ARG with its text, before the handle or the device is looked at: the calls below pass a NULL handle and
    non-null dummy 'device' pointers that are never dereferenced."""
    from regennet_amd import _lib
    lib = _lib.load()
    dev = ctypes.cast((ctypes.c_float * 4)(), ctypes.c_void_p)

    def q(x_start=dev, noise=dev, coef=dev, t=dev, B=2, N=4, features=3, T=5, x_t=dev, noise_out=None):
        rc = lib.rgn_q_sample_rows(None, x_start, noise, coef, t, B, N, features, T, 1, 0, x_t, noise_out, None)
        return rc, (lib.rgn_last_error(None) or b"").decode()

    def vb(x_start=dev, x_t=dev, output=dev, noise=dev, t=dev, coef=dev, B=2, N=4, features=3, T=5, flags=1, terms=dev):
        rc = lib.rgn_vb_terms(None, x_start, x_t, output, noise, t, coef, B, N, features, T, flags, terms, None)
        return rc, (lib.rgn_last_error(None) or b"").decode()

    shared = [(dict(x_start=None), "null"), (dict(coef=None), "null"), (dict(t=None), "null"), (dict(x_t=None), "null"), (dict(B=0), "B < 1"),
              (dict(N=0), "N < 1"), (dict(T=0), "T < 1"), (dict(features=0), "features < 1"), (dict(N=5), "no multiple of B = 2"),
              (dict(features=1 << 20, T=4096), "more than 2^31 - 1")]
    for fn, name, extra in ((q, "rgn_q_sample_rows", [(dict(B=1, N=2 ** 31 - 1, features=3, T=100), "more than 2^31 - 1 workgroups"),
                                                     (dict(noise=None, T=4097), "T <= 4096"),
                                                     (dict(noise=None, features=(1 << 19) + 1, T=2), "features <= 2^19")]),
                            (vb, "rgn_vb_terms", [(dict(output=None), "null"), (dict(terms=None), "null"), (dict(flags=2), "unknown flag")])):
        rc, err = fn()
        assert rc == -1 and err == name + ": null handle"                 # everything else passed
        for kw, text in shared + extra:
            rc, err = fn(**kw)
            assert rc == -1 and err.startswith(name + ": ") and text in err, (name, kw, rc, err)
    for kw in (dict(noise=None), dict(noise=None, T=4096, features=2), dict(noise=None, T=2, features=1 << 19), dict(noise_out=dev), dict(B=1, N=1, features=1, T=1), dict(N=65536),
               dict(B=1, N=2 ** 31 - 1, features=16, T=16)):
        assert q(**kw)[1] == "rgn_q_sample_rows: null handle", kw
    assert vb(noise=None, flags=0)[1] == "rgn_vb_terms: null handle"


def test_score_cli_bpd_flag():
    from regennet_amd.utils.parser_util import score_args
    a = score_args(["--synthetic", "--bpd", "--timestep_respacing", "10", "--num_samples", "4", "--batch_size", "3", "--t_grid", "3"])
    assert a.bpd is True and a.t_grid == 3 and a.timestep_respacing == "10"
    assert score_args(["--synthetic", "--skeleton", "synthetic"]).bpd is False
