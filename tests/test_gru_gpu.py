"""GPU: the GRU action classifier (rgn_gru_forward behind regennet_amd.eval.gru) against the fp64 restatement of tests/gru_ref.py on the fixtures
tests/golden/make_golden_gru.py recorded from the reference's own classes, and the action2motion evaluation built on it.

The parity bound is max(8 x ref_err, 2^-20) per case and output, ref_err being the REFERENCE's fp32 error against fp64 as the fixture stores it: the
factor covers another fp32 summation order (MFMA k-blocks against the CPU's BLAS) and hardware exp / rcp at ~1 ulp against libm over up to 2 x 200
recurrent applications. Measured on an MI355X (profiles/gru_eval_parity.txt): at most 0.19 of the bound.
Without the feature every test here fails at import or at a missing symbol."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import gru_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"

_cache = {}


def _case(name):
    """(model, x, lengths, h0 on the device, fp64 features, fp64 logits, fixture) - computed once per case and shared."""
    if name not in _cache:
        from regennet_amd.eval import gru
        I, H, L, C, N, T, scale, _ = gru_ref.CASES[name]
        sd, x, ln, h0 = gru_ref.case_inputs(name)
        fx = gru_ref.load_fixture(name)
        assert np.array_equal(fx["lengths"], ln)
        model = gru.MotionDiscriminator(I, H, L, device=DEV, output_size=C)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        model = model.to(DEV).eval()
        f64, l64 = gru_ref.gru_forward(sd, x, ln, h0)
        _cache[name] = (model, torch.from_numpy(x).to(DEV), torch.from_numpy(ln).to(DEV), torch.from_numpy(h0).to(DEV), f64, l64, fx)
    return _cache[name]


@pytest.mark.parametrize("name", list(gru_ref.CASES))
def test_every_fixture_within_the_bound_and_argmax_equal(name):
    model, x, ln, h0, f64, l64, fx = _case(name)
    feats, logits = model.forward_both(x, ln, h0)
    feats, logits = feats.double().cpu().numpy(), logits.double().cpu().numpy()
    ef, el = np.abs(feats - f64).max(), np.abs(logits - l64).max()
    bf, bl = gru_ref.bound(fx["ref_err"][0]), gru_ref.bound(fx["ref_err"][1])
    print(f"gru parity {name:9s} features {ef:.3e} (bound {bf:.3e})  logits {el:.3e} (bound {bl:.3e})  vs reference fp32 "
          f"{np.abs(feats - fx['features']).max():.3e} / {np.abs(logits - fx['logits']).max():.3e}")
    assert np.all(np.abs(feats - f64) <= bf), (ef, bf)
    assert np.all(np.abs(logits - l64) <= bl), (el, bl)
    assert np.array_equal(logits.argmax(1), l64.argmax(1))
    assert not model.lengths_clamped()


def test_rows_do_not_depend_on_the_batch():
    model, x, ln, h0, *_ = _case("ha12")
    feats, logits = model.forward_both(x, ln, h0)
    for n in (0, 1, 15, 16, 17, 32):
        f1, l1 = model.forward_both(x[n:n + 1], ln[n:n + 1], h0[:, n:n + 1])
        assert torch.equal(f1[0], feats[n]) and torch.equal(l1[0], logits[n]), n


def test_frames_past_the_length_are_never_looked_at():
    model, x, ln, h0, *_ = _case("ha12")
    feats, logits = model.forward_both(x, ln, h0)
    xn = x.clone()
    for n, l in enumerate(ln.tolist()):
        xn[n, :, :, l:] = float("nan")
    fn, lg = model.forward_both(xn, ln, h0)
    assert torch.equal(fn, feats) and torch.equal(lg, logits)
    assert not torch.isnan(fn).any()


def test_one_output_alone_equals_both():
    from regennet_amd.eval import gru
    model, x, ln, h0, *_ = _case("ha12")
    feats, logits = model.forward_both(x, ln, h0)
    assert torch.equal(model(x, ln, h0), logits)
    fid = gru.MotionDiscriminatorForFID(72, 128, 2, device=DEV, output_size=12)
    fid.load_state_dict(model.state_dict())
    fid = fid.to(DEV).eval()
    assert torch.equal(fid(x, ln, h0), feats)
    f_only, none = model.forward_both(x, ln, h0, want_logits=False)
    assert none is None and torch.equal(f_only, feats)


def test_a_length_out_of_range_is_clamped_and_flagged():
    model, x, ln, h0, *_ = _case("small")
    feats, logits = model.forward_both(x, torch.full_like(ln, x.shape[-1]), h0)
    bad = torch.full_like(ln, x.shape[-1])
    bad[3] = x.shape[-1] + 5
    fb, lb = model.forward_both(x, bad, h0)           # a device tensor: read by the kernel alone
    assert model.lengths_clamped() and not model.lengths_clamped()
    assert torch.equal(fb, feats) and torch.equal(lb, logits)
    with pytest.raises(ValueError, match="lengths"):
        model.forward_both(x, bad.cpu(), h0)


def test_drawn_hidden_state_follows_the_torch_seed():
    model, x, ln, *_ = _case("small")
    torch.manual_seed(5)
    a = model(x, ln)
    torch.manual_seed(5)
    b = model(x, ln)
    torch.manual_seed(6)
    c = model(x, ln)
    assert torch.equal(a, b) and not torch.equal(a, c)
    torch.manual_seed(5)
    h = torch.randn(1, x.shape[0], 32, device=DEV)
    assert torch.equal(model(x, ln, h), a)


class _Fp64Classifier:
    """The fp64 restatement behind the classifier's forward_both."""

    def __init__(self, sd):
        self.sd, self.close_rows = sd, 0

    def forward_both(self, x, lengths=None, hidden_unit=None, **kw):
        f, l = gru_ref.gru_forward(self.sd, x.cpu().numpy(), lengths.cpu().numpy(), hidden_unit.cpu().numpy())
        top = np.sort(l, axis=1)
        self.close_rows += int((top[:, -1] - top[:, -2] <= 2 * gru_ref.bound(2e-7)).sum())       # rows whose argmax the logit bound does not fix
        return torch.from_numpy(f).to(x.device), torch.from_numpy(l).to(x.device)


def test_a2m_evaluation_equals_the_fp64_restatement():
    from regennet_amd import synth
    from regennet_amd.eval import a2m
    sd = synth.make_gru_state_dict(seed=3)
    loaders = a2m.synthetic_loaders(96, batch_size=32, seed=11, device=DEV)

    class Model:
        cond_mode = "action"

    ev = a2m.A2MEvaluation(DEV, state_dict=sd, seed=7)
    got = ev.evaluate(Model(), loaders)
    ref = a2m.A2MEvaluation(DEV, state_dict=sd, seed=7, classifier=_Fp64Classifier(sd))
    want = ref.evaluate(Model(), loaders)
    assert set(got) == {f"{m}_{k}" for m in ("accuracy", "diversity", "multimodality", "fid") for k in ("gen", "gt", "gt2")}
    # features differ by at most e = 2^-20-ish per element (the parity bound; 8 x 1.8e-7 = 1.4e-6 at this geometry). A pair distance moves by at most
    # 2 sqrt(30) e; FID's mean term by the same order and its covariance terms by O(e |f|): 1e-4 is two orders above all of them and two below the
    # metrics themselves. The index draws are the seed's, so nothing else differs. Accuracy is exact except for rows whose fp64 top-2 logit gap is
    # within twice the logit bound (normally none): only those may flip.
    for k in want:
        if k.startswith("accuracy"):
            assert abs(got[k] - want[k]) <= ref.gru_classifier.close_rows / 96 + 1e-7, (k, got[k], want[k])
        else:
            assert abs(got[k] - want[k]) <= 1e-4 * max(1.0, abs(want[k])), (k, got[k], want[k])
    assert got["fid_gt"] == pytest.approx(0.0, abs=1e-6)


def test_cli_synthetic_run_writes_the_metrics(tmp_path):
    out = tmp_path / "metrics.npy"
    r = subprocess.run([sys.executable, "-m", "regennet_amd.eval.a2m", "--synthetic", "--num_samples", "64", "--output_dir", str(tmp_path)], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = np.load(out, allow_pickle=True).item()
    for k in ("accuracy_gen", "fid_gen", "fid_gt2", "diversity_gt", "multimodality_gen"):
        assert k in m["feats"] and len(m["feats"][k]) == 1, (k, m)
    assert "fid_gen" in r.stdout
