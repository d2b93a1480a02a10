"""CPU: what the GRU action classifier promises without a GPU - the fp64 restatement reproduces the reference's recorded outputs, the parity bound of
tests/test_gru_gpu.py separates the right arithmetic from the nearest wrong one, the modules carry the reference's state-dict names, the engine refuses
the geometries it does not serve, and the action2motion evaluation draws the reference's indices."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import gru_ref

GOLDEN = gru_ref.GOLDEN


@pytest.mark.parametrize("name", list(gru_ref.CASES))
def test_restatement_reproduces_the_reference(name):
    """|fp64 restatement - the reference's fp32 outputs| is ref_err by construction; recomputed here from the seeds it must come out within 2 x ref_err
    (the weights, inputs and the restatement are this checkout's, the outputs the reference's)."""
    fx = gru_ref.load_fixture(name)
    sd, x, ln, h0 = gru_ref.case_inputs(name)
    assert np.array_equal(ln, fx["lengths"]) and int(fx["seed"]) == gru_ref.CASE_SEEDS[name]
    assert ln.min() >= 1 and ln.max() <= x.shape[-1]
    if name in ("ha12", "ha12_hot"):
        assert ln[0] == 1 and ln[1] == 60
    if name == "long":
        assert ln.max() == 200
    f64, l64 = gru_ref.gru_forward(sd, x, ln, h0)
    assert np.abs(f64 - fx["features"]).max() <= 2 * fx["ref_err"][0]
    assert np.abs(l64 - fx["logits"]).max() <= 2 * fx["ref_err"][1]
    top = np.sort(l64, axis=1)
    assert (top[:, -1] - top[:, -2]).min() >= 1e-4 if l64.shape[1] > 1 else True


@pytest.mark.parametrize("name", ["ha12", "ha12_hot"])
def test_bf16_mutants_lie_far_outside_the_bound(name):
    """One bf16 rounding of any one operand - the nearest wrong arithmetic - misses the GPU test's bound by at least 10 x (also at the largest factor
    the bound may ever take, 32): the bound does tell a single-plane bf16 kernel from an fp32 one."""
    fx = gru_ref.load_fixture(name)
    sd, x, ln, h0 = gru_ref.case_inputs(name)
    f64, _ = gru_ref.gru_forward(sd, x, ln, h0)
    for operand in ("W_hh", "W_ih", "h", "x"):
        fm, _ = gru_ref.gru_forward(sd, x, ln, h0, mutant=operand)
        err = np.abs(fm - f64).max()
        print(f"{name} bf16({operand}): features off by {err:.2e}, bound {gru_ref.bound(fx['ref_err'][0]):.2e}")
        assert err >= 10 * gru_ref.bound(fx["ref_err"][0], factor=32.0), (operand, err)


def test_state_dict_names_and_shapes_are_the_references():
    from regennet_amd.eval import gru
    keys = json.load(open(os.path.join(GOLDEN, "gru_keys.json")))
    for cls in (gru.MotionDiscriminator, gru.MotionDiscriminatorForFID):
        m = cls(72, 128, 2, device="cpu", output_size=12)
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == keys


def test_load_state_dict_refuses_a_wrong_shape():
    from regennet_amd import synth
    from regennet_amd.eval import gru
    sd = {k: torch.from_numpy(v) for k, v in synth.make_gru_state_dict().items()}
    m = gru.MotionDiscriminator(72, 128, 2, device="cpu", output_size=12)
    m.load_state_dict(sd)
    bad = dict(sd)
    bad["recurrent.weight_ih_l0"] = torch.zeros(384, 71)
    with pytest.raises(RuntimeError, match="size mismatch"):
        m.load_state_dict(bad)
    with pytest.raises(RuntimeError, match="Missing key"):
        m.load_state_dict({k: v for k, v in sd.items() if k != "linear2.bias"})


def _create(**over):
    from regennet_amd import _lib
    lib = _lib.load()
    c = dict(input_size=72, hidden_size=128, num_layers=2, lin1_size=30, output_size=12, device=0)
    c.update(over)
    h = ctypes.c_void_p()
    rc = lib.rgn_gru_create(ctypes.byref(_lib.RgnGruConfig(**c)), ctypes.byref(h))
    err = (lib.rgn_gru_last_error(None) or b"").decode()
    if rc == 0:
        assert lib.rgn_gru_destroy(h) == 0
    return rc, err


REFUSED = [(dict(hidden_size=0), "hidden_size"), (dict(hidden_size=16), "hidden_size"), (dict(hidden_size=100), "hidden_size"),
           (dict(hidden_size=288), "hidden_size"), (dict(num_layers=0), "num_layers"), (dict(num_layers=5), "num_layers"),
           (dict(input_size=0), "input_size"), (dict(input_size=1025), "input_size"), (dict(lin1_size=0), "lin1_size"),
           (dict(lin1_size=65), "lin1_size"), (dict(output_size=0), "output_size"), (dict(output_size=1025), "output_size")]
ACCEPTED = [dict(hidden_size=h, num_layers=l, input_size=i, lin1_size=f, output_size=c)
            for h in range(32, 257, 32) for l, i, f, c in ((1, 1, 1, 1), (2, 72, 30, 12), (4, 1024, 64, 1024), (3, 54, 30, 13))]


def test_rgn_gru_create_refuses_what_no_kernel_serves_and_accepts_the_rest():
    """The geometry check runs before the device is touched: the same answers with and without a GPU; an accepted geometry gets as far as the device."""
    for over, word in REFUSED:
        rc, err = _create(**over)
        assert rc == -7 and err.startswith("rgn_gru_create: ") and word in err, (over, rc, err)
    for over in ACCEPTED:
        rc, err = _create(**over)
        assert rc == 0 or (rc == -6 and "no HIP device" in err), (over, rc, err)
    from regennet_amd import _lib
    lib = _lib.load()
    assert lib.rgn_gru_create(None, None) == -1 and b"null" in lib.rgn_gru_last_error(None)
    assert lib.rgn_gru_destroy(None) == -1 and lib.rgn_gru_finalize(None) == -1
    assert lib.rgn_gru_forward(None, 1, 1, None, None, None, None, None, None) == -1 and b"null x" in lib.rgn_gru_last_error(None)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_gpu_means_loud_failure_not_fallback():
    from regennet_amd.eval import gru
    m = gru.MotionDiscriminator(72, 128, 2, device="cpu", output_size=12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 24, 3, 8), lengths=torch.tensor([8, 8]))


class _StubClassifier:
    """features = a fixed projection of the motion's mean pose, logits peaked at the label the motion was built with."""

    def __init__(self):
        self.proj = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).standard_normal((72, 30)).astype(np.float32))

    def forward_both(self, x, lengths=None, hidden_unit=None, **kw):
        assert tuple(hidden_unit.shape) == (2, x.shape[0], 128)
        feats = torch.tanh(x.mean(dim=3).reshape(x.shape[0], -1) @ self.proj)
        return feats, torch.nn.functional.one_hot((feats[:, 0] > 0).long() + 3, 12).float()


def _reference_draws(feats, labels, num_labels, with_labels):
    """diversity.py:20-71 restated draw by draw, distances by torch.dist one pair at a time."""
    n = feats.shape[0]
    first, second = np.random.randint(0, n, 200), np.random.randint(0, n, 200)
    diversity = sum(torch.dist(feats[a], feats[b]) for a, b in zip(first, second)) / 200
    if not with_labels:
        return diversity.item(), float("nan")
    mm, quotas = 0, np.zeros(num_labels)
    quotas[np.unique(labels.numpy())] = 20
    while np.any(quotas > 0):
        a = np.random.randint(0, n)
        if not quotas[labels[a]]:
            continue
        b = np.random.randint(0, n)
        while labels[a] != labels[b]:
            b = np.random.randint(0, n)
        quotas[labels[a]] -= 1
        mm += torch.dist(feats[a], feats[b])
    return diversity.item(), (mm / (20 * num_labels)).item()


@pytest.mark.parametrize("cond_mode", ["action", "no_cond"])
def test_a2m_evaluation_draws_the_references_indices(cond_mode):
    from regennet_amd.eval import a2m

    class Model:
        pass

    Model.cond_mode = cond_mode
    loaders = a2m.synthetic_loaders(50, batch_size=16, seed=3, device="cpu")
    stub = _StubClassifier()
    got = a2m.A2MEvaluation("cpu", seed=21, classifier=stub).evaluate(Model, loaders)
    np.random.seed(21)
    for key, loader in loaders.items():
        feats = torch.cat([stub.forward_both(b["output_xyz"], hidden_unit=torch.zeros(2, len(b["output_xyz"]), 128))[0] for b in loader])
        labels = torch.cat([b["y"] for b in loader])
        d, m = _reference_draws(feats, labels, 12, cond_mode == "action")
        assert got[f"diversity_{key}"] == pytest.approx(d, rel=1e-5)
        if cond_mode == "action":
            assert got[f"multimodality_{key}"] == pytest.approx(m, rel=1e-5)
            pred = (feats[:, 0] > 0).long() + 3
            assert got[f"accuracy_{key}"] == pytest.approx((pred == labels).float().mean().item())
        else:
            assert np.isnan(got[f"multimodality_{key}"]) and np.isnan(got[f"accuracy_{key}"])
    assert got["fid_gt"] == pytest.approx(0.0, abs=1e-6) and got["fid_gen"] > 1e-3      # (the fp64 eigen-solver's residue of a set against itself: ~1e-8)
    assert set(got) == {f"{m}_{k}" for m in ("accuracy", "diversity", "multimodality", "fid") for k in ("gen", "gt", "gt2")}


def test_synthetic_checkpoint_is_seeded_and_in_the_default_init_range():
    from regennet_amd import synth
    a, b, c = synth.make_gru_state_dict(seed=1), synth.make_gru_state_dict(seed=1), synth.make_gru_state_dict(seed=2, scale=3.0)
    assert all(np.array_equal(a[k], b[k]) for k in a) and not np.array_equal(a["linear1.weight"], c["linear1.weight"])
    assert np.abs(a["recurrent.weight_hh_l1"]).max() <= 1 / np.sqrt(128) and np.abs(c["recurrent.weight_hh_l1"]).max() > 1 / np.sqrt(128)
