"""rgn_hml_to_joints (csrc/rgn_hml.hip) on the device against the fp64 restatement of the reference's hml_vec post-processing (tests/hml_ref.py),
element for element, at every fixture and at synthetic shapes; what the call promises beside its values; and the two CLIs end to end.

THE BOUND (derived in tests/hml_ref.py's module text, from the host model and the number formats, never from the kernel's output):
    |kernel - restatement| <= 2^-23 |restatement| + (T + 16) 2^-52 A
- the one rounding to fp32, plus fp64 sums of at most T terms in any order, plus sincos and the rotation's handful of operations - with A the
absolute-sum companion of the element's recurrences. Shapes: T = 1, 2, 63, 64, 65, 196, 257 and 300 (past the kernel's chunk of 256 frames) and 1100
(above 1024); J = 2, 21, 22; B = 1 and 5."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import hml_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("hml_t196", "hml_kit_t65", "hml_t1", "hml_t2", "hml_raw_t64")
# (B, J, T, raw)
SHAPES = [(1, 22, 1, False), (5, 22, 2, False), (1, 21, 63, False), (5, 22, 64, True), (1, 2, 65, False), (5, 21, 196, False), (1, 22, 257, False),
          (5, 2, 300, True), (1, 22, 1100, False)]
CHILD_TIME_LIMIT = 240       # seconds, per child process


@pytest.fixture(scope="module")
def engine():
    from regennet_amd.sample.render import postprocessing_engine
    model, eng = postprocessing_engine(torch.device("cuda", 0))
    yield eng
    torch.cuda.synchronize()
    model._engine.close()


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        raw = bool(z["raw"])
        return z["x"], (None if raw else z["mean"]), (None if raw else z["std"]), z["expected"]


def run(engine, x, mean=None, std=None):
    from regennet_amd.utils.hml import hml_to_joints
    out = hml_to_joints(torch.from_numpy(np.ascontiguousarray(x)).cuda(), mean, std, engine=engine)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check(tag, got, x, mean, std):
    T = x.shape[-1]
    ref = hml_ref.hml_joints_ref(x, mean, std)
    bound = hml_ref.gpu_bound(ref, hml_ref.error_model(x, mean, std), T)
    assert got.dtype == np.float32 and got.shape == ref.shape
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)
    print(f"{tag}: max |kernel - restatement| {err.max():.3e}, / bound {ratio.max():.4f}")
    assert np.isfinite(got).all() and (err <= bound).all(), (tag, float(ratio.max()))
    return ref


@pytest.mark.parametrize("name", FIXTURES)
def test_kernel_equals_the_restatement_at_every_fixture(engine, name):
    x, mean, std, expected = load_fixture(name)
    got = run(engine, x, mean, std)
    check(name, got, x, mean, std)
    # ... and sits as close to the reference's own fp32 run as that run's model allows
    both = hml_ref.gamma32(x.shape[-1]) * hml_ref.error_model(x, mean, std) + 2.0 ** -23 * np.abs(expected)
    assert (np.abs(got.astype(np.float64) - expected) <= both).all()


@pytest.mark.parametrize("B,J,T,raw", SHAPES)
def test_kernel_equals_the_restatement_at_synthetic_shapes(engine, B, J, T, raw):
    x, mean, std = hml_ref.make_inputs(B, hml_ref.rows_of(J), T, seed=100 + 7 * T + J, raw=raw)
    check(f"B{B} J{J} T{T}{' raw' if raw else ''}", run(engine, x, mean, std), x, mean, std)


@pytest.mark.parametrize("J,T", [(22, 196), (21, 300)])
def test_rows_of_a_batch_equal_single_motion_calls_bit_for_bit(engine, J, T):
    x, mean, std = hml_ref.make_inputs(5, hml_ref.rows_of(J), T, seed=31)
    batch = run(engine, x, mean, std)
    for b in range(5):
        assert np.array_equal(batch[b], run(engine, x[b:b + 1], mean, std)[0]), b
    assert np.array_equal(batch, run(engine, x, mean, std))            # and the same on every run


@pytest.mark.parametrize("J,T", [(22, 65), (2, 300)])
def test_rows_past_the_local_positions_are_never_read(engine, J, T):
    x, mean, std = hml_ref.make_inputs(2, hml_ref.rows_of(J), T, seed=32)
    clean = run(engine, x, mean, std)
    first_unread = 3 * (J - 1) + 4
    x, mean, std = x.copy(), mean.copy(), std.copy()
    x[:, first_unread:], mean[first_unread:], std[first_unread:] = np.nan, np.nan, np.nan
    assert np.array_equal(run(engine, x, mean, std), clean)
    assert np.array_equal(run(engine, x), run(engine, np.nan_to_num(x)))      # without statistics too


def test_recover_from_ric_has_the_reference_layouts(engine):
    from regennet_amd.utils.hml import hml_to_joints, recover_from_ric
    x, _, _ = hml_ref.make_inputs(3, 263, 65, seed=33, raw=True)
    xd = torch.from_numpy(x).cuda()
    want = hml_to_joints(xd, engine=engine).permute(0, 3, 1, 2)                      # [B, T, J, 3]
    data = xd[:, :, 0].permute(0, 2, 1).contiguous()                                  # [B, T, D]
    got3 = recover_from_ric(data, 22, engine=engine)
    got4 = recover_from_ric(data[:, None], 22, engine=engine)                         # [B, 1, T, D], the shape cgenerate.py:150-151 hands over
    assert tuple(got3.shape) == (3, 65, 22, 3) and tuple(got4.shape) == (3, 1, 65, 22, 3)
    assert torch.equal(got3, want) and torch.equal(got4[:, 0], want)
    with pytest.raises(ValueError, match="joints_num"):
        recover_from_ric(data, 21, engine=engine)


def test_a_captured_graph_replays_the_eager_call(engine):
    x, mean, std = hml_ref.make_inputs(5, 263, 300, seed=34)
    xd, md, sd = (torch.from_numpy(a).cuda() for a in (x, mean, std))
    out = torch.empty((5, 22, 3, 300), device="cuda")

    def call():
        engine.hml_to_joints(xd, md, sd, 22, out, torch.cuda.current_stream().cuda_stream)

    call()
    torch.cuda.synchronize()
    eager = out.cpu().numpy()
    out.fill_(float("nan"))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), eager)


def test_device_side_refusals(engine):
    from regennet_amd import _lib
    from regennet_amd.utils.hml import hml_to_joints
    with pytest.raises(ValueError, match="12 J - 1"):
        hml_to_joints(torch.zeros(1, 56, 1, 8, device="cuda"), engine=engine)
    with pytest.raises(ValueError, match=r"\[B, D, 1, T\]"):
        hml_to_joints(torch.zeros(1, 263, 6, 8, device="cuda"), engine=engine)
    x, out = torch.zeros(1, 263, 1, 4097, device="cuda"), torch.zeros(1, 22, 3, 4097, device="cuda")
    with pytest.raises(_lib.RgnError, match="T = 4097 outside"):
        engine.hml_to_joints(x, None, None, 22, out, 0)


CHILD = ["--synthetic", "--dataset", "humanml", "--layers", "1", "--latent_dim", "64", "--timestep_respacing", "ddim5", "--use_ddim", "--motion_length", "40",
         "--num_samples", "2", "--num_repetitions", "1"]


def child(module, extra, out_dir):
    r = subprocess.run([sys.executable, "-m", module] + CHILD + extra + ["--output_dir", str(out_dir)], cwd=ROOT, capture_output=True, text=True,
                       timeout=CHILD_TIME_LIMIT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(os.path.join(str(out_dir), "results.npy"), allow_pickle=True).item(), r.stdout


def joints_match(tag, motion, features):
    ref = hml_ref.hml_joints_ref(features)
    bound = hml_ref.gpu_bound(ref, hml_ref.error_model(features), features.shape[-1])
    assert motion.dtype == np.float32 and motion.shape == ref.shape, (tag, motion.shape)
    assert (np.abs(motion.astype(np.float64) - ref) <= bound).all(), tag


def test_cgenerate_stores_the_joints_of_its_own_output(tmp_path):
    d, stdout = child("regennet_amd.sample.cgenerate", [], tmp_path)
    assert d["output"].shape == (2, 263, 1, 40) and d["cmotion"].shape == (2, 263, 1, 40) and d["motion"].shape == (2, 22, 3, 40) and list(d["lengths"]) == [40, 40]
    assert "taken as already de-normalised" in stdout
    joints_match("cgenerate", d["motion"], d["output"])


def test_edit_upper_body_keeps_the_lower_body_rows_bit_for_bit(tmp_path):
    from regennet_amd.data_loaders.humanml_utils import HML_LOWER_BODY_MASK
    d, _ = child("regennet_amd.sample.edit", ["--edit_mode", "upper_body"], tmp_path)
    out, inp, mask = d["output"], d["input_motions"], d["mask"]
    assert out.shape == inp.shape == mask.shape == (2, 263, 1, 40) and all(np.array_equal(mask[b, :, 0, t], HML_LOWER_BODY_MASK) for b in range(2) for t in (0, 39))
    assert np.array_equal(out[mask].view(np.uint32), inp[mask].view(np.uint32))          # the kept rows of the input, in the unsmoothed sample
    assert not np.array_equal(out[~mask], inp[~mask])                                    # ... and the rest was generated
    joints_match("edit motion", d["motion"], out)
    joints_match("edit input_motion", d["input_motion"], inp)
