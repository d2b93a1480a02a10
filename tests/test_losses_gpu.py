"""GPU: rgn_loss_terms (csrc/rgn_loss.hip) and diffusion.training_losses against the fp64 restatement that tests/test_losses_cpu.py pins to the
reference.

Bound, per motion and term (the project's rot2xyz convention): the fp32 run of the SAME restatement deviates from its fp64 run by d - the
reference arithmetic at the kernel's precision, computed here on the same inputs, never taken from the kernel. The kernel may associate its
sums and the chain's products differently, which is the same order of error again in either direction, so it must stay within 4 d, with one
fp32 spacing of the value as floor (the kernel's result is an fp32 number). NaN (an empty mask) must be NaN exactly where the restatement's is.
A motion that the input generator reports as undecided (a ground-truth foot speed within 16 d of the threshold, tests/loss_cases.py) is left out
of the fc comparison and reported. REGENNET_LOSS_TABLE=<file> writes the measured table (profiles/loss_terms_parity.txt)."""
import os

import numpy as np
import pytest
import torch

from regennet_amd import _lib, synth
from tests import loss_cases
from tests.losses_ref import FOOT_JOINTS, TERMS, loss_terms_ref, stack_terms

pytestmark = pytest.mark.gpu
TABLE = []
ALL = dict(lambda_rcxyz=1.0, lambda_vel=1.0, lambda_fc=1.0, lambda_orient=1.0, lambda_body=1.0, lambda_transl=1.0)


@pytest.fixture(scope="module")
def engine():
    """One tiny model on the GPU: its engine is the finalized handle every kernel call below runs on."""
    from tests.helpers import build_hip
    cfg = synth.get_config("tiny")
    model, _ = build_hip(cfg, synth.make_state_dict(cfg, seed=0), resp="5")
    eng, _ = model._get_engine(2, cfg["num_frames"])
    yield eng
    if TABLE and os.environ.get("REGENNET_LOSS_TABLE"):
        with open(os.environ["REGENNET_LOSS_TABLE"], "w") as f:
            f.write(f"rgn_loss_terms on {torch.cuda.get_device_name(0)}: |kernel - fp64 restatement| against the bound max(4 x |fp32 restatement - fp64 restatement|, "
                    "1 fp32 spacing), per case and term at the motion with the largest error / bound\n")
            f.write(f"{'case':44s} {'term':10s} {'value':>11s} {'fp32 ref':>10s} {'bound':>10s} {'kernel':>10s}\n")
            for row in TABLE:
                f.write("%-44s %-10s %11.4e %10.3e %10.3e %10.3e%s\n" % row)


def run_kernel(eng, inp, mask, sk, foot, row, thr, flags=_lib.LOSS_FC):
    """Engine.loss_terms on numpy inputs -> numpy [B, 7] fp32."""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    out = torch.full((inp["target"].shape[0], 7), float("nan"), device="cuda")
    eng.loss_terms(dev(inp["target"]), dev(inp["output"]), dev(inp["cmotion"]), dev(mask), sk["rest_joints"], sk["parents"],
                   foot, row, thr, flags, out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def restate(target, output, cmotion, mask, sk, foot, row, thr):
    r64 = stack_terms(loss_terms_ref(target, output, cmotion, mask, sk, thr, foot, row, dtype=torch.float64))
    r32 = stack_terms(loss_terms_ref(target, output, cmotion, mask, sk, thr, foot, row, dtype=torch.float32))
    return r64, r32


def check(label, got, r64, r32, undecided=None, extra=None, truth=None):
    """got [B, 7] within the 4 d rule of r64 (or, with `truth` and `extra` [B, 7], within extra + the rule's bound of `truth`)."""
    assert got.shape == r64.shape and got.dtype == np.float32
    truth = r64 if truth is None else truth
    assert np.array_equal(np.isnan(got), np.isnan(r64)) and np.array_equal(np.isnan(r32), np.isnan(r64)), (label, got, r64)
    failed = []
    for k, term in enumerate(TERMS):
        worst = None
        for b in range(got.shape[0]):
            if np.isnan(r64[b, k]):
                continue
            d = abs(r32[b, k] - r64[b, k])
            bound = max(4 * d, float(np.spacing(np.float32(abs(r64[b, k]))))) + (0.0 if extra is None else float(extra[b, k]))
            err = abs(float(got[b, k]) - truth[b, k])
            skipped = term == "fc" and undecided is not None and bool(undecided[b])
            if not skipped and err > bound:
                failed.append((term, b, err, bound))
            if worst is None or err / bound > worst[0]:
                worst = (err / bound, abs(truth[b, k]), d, bound, err, "  (undecided motion: not compared)" if skipped else "")
        if worst is not None:
            TABLE.append((label, term) + worst[1:])
            print("%-44s %-10s value %.4e  fp32 ref %.3e  bound %.3e  kernel %.3e%s" % ((label, term) + worst[1:]))
    assert not failed, (label, failed)


def test_kernel_fixtures(engine, golden):
    for name in ("losses_k_b3t7", "losses_k_b2t33"):
        g = golden(name)
        sk = {"rest_joints": g["rest_joints"], "parents": g["parents"]}
        inp = {k: g[k] for k in ("target", "output", "cmotion")}
        foot, row, thr = tuple(int(j) for j in g["foot_joints"]), int(g["transl_row"]), float(g["vel_threshold"])
        got = run_kernel(engine, inp, g["mask"], sk, foot, row, thr)
        r64, r32 = restate(inp["target"], inp["output"], inp["cmotion"], g["mask"], sk, foot, row, thr)
        assert float((np.abs(r64 - g["expected"]) / np.abs(g["expected"])).max()) < 1e-12      # (the restatement is the recorded reference run)
        check(name, got, r64, r32, truth=g["expected"])


@pytest.mark.parametrize("B,T,skel,mask_kind,drift,thr,seed", loss_cases.GRID)
def test_grid(engine, B, T, skel, mask_kind, drift, thr, seed):
    J, foot, row = loss_cases.SKELETONS[skel]
    sk = loss_cases.skeleton(skel)
    inp, cond, used = loss_cases.find_inputs(B, T, skel, drift, thr, seed)
    mask = loss_cases.make_mask(mask_kind, B, T, seed)
    got = run_kernel(engine, inp, mask, sk, foot, row, thr)
    r64, r32 = restate(inp["target"], inp["output"], inp["cmotion"], mask, sk, foot, row, thr)
    assert np.isfinite(r64).all()
    check(f"B{B} T{T} {skel} mask={mask_kind} thr={thr}", got, r64, r32, undecided=cond["undecided"])


def test_a_motion_of_length_one_inside_a_batch(engine):
    """Its vel_mse and fc divide 0 by 0 (no frame pair under the mask): NaN exactly where the restatement's are; the other terms of that row are
    finite, and the other rows are what they are without it, bit for bit."""
    B, T = 3, 7
    sk = loss_cases.skeleton("tree55")
    inp, cond, _ = loss_cases.find_inputs(B, T, "tree55", 0.01, 0.03, 31, max_undecided=0)
    mask = np.ones((B, T), bool)
    mask[1, 1:] = False
    got = run_kernel(engine, inp, mask, sk, FOOT_JOINTS, 55, 0.03)
    r64, r32 = restate(inp["target"], inp["output"], inp["cmotion"], mask, sk, FOOT_JOINTS, 55, 0.03)
    nan = np.zeros((B, 7), bool)
    nan[1, [TERMS.index("vel_mse"), TERMS.index("fc")]] = True
    assert np.array_equal(np.isnan(r64), nan) and np.array_equal(np.isnan(got), nan)
    check("B3 T7 one motion of length 1", got, r64, r32)
    full = run_kernel(engine, inp, np.ones((B, T), bool), sk, FOOT_JOINTS, 55, 0.03)
    assert np.array_equal(got[[0, 2]].view(np.int32), full[[0, 2]].view(np.int32))
    none = run_kernel(engine, inp, np.zeros((B, T), bool), sk, FOOT_JOINTS, 55, 0.03)          # no frame at all: 0 / 0 everywhere
    assert np.isnan(none).all()


def test_rows_do_not_depend_on_the_batch_and_runs_are_identical(engine):
    B, T = 5, 65
    sk = loss_cases.skeleton("tree55")
    inp, _, _ = loss_cases.find_inputs(B, T, "tree55", 0.004, 0.01, 41)
    mask = loss_cases.make_mask("ragged", B, T, 41)
    full = run_kernel(engine, inp, mask, sk, FOOT_JOINTS, 55, 0.01)
    again = run_kernel(engine, inp, mask, sk, FOOT_JOINTS, 55, 0.01)
    assert np.isfinite(full).all() and np.array_equal(full.view(np.int32), again.view(np.int32))
    for b in range(B):
        one = run_kernel(engine, {k: v[b:b + 1] for k, v in inp.items()}, mask[b:b + 1], sk, FOOT_JOINTS, 55, 0.01)
        assert np.array_equal(full[b:b + 1].view(np.int32), one.view(np.int32)), b
    off = run_kernel(engine, inp, mask, sk, FOOT_JOINTS, 55, 0.01, flags=0)                    # without RGN_LOSS_FC: the column is 0, the rest unchanged
    keep = [k for k in range(7) if TERMS[k] != "fc"]
    assert np.array_equal(off[:, keep].view(np.int32), full[:, keep].view(np.int32)) and not off[:, TERMS.index("fc")].any()


class _Spy:
    """Stands where DistributedDataParallel stands in the reference's training loop (`enc = model.model.module`): `.module` and a call, which it logs."""

    def __init__(self, module):
        self.module, self.calls = module, []

    def __call__(self, x, ts, **kw):
        out = self.module(x, ts, **kw)
        self.calls.append((x.clone(), ts.clone(), out.clone()))
        return out


def e2e_setup(g, lambdas):
    from tests.helpers import build_hip, fixture_cfg
    cfg = fixture_cfg(g)
    model, diffusion = build_hip(cfg, synth.make_state_dict(cfg, seed=0), resp=str(g["resp"]))
    for k, v in dict(lambdas, vel_threshold=float(g["vel_threshold"]), num_person=1, body_model="smplx", data_rep="rot6d").items():
        setattr(diffusion, k, v)
    sk = {"rest_joints": g["rest_joints"], "parents": g["parents"]}
    model.set_skeleton(sk)
    B, T = g["mask"].shape
    y = {"mask": torch.from_numpy(g["mask"]).reshape(B, 1, 1, T), "cmotion": torch.from_numpy(g["cmotion"]).cuda()}
    if "action" in g:
        y["action"] = torch.from_numpy(g["action"]).cuda()
    return model, diffusion, sk, y


@pytest.mark.parametrize("name", ["losses_e2e_tiny", "losses_e2e_tiny_r50", "losses_e2e_ntu_action"])
def test_training_losses_end_to_end(golden, name):
    """diffusion.training_losses on the recorded inputs: the denoiser saw the reference's x_t and (respaced: mapped) timesteps and answered within
    1e-3 of the reference's output; the returned terms are the restatement's on the device's own output (4 d rule) and lie within the recorded
    sensitivity to that 1e-3 (+ the rule's bound) of the reference's terms."""
    g = golden(name)
    model, diffusion, sk, y = e2e_setup(g, ALL)
    try:
        spy = _Spy(model)
        t = torch.from_numpy(g["t"]).cuda()
        out = diffusion.training_losses(spy, torch.from_numpy(g["target"]).cuda(), t, model_kwargs={"y": y}, noise=torch.from_numpy(g["noise"]).cuda(),
                                        dataset="ntu")
        assert set(out) == set(TERMS) | {"loss"} and all(tuple(v.shape) == t.shape and v.is_cuda for v in out.values())
        (x_t, ts, dev_out), = spy.calls
        assert ts.cpu().tolist() == g["t_model"].tolist() and ts.dtype == torch.long           # the denoiser sees ORIGINAL timesteps
        if str(g["resp"]):
            assert g["t_model"].tolist() != g["t"].tolist() and [diffusion.timestep_map[i] for i in g["t"]] == g["t_model"].tolist()
        assert torch.equal(x_t, diffusion.q_sample(torch.from_numpy(g["target"]).cuda(), t, torch.from_numpy(g["noise"]).cuda()))
        err = float(np.abs(dev_out.cpu().numpy().astype(np.float64) - g["model_output"]).max())
        print(f"{name}: max |device model output - reference's| = {err:.3e}")
        assert err < 1e-3, err
        got = np.stack([out[k].cpu().numpy() for k in TERMS], 1)
        r64, r32 = restate(g["target"], dev_out.cpu().numpy(), g["cmotion"], g["mask"], sk, FOOT_JOINTS, 55, float(g["vel_threshold"]))
        check(name + " (device output)", got, r64, r32)
        check(name + " (reference terms)", got, r64, r32, extra=g["sens"], truth=g["expected"])
        want = got[:, 0] + 0.0 + got[:, 2] + got[:, 1] + got[:, 3] + got[:, 4] + got[:, 5] + got[:, 6]          # all weights 1, the reference's order
        assert np.array_equal(out["loss"].cpu().numpy(), want)
    finally:
        model.set_skeleton(None)
        for e in model._engines.values():
            e.close()


def test_dict_keys_and_loss_weighting(golden):
    """all weights zero; the reference's defaults (orient, body, transl at 1); all positive; dataset=None against dataname='ntu'. The columns do
    not depend on the weights, and loss is their weighted sum in the reference's order."""
    import types
    g = golden("losses_e2e_tiny")
    model, diffusion, sk, y = e2e_setup(g, ALL)
    try:
        args = (model, torch.from_numpy(g["target"]).cuda(), torch.from_numpy(g["t"]).cuda())
        kw = dict(model_kwargs={"y": y}, noise=torch.from_numpy(g["noise"]).cuda())
        base = diffusion.training_losses(*args, dataset=types.SimpleNamespace(dataname="ntu"), **kw)
        sets = {"zero": {k: 0.0 for k in ALL}, "defaults": dict({k: 0.0 for k in ALL}, lambda_orient=1.0, lambda_body=1.0, lambda_transl=1.0),
                "all": dict(lambda_rcxyz=0.5, lambda_vel=2.0, lambda_fc=3.0, lambda_orient=1.0, lambda_body=0.25, lambda_transl=4.0)}
        for label, lam in sets.items():
            for k, v in lam.items():
                setattr(diffusion, k, v)
            for ds in (None, types.SimpleNamespace(dataname="ntu"), "chi3d", "kit"):
                out = diffusion.training_losses(*args, dataset=ds, **kw)
                name = getattr(ds, "dataname", ds)
                keys = {"rot_mse", "loss"} | {k for k in ("rcxyz_mse", "vel_mse", "orient", "body", "transl") if lam["lambda_" + k.replace("_mse", "")] > 0}
                if lam["lambda_fc"] > 0 and name in ("ntu", "chi3d"):
                    keys.add("fc")
                assert set(out) == keys, (label, name, set(out))
                assert all(torch.equal(out[k], base[k]) for k in keys - {"loss"})
                c = lambda k: out[k] if k in out else 0.0                                   # noqa: E731
                want = out["rot_mse"] + 0.0 + lam["lambda_vel"] * c("vel_mse") + lam["lambda_rcxyz"] * c("rcxyz_mse") + lam["lambda_fc"] * c("fc") + \
                    lam["lambda_orient"] * c("orient") + lam["lambda_body"] * c("body") + lam["lambda_transl"] * c("transl")
                assert torch.equal(out["loss"], want), (label, name)
        for k in ALL:
            setattr(diffusion, k, 0.0)
        assert torch.equal(diffusion.training_losses(*args, **kw)["loss"], base["rot_mse"])
    finally:
        model.set_skeleton(None)
        for e in model._engines.values():
            e.close()


def test_score_cli_prints_its_table_and_writes_the_per_motion_values(tmp_path, capsys):
    from regennet_amd.eval import score
    path = score.main(["--synthetic", "--skeleton", "synthetic", "--num_samples", "4", "--batch_size", "3", "--t_grid", "3", "--lambda_fc", "1",
                       "--output_dir", str(tmp_path)])
    text = capsys.readouterr().out
    res = np.load(path, allow_pickle=True).item()
    assert res["timesteps"].tolist() == [0, 500, 999] and set(res) == {"rot_mse", "fc", "orient", "body", "transl", "loss", "timesteps", "lengths"}
    assert all(res[k].shape == (3, 4) and np.isfinite(res[k]).all() for k in ("rot_mse", "fc", "orient", "body", "transl", "loss"))
    lines = [ln.split() for ln in text.splitlines() if ln.split() and ln.split()[0] in ("t", "0", "500", "999")]
    assert lines[0] == ["t", "rot_mse", "fc", "orient", "body", "transl", "loss"] and [ln[0] for ln in lines[1:]] == ["0", "500", "999"]
    assert abs(float(lines[2][-1]) - float(res["loss"][1].mean())) <= 1e-5 * abs(float(res["loss"][1].mean()))
