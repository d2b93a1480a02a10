"""GPU: the text-to-motion evaluator on the device (regennet_amd.eval.t2m, rgn_t2m.hip) against the fp64 restatement of tests/t2m_ref.py under the
project's parity rule max(8 x the reference's own fp32 error, 2^-20); row independence, dead frames and clamped lengths bit for bit; the matching
kernel; and regennet_amd.eval.humanml end to end against what the reference's eval_humanml.py returned (tests/golden/t2m_eval.npz).

Measured on an MI355X, error / bound per case and output: profiles/t2m_eval_parity.txt."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from regennet_amd import _lib
from regennet_amd.eval import humanml, t2m
from tests import t2m_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_KEYS = dict(dim_pose="dim_pose", movement_hidden="dim_movement_enc_hidden", movement_latent="dim_movement_latent", motion_hidden="dim_motion_hidden",
                dim_word="dim_word", dim_pos_ohot="dim_pos_ohot", text_hidden="dim_text_hidden", coemb="dim_coemb_hidden")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(wrapper, inputs, fp64 movements, fp64 motion embeddings, fp64 text embeddings, fixture), computed once and never written to"""
    sds, inp = t2m_ref.case_inputs(name)
    geo = t2m_ref.CASES[name][0]
    w = t2m.EvaluatorMDMWrapper("kit" if geo["dim_pose"] == 251 else "humanml", DEV, state_dicts=sds, **{OPT_KEYS[k]: v for k, v in geo.items()})
    mov64, motion64 = t2m_ref.motion_side(sds, inp["motions"], inp["m_lens"])
    text64 = t2m_ref.text_side(sds, inp["word_embs"], inp["pos_ohot"], inp["cap_lens"])
    return w, inp, mov64, motion64, text64, t2m_ref.load_fixture(name)


def _dev(inp, **over):
    d = dict(inp, **over)
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in d.items()}


def _co(w, d, keep_order=True):
    text, motion = w.get_co_embeddings(d["word_embs"], d["pos_ohot"], d["cap_lens"], d["motions"], d["m_lens"], keep_order=keep_order)
    return text.cpu().numpy(), motion.cpu().numpy()


@pytest.mark.parametrize("name", list(t2m_ref.CASES))
def test_every_fixture_is_within_the_parity_bound(name):
    w, inp, mov64, motion64, text64, fx = _case(name)
    d = _dev(inp)
    text, motion = _co(w, d)
    mov = w.movement_encoder(d["motions"][..., :-4], d["m_lens"]).cpu().numpy()
    assert not w.lengths_clamped() and not w.movement_encoder.lengths_clamped()
    live = t2m_ref.live_mask(inp["m_lens"], mov.shape[1])
    errs = (np.abs(mov - mov64)[live].max(), np.abs(motion - motion64).max(), np.abs(text - text64).max())
    for what, e, r in zip(t2m_ref.OUTPUTS, errs, fx["ref_err"]):
        print(f"t2m parity {name:6s} {what:10s} err {e:.3e} bound {t2m_ref.bound(r):.3e} ratio {e / t2m_ref.bound(r):.3f}")
    for what, e, r in zip(t2m_ref.OUTPUTS, errs, fx["ref_err"]):
        assert e <= t2m_ref.bound(r), (name, what, e, t2m_ref.bound(r))
    assert (mov[~live] == 0).all()                            # frames the recurrence never reads are not computed
    # the stand-alone modules: every movement frame, and the motion encoder on movements
    full = w.movement_encoder(d["motions"][..., :-4]).cpu().numpy()
    assert np.abs(full - mov64).max() <= t2m_ref.bound(fx["ref_err"][0]) and (full[live] == mov[live]).all()
    alone = w.motion_encoder(torch.from_numpy(full).to(DEV), d["m_lens"] // 4).cpu().numpy()
    assert (alone == motion).all()
    assert (w.text_encoder(d["word_embs"], d["pos_ohot"], d["cap_lens"]).cpu().numpy() == text).all()


def test_rows_do_not_depend_on_the_batch():
    w, inp, *_ = _case("t2m")
    text, motion = _co(w, _dev(inp))
    for n in (0, 1, 15, 16, 17, 32):
        t1, m1 = _co(w, _dev({k: v[n:n + 1] for k, v in inp.items()}))
        assert (t1[0] == text[n]).all() and (m1[0] == motion[n]).all(), n
    perm = np.random.Generator(np.random.PCG64(5)).permutation(len(text))
    tp, mp = _co(w, _dev({k: v[perm] for k, v in inp.items()}))
    assert (tp == text[perm]).all() and (mp == motion[perm]).all()


def test_the_wrapper_returns_the_reference_row_order():
    w, inp, *_ = _case("t2m")
    d = _dev(inp)
    text, motion = _co(w, d)
    ts, ms = _co(w, d, keep_order=False)
    align = np.argsort(inp["m_lens"].tolist())[::-1].copy()          # evaluator_wrapper.py:160
    assert (ts == text[align]).all() and (ms == motion[align]).all()
    only = w.get_motion_embeddings(d["motions"], d["m_lens"]).cpu().numpy()
    assert (only == motion[align]).all()


@pytest.mark.parametrize("name", ["t2m", "odd_T"])
def test_nothing_past_the_receptive_field_is_looked_at(name):
    w, inp, *_ = _case(name)
    text, motion = _co(w, _dev(inp))
    motions, word, pos = inp["motions"].copy(), inp["word_embs"].copy(), inp["pos_ohot"].copy()
    for n in range(len(motions)):
        motions[n, 4 * (inp["m_lens"][n] // 4) + 3:] = np.nan
        word[n, inp["cap_lens"][n]:] = np.nan
        pos[n, inp["cap_lens"][n]:] = np.nan
    assert np.isnan(motions).any() or name == "odd_T"
    tn, mn = _co(w, _dev(inp, motions=motions, word_embs=word, pos_ohot=pos))
    assert np.isfinite(tn).all() and np.isfinite(mn).all()
    assert (tn == text).all() and (mn == motion).all()


def test_a_length_out_of_range_is_clamped_and_flagged():
    w, inp, *_ = _case("small")
    text, motion = _co(w, _dev(inp))
    assert not w.lengths_clamped()
    m_lens, cap_lens = inp["m_lens"].copy(), inp["cap_lens"].copy()
    m_lens[2], cap_lens[3] = 10000, 0
    tc, mc = _co(w, _dev(inp, m_lens=m_lens, cap_lens=cap_lens))
    assert w.lengths_clamped() and not w.lengths_clamped()
    keep_m, keep_t = np.arange(len(text)) != 2, np.arange(len(text)) != 3
    assert (mc[keep_m] == motion[keep_m]).all() and (tc[keep_t] == text[keep_t]).all()
    assert np.isfinite(tc).all() and np.isfinite(mc).all()
    full = inp["m_lens"].copy()
    full[2] = inp["motions"].shape[1]                                # 10000 clamps to every movement frame
    assert (_co(w, _dev(inp, m_lens=full))[1][2] == mc[2]).all()


@pytest.mark.parametrize("name", list(t2m_ref.MATCH_CASES))
def test_match_ranks_equal_the_fp64_restatement(name):
    text, motion = t2m_ref.match_inputs(name)
    fx = dict(np.load(os.path.join(t2m_ref.GOLDEN, f"t2m_match_{name}.npz")))
    diag, rank = _lib.t2m_match(torch.from_numpy(text).to(DEV), torch.from_numpy(motion).to(DEV), 32)
    diag, rank = diag.cpu().numpy(), rank.cpu().numpy()
    allow = t2m_ref.match_bound(fx["diag"].max())
    print(f"t2m match {name}: diag err {np.abs(diag - fx['diag']).max():.3e} allowance {allow:.3e} margin {float(fx['margin']):.3e}")
    assert float(fx["margin"]) > 64 * allow                          # the condition under which equal ranks may be demanded of every row
    assert (rank == fx["rank"]).all()
    assert np.abs(diag - fx["diag"]).max() <= allow


def test_evaluation_end_to_end_against_the_reference(tmp_path):
    """regennet_amd.eval.humanml.evaluation on the metric case (64 ground-truth + 64 generated motions at the real geometry, served through
    array_loader in the recorded batch order; seeded index draws, two replications, multimodality on) against what the reference's eval_humanml.py
    returned for the same arrays (tests/golden/t2m_eval.npz)."""
    fx = dict(np.load(os.path.join(t2m_ref.GOLDEN, "t2m_eval.npz")))
    sds, gt, gen = t2m_ref.eval_inputs()
    w = t2m.EvaluatorMDMWrapper("humanml", DEV, state_dicts=sds)
    order, aligned = t2m_ref.eval_order(gt["cap_lens"], gt["m_lens"])
    texts = (gt["word_embs"][order], gt["pos_ohot"][order], gt["cap_lens"][order])
    gt_loader = humanml.array_loader(*texts, gt["motions"][order], gt["m_lens"][order], device=DEV)
    gen_loader = humanml.array_loader(*texts, gen[order], gt["m_lens"][order], device=DEV)
    mm = [(torch.from_numpy(m).to(DEV)[None], torch.from_numpy(l).to(DEV)[None]) for m, l in t2m_ref.eval_mm(gen, gt["m_lens"])]
    ranks = []
    mean = humanml.evaluation(w, gt_loader, {"vald": lambda: (gen_loader, mm)}, str(tmp_path / "eval.log"), replication_times=2,
                              diversity_times=t2m_ref.EVAL_DIVERSITY_TIMES, mm_num_times=t2m_ref.EVAL_MM_TIMES, run_mm=True, seed=t2m_ref.EVAL_SEED,
                              ranks=ranks)
    assert not w.lengths_clamped()
    for tag, name in (("gt", "ground truth"), ("gen", "vald")):          # per-row ranks, every row (the margin condition was asserted at recording)
        for rep in ranks:
            assert np.array_equal(rep[name].cpu().numpy(), fx[f"rank_{tag}"][aligned]), name
        assert np.array_equal(mean["R_precision_" + name], fx["mean_R_precision_" + name.replace(" ", "_")])
    # matching score, diversity and multimodality: the project's parity rule against the fp64 restatement on the same index pairs
    # (tests/t2m_ref.eval_metrics64), ref_err the reference's own error against it
    for k in t2m_ref.EVAL_METRICS:
        f64, bound = float(fx["f64_" + k.replace(" ", "_")]), t2m_ref.bound(fx["ref_err_" + k.replace(" ", "_")])
        print(f"t2m eval {k:28s} {float(mean[k]):.7f} fp64 {f64:.7f} err {abs(float(mean[k]) - f64):.2e} bound {bound:.2e}")
    for k in t2m_ref.EVAL_METRICS:
        f64, bound = float(fx["f64_" + k.replace(" ", "_")]), t2m_ref.bound(fx["ref_err_" + k.replace(" ", "_")])
        assert abs(float(mean[k]) - f64) <= bound, (k, float(mean[k]), f64, bound)
    # FID against the reference's scipy value: the project's tolerance (tests/test_host_logic_cpu.py) for the generated set. A set against itself is
    # rank-deficient (64 x 512): there the reference's sqrtm leaves |FID(gt, gt)| = 2e-5 where the value is 0 - its own error - and the device value
    # is held to 8 x that
    ref = float(fx["mean_FID_vald"])
    print(f"t2m eval FID_vald {float(mean['FID_vald']):.7f} reference {ref:.7f} diff {abs(float(mean['FID_vald']) - ref):.2e}")
    assert abs(float(mean["FID_vald"]) - ref) <= 1e-6 * max(1.0, abs(ref))
    ref = float(fx["mean_FID_ground_truth"])
    print(f"t2m eval FID_ground truth {float(mean['FID_ground truth']):.7f} reference {ref:.7f}")
    assert abs(float(mean["FID_ground truth"])) <= 8 * abs(ref)
    assert len(mean) == sum(k.startswith("mean_") for k in fx) == 9 and sum(k.startswith("f64_") for k in fx) == 5


def test_cli_synthetic_in_a_fresh_process(tmp_path):
    r = subprocess.run([sys.executable, "-m", "regennet_amd.eval.humanml", "--synthetic", "--num_samples", "64", "--output_dir", str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = np.load(tmp_path / "metrics.npy", allow_pickle=True).item()
    for family in ("Matching Score", "R_precision", "FID", "Diversity", "MultiModality"):
        assert any(k.startswith(family + "_") for k in m), (family, sorted(m))
    assert all(np.isfinite(np.asarray(v)).all() for v in m.values())
    # (a rank-deficient 64 x 512 set against itself leaves the fp64 eigen-solver's residue, 1e-5 of a trace of 90)
    assert abs(float(m["FID_ground truth"])) < 1e-3 and float(m["FID_vald"]) > 1e-1
