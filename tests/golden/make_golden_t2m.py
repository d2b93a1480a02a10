"""Golden vectors of the text-to-motion evaluator, recorded by RUNNING THE REFERENCE's own modules on the CPU (build machine only).

    python tests/golden/make_golden_t2m.py

Imports the reference's data_loaders/humanml/networks/{modules,evaluator_wrapper}.py, data_loaders/humanml/utils/metrics.py and eval/eval_humanml.py
through _ref_import, writes the synthetic checkpoints of regennet_amd.synth.make_t2m_state_dicts as a finest.tar into a scratch directory and lets the
reference's EvaluatorMDMWrapper load it (strict). Writes DATA only:

  t2m_<case>.npz  per case of tests/t2m_ref.CASES: the reference's fp32 `movements` (of the rows tests/t2m_ref.movement_rows names; frames below m_lens // 4, zeros elsewhere), `motion_emb` and
                  `text_emb` in INPUT order, `ref_err` = max |reference fp32 - fp64 restatement| per output, digests of the inputs. Asserted: every
                  embedding has max-abs in [1, 4].
  t2m_match_<case>.npz  the fp64 diagonal, ranks and margin of tests/t2m_ref.MATCH_CASES, with the ranks of the reference's own metrics.py. Asserted:
                  in EVERY row each |d[i, j] - d[i, i]| exceeds 64 x the device's allowance (2^-20 of the largest distance), and about half the
                  true pairs rank first.
  t2m_eval.npz    the metric case (tests/t2m_ref.eval_inputs): what eval_humanml.evaluation returned (mean_dict) for seeded index draws, the
                  per-row ranks of both loaders, the fp32 embeddings, the log; `f64_<metric>`, the fp64 restatement of matching score, diversity and
                  multimodality on the same index pairs (tests/t2m_ref.eval_metrics64), and `ref_err_<metric>`, the reference's own error against it. Asserted: the same margin condition on the fp64 embeddings.
  t2m_keys.json   key names and shapes of the reference's three state dicts at the HumanML3D geometry.

Inputs and weights are NOT stored: tests regenerate them from the seeds (tests/t2m_ref.case_inputs)."""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
from tests import t2m_ref  # noqa: E402


def import_ref_eval():
    """the reference's eval/eval_humanml.py; its data-set and distributed imports (never run here) get inert stand-ins"""
    import types
    for m in ("spacy", "blobfile", "mpi4py"):
        sys.modules.setdefault(m, types.ModuleType(m))
    if not hasattr(sys.modules["mpi4py"], "MPI"):
        sys.modules["mpi4py"].MPI = None
    from eval import eval_humanml
    return eval_humanml


def digest(inp):
    h = hashlib.sha256()
    for k in sorted(inp):
        h.update(np.ascontiguousarray(inp[k]).tobytes())
    return np.frombuffer(h.digest()[:8], np.uint8).copy()


def ref_wrapper(sds, dataset_name, geo, scratch):
    """the reference's EvaluatorMDMWrapper on a finest.tar written from `sds` (its geometry patched where a case is not the real one)"""
    from data_loaders.humanml.networks import evaluator_wrapper as ew
    ckpt_dir = "t2m" if dataset_name == "humanml" else dataset_name
    d = os.path.join(scratch, ckpt_dir, "text_mot_match", "model")
    os.makedirs(d, exist_ok=True)
    ck = {k: {kk: torch.from_numpy(vv) for kk, vv in v.items()} for k, v in sds.items()}
    ck["epoch"] = 0
    torch.save(ck, os.path.join(d, "finest.tar"))
    cwd = os.getcwd()
    os.chdir(scratch)
    try:
        real = geo["movement_hidden"] == 512
        if real:
            w = ew.EvaluatorMDMWrapper(dataset_name, "cpu")
        else:
            w = object.__new__(ew.EvaluatorMDMWrapper)
            w.opt = {"dataset_name": dataset_name, "device": "cpu", "dim_word": geo["dim_word"], "dim_pos_ohot": geo["dim_pos_ohot"],
                     "dim_motion_hidden": geo["motion_hidden"], "dim_text_hidden": geo["text_hidden"], "dim_coemb_hidden": geo["coemb"],
                     "dim_pose": geo["dim_pose"], "dim_movement_enc_hidden": geo["movement_hidden"], "dim_movement_latent": geo["movement_latent"],
                     "checkpoints_dir": ".", "unit_length": 4}
            w.device = "cpu"
            w.text_encoder, w.motion_encoder, w.movement_encoder = ew.build_evaluators(w.opt)
            for m in (w.text_encoder, w.motion_encoder, w.movement_encoder):
                m.eval()
    finally:
        os.chdir(cwd)
    return w


def ref_outputs(w, inp):
    """(movements, motion_emb, text_emb) of the reference in input order. The reference wants the text rows sorted by cap_lens and sorts the motions
    itself; both orders are undone here."""
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    with torch.no_grad():
        order = np.argsort(-inp["cap_lens"], kind="stable")
        text = np.empty((len(order), w.opt["dim_coemb_hidden"]), np.float32)
        text[order] = w.text_encoder(t["word_embs"][order], t["pos_ohot"][order], t["cap_lens"][order]).numpy()
        align = np.argsort(inp["m_lens"].tolist())[::-1].copy()
        motion = np.empty_like(text)
        motion[align] = w.get_motion_embeddings(t["motions"], t["m_lens"]).numpy()
        mov = w.movement_encoder(t["motions"][..., :-4]).numpy()
    return mov, motion, text


def record_cases(scratch):
    for name, (geo, N, T, Lw, scale, out_scale) in t2m_ref.CASES.items():
        sds, inp = t2m_ref.case_inputs(name)
        dataset = "kit" if geo["dim_pose"] == 251 else "humanml"
        w = ref_wrapper(sds, dataset, geo, os.path.join(scratch, name))
        if name == "t2m":
            keys = {part: {k: list(v.shape) for k, v in m.state_dict().items()}
                    for part, m in (("movement_encoder", w.movement_encoder), ("text_encoder", w.text_encoder), ("motion_encoder", w.motion_encoder))}
            with open(os.path.join(HERE, "t2m_keys.json"), "w") as f:
                json.dump(keys, f, indent=1, sort_keys=True)
        mov, motion, text = ref_outputs(w, inp)
        mov64, motion64 = t2m_ref.motion_side(sds, inp["motions"], inp["m_lens"])
        text64 = t2m_ref.text_side(sds, inp["word_embs"], inp["pos_ohot"], inp["cap_lens"])
        live = t2m_ref.live_mask(inp["m_lens"], mov.shape[1])
        ref_err = np.array([np.abs(mov - mov64)[live].max(), np.abs(motion - motion64).max(), np.abs(text - text64).max()])
        for what, e in (("motion_emb", motion), ("text_emb", text)):
            m = float(np.abs(e).max())
            assert 1.0 <= m <= 4.0, (name, what, m)
        rows = t2m_ref.movement_rows(N)                      # the whole array would pass the size limit of a committed file
        mov = np.where(live[..., None], mov, 0.0).astype(np.float32)[rows]
        np.savez_compressed(os.path.join(HERE, f"t2m_{name}.npz"), movements=mov, motion_emb=motion.astype(np.float32), text_emb=text.astype(np.float32),
                            ref_err=ref_err, seed=np.int64(t2m_ref.CASE_SEEDS[name]), m_lens=inp["m_lens"], cap_lens=inp["cap_lens"], digest=digest(inp))
        print(f"{name:6s} N {N:3d} T {T:3d} Lw {Lw:2d}  ref_err movements {ref_err[0]:.2e} motion {ref_err[1]:.2e} text {ref_err[2]:.2e}  "
              f"max|emb| {np.abs(motion).max():.2f} {np.abs(text).max():.2f}")


def record_match():
    from data_loaders.humanml.utils import metrics as ref_metrics
    for name, (N, D, seed, _) in t2m_ref.MATCH_CASES.items():
        text, motion = t2m_ref.match_inputs(name)
        diag, rank, margin = t2m_ref.match(text, motion)
        allow = t2m_ref.match_bound(diag.max())
        assert margin > 64 * allow, (name, margin, 64 * allow)
        first = float((rank == 0).mean())
        assert 0.35 <= first <= 0.65, (name, first)
        ref_rank = np.zeros(N, np.int64)
        for g0 in range(0, N, 32):
            order = np.argsort(ref_metrics.euclidean_distance_matrix(text[g0:g0 + 32], motion[g0:g0 + 32]), axis=1)
            ref_rank[g0:g0 + 32] = np.argmax(order == np.arange(order.shape[0])[:, None], axis=1)
        assert (ref_rank == rank).all(), name
        ref_diag = ref_metrics.calculate_matching_score(text, motion)
        np.savez(os.path.join(HERE, f"t2m_match_{name}.npz"), diag=diag, rank=rank, margin=np.float64(margin), ref_diag=ref_diag.astype(np.float32),
                 digest=digest({"t": text, "m": motion}))
        print(f"match {name}: N {N} D {D}  true pair first in {first:.2f}  margin {margin:.3e} >= 64 x {allow:.3e}")


def eval_batches(gt, motions):
    """eval_humanml's 7-tuples of 32, text rows sorted by length inside a batch as the reference's collate leaves them"""
    out = []
    for b0 in range(0, t2m_ref.EVAL_N, 32):
        idx = b0 + np.argsort(-gt["cap_lens"][b0:b0 + 32], kind="stable")
        out.append((torch.from_numpy(gt["word_embs"][idx]), torch.from_numpy(gt["pos_ohot"][idx]), None, torch.from_numpy(gt["cap_lens"][idx]),
                    torch.from_numpy(motions[idx]), torch.from_numpy(gt["m_lens"][idx]), None))
    return out


def record_eval(scratch):
    import contextlib
    import io
    ref_eval = import_ref_eval()
    from data_loaders.humanml.utils import metrics as ref_metrics
    sds, gt, gen = t2m_ref.eval_inputs()
    w = ref_wrapper(sds, "humanml", t2m_ref.CASES["t2m"][0], os.path.join(scratch, "eval"))
    gt_loader, gen_loader = eval_batches(gt, gt["motions"]), eval_batches(gt, gen)
    mm = t2m_ref.eval_mm(gen, gt["m_lens"])
    mm_loader = [(torch.from_numpy(m)[None], torch.from_numpy(l)[None]) for m, l in mm]
    log = os.path.join(scratch, "eval.log")
    np.random.seed(t2m_ref.EVAL_SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        mean = ref_eval.evaluation(w, gt_loader, {"vald": lambda: (gen_loader, mm_loader)}, log, replication_times=2,
                                   diversity_times=t2m_ref.EVAL_DIVERSITY_TIMES, mm_num_times=t2m_ref.EVAL_MM_TIMES, run_mm=True)
    out = {"mean_" + k.replace(" ", "_"): np.asarray(v) for k, v in mean.items()}
    lines = [ln for ln in open(log).read().splitlines() if not ln.startswith("Time:")]
    # per-row ranks (input order) and the margin condition, from the reference's fp32 embeddings and the fp64 restatement's
    t64 = t2m_ref.text_side(sds, gt["word_embs"], gt["pos_ohot"], gt["cap_lens"])
    for tag, motions in (("gt", gt["motions"]), ("gen", gen)):
        _, me, te = ref_outputs(w, dict(gt, motions=motions))
        rank = np.zeros(t2m_ref.EVAL_N, np.int64)
        for g0 in range(0, t2m_ref.EVAL_N, 32):
            order = np.argsort(ref_metrics.euclidean_distance_matrix(te[g0:g0 + 32], me[g0:g0 + 32]), axis=1)
            rank[g0:g0 + 32] = np.argmax(order == np.arange(32)[:, None], axis=1)
        _, m64 = t2m_ref.motion_side(sds, motions, gt["m_lens"])
        diag, rank64, margin = t2m_ref.match(t64, m64)
        assert (rank64 == rank).all(), tag
        allow = t2m_ref.match_bound(diag.max())
        assert margin > 64 * allow, (tag, margin, 64 * allow)
        out[f"rank_{tag}"], out[f"emb_{tag}"], out["text"] = rank, me.astype(np.float32), te.astype(np.float32)
        top = (rank[:, None] < np.arange(1, 4)[None, :]).mean(0)
        assert np.allclose(top, mean["R_precision_" + ("ground truth" if tag == "gt" else "vald")]), tag
        print(f"eval {tag}: margin {margin:.3e} >= 64 x {allow:.3e}")
    # the fp64 restatement of the scalar metrics on the same index pairs, and the reference's own error against it
    f64 = t2m_ref.eval_metrics64()
    for k in t2m_ref.EVAL_METRICS:
        out["f64_" + k.replace(" ", "_")] = np.float64(f64[k])
        out["ref_err_" + k.replace(" ", "_")] = np.float64(abs(float(mean[k]) - f64[k]))
        print(f"eval {k:28s} reference {float(mean[k]):.7f} fp64 {f64[k]:.7f} ref_err {abs(float(mean[k]) - f64[k]):.2e}")
    np.savez_compressed(os.path.join(HERE, "t2m_eval.npz"), log=np.array("\n".join(lines)), **out)
    for k, v in mean.items():
        print("eval", k, v)


def main():
    _ref_import.install()
    torch.set_num_threads(4)
    with tempfile.TemporaryDirectory() as scratch:
        what = sys.argv[1:] or ["cases", "match", "eval"]
        if "cases" in what:
            record_cases(scratch)
        if "match" in what:
            record_match()
        if "eval" in what:
            record_eval(scratch)


if __name__ == "__main__":
    main()
