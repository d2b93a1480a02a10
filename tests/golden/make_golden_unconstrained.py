"""Golden vectors of the unconstrained evaluation's metrics, recorded by RUNNING THE REFERENCE's own functions (CPU; sklearn and tqdm needed).

    python tests/golden/make_golden_unconstrained.py

Loads the reference's eval/unconstrained/metrics/kid.py and precision_recall.py by file path (under _ref_import.REF_ROOT) and writes
tests/golden/unconstrained_pr.npz and unconstrained_kid.npz - DATA only: the features of tests/unconstrained_ref.py's recipe, the numpy seed, the
index arrays the reference drew, its mmds / vars / (mean, std), its precision and recall per k, its deviation from the fp64 restatement, and the
restatement's per-row radii and flags. Nothing of the reference's source travels."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from _ref_import import REF_ROOT  # noqa: E402
from tests import unconstrained_ref as ur  # noqa: E402


def load(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REF_ROOT, "eval", "unconstrained", "metrics", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record_pr(pr):
    out = {}
    for case in ur.PR_CASES:
        real, gen = ur.pr_features(case)
        out[f"{case}_real"], out[f"{case}_gen"] = real, gen
        tr, tg = torch.from_numpy(real), torch.from_numpy(gen)
        for k in ur.PR_KS:
            # the reference's own numbers, on the whole sets (precision: the generated rows inside the real manifold; recall: the other way round)
            prec, rec = pr.manifold_estimate(tr, tg, k), pr.manifold_estimate(tg, tr, k)
            p64, r_real, f_gen = ur.manifold_estimate(real, gen, k)
            r64, r_gen, f_real = ur.manifold_estimate(gen, real, k)
            assert (prec, rec) == (p64, r64), (case, k, prec, rec, p64, r64)          # the reference's values equal the fp64 restatement's exactly
            out[f"{case}_k{k}_precision"], out[f"{case}_k{k}_recall"] = np.float64(prec), np.float64(rec)
            out[f"{case}_k{k}_radii_real"], out[f"{case}_k{k}_radii_gen"] = r_real, r_gen
            out[f"{case}_k{k}_flags_gen"], out[f"{case}_k{k}_flags_real"] = f_gen, f_real
            print(f"[pr {case} k={k}] precision {prec:.4f} recall {rec:.4f}", flush=True)
        out[f"{case}_precision_and_recall"] = np.asarray(pr.precision_and_recall(tg, tr), np.float64)     # k = 3 on the sets cut to the shorter one
    np.savez_compressed(os.path.join(HERE, "unconstrained_pr.npz"), **out)


def record_kid(kid):
    out = {"seed": np.int64(ur.KID_SEED), "n_subsets": np.int64(ur.KID_SUBSETS)}
    real_choice = np.random.choice
    for case, (seed, Nr, Ng, D, subset) in ur.KID_CASES.items():
        real, gen = ur.make_features(seed, Nr, Ng, D)
        drawn = []

        def spy(*a, **kw):
            drawn.append(real_choice(*a, **kw))
            return drawn[-1]

        np.random.seed(ur.KID_SEED)
        np.random.choice = spy               # kid.py:14 takes np.random.choice when it is called: record what it draws
        try:
            mmds, vars_ = kid.polynomial_mmd_averages(real, gen, n_subsets=ur.KID_SUBSETS, subset_size=subset)
        finally:
            np.random.choice = real_choice
        idx_g, idx_r = np.stack(drawn[0::2]).astype(np.int32), np.stack(drawn[1::2]).astype(np.int32)
        m64, v64, bound = ur.poly_mmd(real, gen, idx_g, idx_r)
        fkey = f"features_{seed}_{Nr}_{Ng}_{D}"          # cases on the same feature sets share one copy
        out[fkey + "_real"], out[fkey + "_gen"], out[f"{case}_features"], out[f"{case}_subset"] = real, gen, np.str_(fkey), np.int64(subset)
        out[f"{case}_idx_g"], out[f"{case}_idx_r"] = idx_g, idx_r
        out[f"{case}_mmds"], out[f"{case}_vars"] = mmds, vars_
        out[f"{case}_mean_std"] = np.asarray([mmds.mean(), mmds.std()])
        out[f"{case}_e_ref_mmd"], out[f"{case}_e_ref_var"] = np.abs(mmds - m64).max(), np.abs(vars_ - v64).max()
        print(f"[kid {case}] mmds {mmds.min():.3f}..{mmds.max():.3f} vars {vars_.min():.3f}..{vars_.max():.3f} e_ref_mmd {np.abs(mmds - m64).max():.2e} "
              f"(bound {bound.min():.2e}..{bound.max():.2e}) e_ref_var {np.abs(vars_ - v64).max():.2e}", flush=True)
    np.savez_compressed(os.path.join(HERE, "unconstrained_kid.npz"), **out)


if __name__ == "__main__":
    record_kid(load("kid"))
    record_pr(load("precision_recall"))
