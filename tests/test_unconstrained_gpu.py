"""GPU: the unconstrained evaluation's metrics on the device (rgn_poly_mmd, rgn_knn_radius, rgn_manifold_hits; regennet_amd/eval/unconstrained.py)
against the goldens the reference's own functions recorded and the fp64 restatement (tests/unconstrained_ref.py).

    radii     |r_dev - r64| <= tau r64 per row, tau = (D + 2) 2^-23: the first-order bound on the disagreement of two fp32 direct-difference
              distances summed in different orders; exactly 0 on the duplicate rows.
    flags     == the golden's for every case, k and direction, and precision_and_recall's two numbers == the reference's: no row of the fixtures is
              undecided at tau (tests/test_unconstrained_cpu.py re-checks that on every run), so membership does not depend on the summation order.
    mmds      within the error model's derived bound of the restatement on the recorded draws.
    vars      within 8 x the case's recorded e_ref_var: the reference's own fp32 deviation from the same restatement on the same draws.
tests/test_unconstrained_cpu.py shows that these bounds tell the mutants apart. REGENNET_UNCONSTRAINED_TABLE=<file> writes the measured table
(profiles/unconstrained_parity.txt).

On the commit before the feature every test here fails: regennet_amd.eval.unconstrained does not exist."""
import os

import numpy as np
import pytest
import torch

from tests import unconstrained_ref as ur

pytestmark = pytest.mark.gpu
VAR_MARGIN = 8
_TABLE = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _kid_case(g, case):
    fkey = str(g[f"{case}_features"])
    return g[fkey + "_real"], g[fkey + "_gen"], g[f"{case}_idx_g"], g[f"{case}_idx_r"]


@pytest.fixture(scope="module")
def kid64(golden):
    g = golden("unconstrained_kid")
    return {case: ur.poly_mmd(*_kid_case(g, case)) for case in ur.KID_CASES}


def _write_table():
    path = os.environ.get("REGENNET_UNCONSTRAINED_TABLE")
    if path and _TABLE:
        with open(path, "w") as f:
            f.write("\n".join(_TABLE[k] for k in sorted(_TABLE)) + "\n")


# ---- precision / recall ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ur.PR_CASES))
def test_radii_flags_and_counts(golden, case):
    from regennet_amd.eval import unconstrained as un
    g = golden("unconstrained_pr")
    real, gen = g[f"{case}_real"], g[f"{case}_gen"]
    dr, dg = _dev(real), _dev(gen)
    t = ur.tau(real.shape[1])
    worst = 0.0
    for k in ur.PR_KS:
        for A, B, tagA, tagB in ((dr, dg, "real", "gen"), (dg, dr, "gen", "real")):
            r64 = g[f"{case}_k{k}_radii_{tagA}"]
            radii = un.knn_radius(A, k)
            assert radii.dtype == torch.float32 and tuple(radii.shape) == (len(A),)
            r = radii.cpu().numpy().astype(np.float64)
            assert np.all(np.abs(r - r64) <= t * r64), (case, k, tagA, np.abs(r - r64).max())
            worst = max(worst, float((np.abs(r - r64)[r64 > 0] / (t * r64[r64 > 0])).max()))
            assert np.array_equal(r == 0, r64 == 0)
            flags, count = un.manifold_hits(B, A, radii)
            assert flags.dtype == torch.uint8 and count.dtype == torch.int32
            want = g[f"{case}_k{k}_flags_{tagB}"]
            assert np.array_equal(flags.cpu().numpy().astype(bool), want), (case, k, tagB, np.flatnonzero(flags.cpu().numpy().astype(bool) != want))
            assert int(count.item()) == int(want.sum())
            # two calls agree bit for bit
            assert torch.equal(un.knn_radius(A, k), radii)
            f2, c2 = un.manifold_hits(B, A, radii)
            assert torch.equal(f2, flags) and torch.equal(c2, count)
        assert un.manifold_estimate(dr, dg, k) == float(g[f"{case}_k{k}_precision"])
        assert un.manifold_estimate(dg, dr, k) == float(g[f"{case}_k{k}_recall"])
    assert un.precision_and_recall(dg, dr) == tuple(g[f"{case}_precision_and_recall"])
    if case == "duplicates":
        for k in (1, 3):
            assert torch.all(un.knn_radius(dr, k)[:4] == 0)               # four identical rows: the radii are exactly 0 ...
            assert bool(un.manifold_hits(dg[:1], dr[:4], un.knn_radius(dr, k)[:4])[0][0])      # ... and d = 0 <= 0 is a hit
        assert un.precision_and_recall(dg, dr)[0] == 0.425
    _TABLE[f"1 pr {case}"] = "%-14s radii: worst |r - r64| / (tau r64) = %.3e over k = 1, 3, 8 and both sets; flags, counts, precision and recall equal the reference's" % (case, worst)
    _write_table()


# ---- KID ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ur.KID_CASES))
def test_mmds_and_vars_on_the_recorded_draws(golden, kid64, case):
    from regennet_amd.eval import unconstrained as un
    g = golden("unconstrained_kid")
    real, gen, idx_g, idx_r = _kid_case(g, case)
    dr, dg = _dev(real), _dev(gen)
    m64, v64, bound = kid64[case]
    mmds, vars_ = un.poly_mmd(dr, dg, idx_g, idx_r)
    assert mmds.dtype == vars_.dtype == torch.float64 and mmds.is_cuda
    m2, v2 = un.poly_mmd(dr, dg, idx_g, idx_r)
    assert torch.equal(m2, mmds) and torch.equal(v2, vars_)                # bit for bit
    mmds, vars_ = mmds.cpu().numpy(), vars_.cpu().numpy()
    e_ref_var = float(g[f"{case}_e_ref_var"])
    rm, ev = (np.abs(mmds - m64) / bound).max(), np.abs(vars_ - v64).max()
    line = "%-14s mmds: worst error / derived bound = %.3e (error %.3e, bound %.3e)   vars: worst error %.3e = %.2f x e_ref_var (%.3e; tolerance 8 x)" % (
        case, rm, np.abs(mmds - m64).max(), bound.min(), ev, ev / e_ref_var, e_ref_var)
    if ev > e_ref_var:
        line += "   ABOVE 1 x e_ref_var"
    print("\n" + line)
    _TABLE[f"0 kid {case}"] = line
    _write_table()
    assert np.all(np.abs(mmds - m64) <= bound), (np.abs(mmds - m64), bound)
    assert ev <= VAR_MARGIN * e_ref_var, (ev, e_ref_var)


@pytest.mark.parametrize("case", list(ur.KID_CASES))
def test_calculate_kid_draws_and_matches_the_reference(golden, kid64, case):
    """The whole Python path: the same np.random.seed draws the reference's rows, and (mean, std) lands on the reference's pair. The golden pair is
    the reference's fp32 result, e_ref_mmd from the restatement; the device is within `bound` of it; the population std is 1-Lipschitz in the
    largest entry error, like the mean."""
    from regennet_amd.eval import unconstrained as un
    g = golden("unconstrained_kid")
    real, gen, _, _ = _kid_case(g, case)
    subset = int(g[f"{case}_subset"])
    np.random.seed(ur.KID_SEED)
    mean, std = un.calculate_kid(_dev(real), _dev(gen), n_subsets=ur.KID_SUBSETS, subset_size=subset)
    tol = kid64[case][2].max() + float(g[f"{case}_e_ref_mmd"])
    assert abs(mean - g[f"{case}_mean_std"][0]) <= tol and abs(std - g[f"{case}_mean_std"][1]) <= tol
    np.random.seed(ur.KID_SEED)
    mmds, vars_ = un.polynomial_mmd_averages(_dev(real), _dev(gen), n_subsets=ur.KID_SUBSETS, subset_size=subset)
    assert isinstance(mmds, np.ndarray) and mmds.dtype == np.float64
    assert np.all(np.abs(mmds - kid64[case][0]) <= kid64[case][2])
    assert np.abs(vars_ - kid64[case][1]).max() <= VAR_MARGIN * float(g[f"{case}_e_ref_var"])


def test_a_subset_larger_than_the_set_raises(golden):
    from regennet_amd.eval import unconstrained as un
    seed, Nr, Ng, D, subset = ur.KID_VALUE_ERROR
    real, gen = ur.make_features(seed, Nr, Ng, D)
    np.random.seed(ur.KID_SEED)
    with pytest.raises(ValueError, match="larger sample than population"):
        un.polynomial_mmd_averages(_dev(real), _dev(gen), n_subsets=ur.KID_SUBSETS, subset_size=subset)
    with pytest.raises(ValueError, match="outside its feature set"):
        un.poly_mmd(_dev(real), _dev(gen), np.full((1, 10), Nr, np.int32), np.zeros((1, 10), np.int32))


def test_other_kernel_arguments(golden, kid64):
    """degree, gamma and coef0 other than the defaults (the bound is the same model's), and one subset of three rows: the smallest the variance
    estimate takes."""
    from regennet_amd.eval import unconstrained as un
    g = golden("unconstrained_kid")
    real, gen, idx_g, idx_r = _kid_case(g, "replace")
    for kw in (dict(degree=2, gamma=0.01, coef0=0.5), dict(degree=1, gamma=0.02, coef0=0.0), dict(degree=4, gamma=None, coef0=1)):
        for ig, ir in ((idx_g, idx_r), (idx_g[:1, :3], idx_r[:1, :3])):
            m64, v64, bound = ur.poly_mmd(real, gen, ig, ir, **kw)
            mmds, vars_ = un.poly_mmd(_dev(real), _dev(gen), ig, ir, **kw)
            assert np.all(np.abs(mmds.cpu().numpy() - m64) <= bound), (kw, ig.shape)
            assert np.all(np.isfinite(vars_.cpu().numpy()))


# ---- the evaluation ------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_unconstrained_metrics(golden):
    from regennet_amd.eval import calculate_activation_statistics, calculate_fid
    from regennet_amd.eval import unconstrained as un
    g = golden("unconstrained_pr")
    dr, dg = _dev(g["n130_real"]), _dev(g["n130_gen"])
    np.random.seed(3)
    m = un.evaluate_unconstrained_metrics(dg, dr, kid_subsets=4, kid_subset_size=100)
    assert sorted(m) == ["diversity_gen", "diversity_gt", "fid", "kid", "precision", "recall"]
    assert m["fid"] == float(calculate_fid(calculate_activation_statistics(dg), calculate_activation_statistics(dr)))
    assert (m["precision"], m["recall"]) == tuple(g["n130_precision_and_recall"])
    assert all(np.isfinite(m[k]) and m[k] > 0 for k in ("kid", "diversity_gen", "diversity_gt"))
    # the draws come in the reference's order: KID, then the dataset's diversity, then the generated set's
    np.random.seed(3)
    kid = un.calculate_kid(dr, dg, n_subsets=4, subset_size=100)
    div_gt, div_gen = un.calculate_diversity(dr), un.calculate_diversity(dg)
    assert (m["kid"], m["diversity_gt"], m["diversity_gen"]) == (kid[0], div_gt.item(), div_gen.item())
    np.random.seed(3)
    fast = un.evaluate_unconstrained_metrics(dg, dr, fast=True, kid_subsets=4, kid_subset_size=100)
    assert fast["precision"] is None and fast["recall"] is None and fast["kid"] == m["kid"]
    # the reference's own default subset of 1000 does not fit 130 features: numpy's error, as there
    with pytest.raises(ValueError):
        un.evaluate_unconstrained_metrics(dg, dr)


def test_calculate_diversity_is_the_reference_sum(golden):
    from regennet_amd.eval import unconstrained as un
    g = golden("unconstrained_pr")
    act = g["n97x80_real"]
    np.random.seed(11)
    got = un.calculate_diversity(_dev(act)).item()
    np.random.seed(11)
    first, second = np.random.randint(0, len(act), 200), np.random.randint(0, len(act), 200)
    want = np.linalg.norm(act[first].astype(np.float64) - act[second].astype(np.float64), axis=1).sum() / 200
    assert abs(got - want) <= ur.tau(act.shape[1]) * want            # fp32 distances and an fp32 sum of 200 of them against fp64


def test_evaluation_evaluate_unconstrained_end_to_end(golden):
    """Evaluation.evaluate_unconstrained over synthetic 'gt' and 'gen' loaders without labels: ONE recogniser forward per batch, every metric produced."""
    from regennet_amd import synth
    from regennet_amd.eval import Evaluation
    sd = synth.make_stgcn_state_dict(golden("stgcn")["A"], num_class=26, seed=0)
    ev = Evaluation("ntu", "smplx", {"nfeats": 12, "num_classes": 26, "num_person": 2,
                                     "state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}, "cuda:0", seed=7)
    rng = np.random.Generator(np.random.PCG64(3))

    def loader(shift):
        return [{"output": torch.from_numpy((rng.standard_normal((16, 56, 12, 60)) + shift).astype(np.float32)).cuda()} for _ in range(2)]

    calls, fwd = [], ev.model.forward
    ev.model.forward = lambda b: (calls.append(1), fwd(b))[1]
    m = ev.evaluate_unconstrained({"gt": loader(0.0), "gen": loader(0.3)}, kid_subsets=3, kid_subset_size=32)
    ev.model.forward = fwd
    assert len(calls) == 4
    assert sorted(m) == ["diversity_gen", "diversity_gt", "fid", "kid", "precision", "recall"]
    assert all(np.isfinite(m[k]) for k in m) and m["fid"] > 0 and 0 <= m["precision"] <= 1 and 0 <= m["recall"] <= 1
