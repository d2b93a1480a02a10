"""CPU: the unconstrained evaluation's metrics (KID, precision / recall) without a GPU - the fp64 restatement (tests/unconstrained_ref.py) against the
goldens the reference's own functions recorded (tests/golden/make_golden_unconstrained.py), the fixture condition the GPU test's exact comparison
rests on, the index draws, the C-ABI's argument checks with no device, the refusal of CPU tensors, and the MUTANTS: host-model variants of either
metric that must fall outside the bounds tests/test_unconstrained_gpu.py holds the kernels to (REGENNET_UNCONSTRAINED_MUTANTS=<file> writes the
table, profiles/unconstrained_mutants.txt).

On the commit before the feature every test that touches the package fails: regennet_amd.eval.unconstrained does not exist and the library has
none of the symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import unconstrained_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rgn_poly_mmd_workspace", "rgn_poly_mmd", "rgn_knn_radius", "rgn_manifold_hits")
VAR_MARGIN = 8          # vars: within 8 x the reference's own fp32 deviation from the restatement (the issue's yardstick)


def kid_case(g, case):
    fkey = str(g[f"{case}_features"])
    return g[fkey + "_real"], g[fkey + "_gen"], g[f"{case}_idx_g"], g[f"{case}_idx_r"]


@pytest.fixture(scope="module")
def kid64(golden):
    """The restatement of every KID case, computed once: case -> (mmds, vars, bound)."""
    g = golden("unconstrained_kid")
    return {case: ur.poly_mmd(*kid_case(g, case)) for case in ur.KID_CASES}


# ---- the restatement against the goldens ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ur.KID_CASES))
def test_kid_restatement_reproduces_the_reference(golden, kid64, case):
    g = golden("unconstrained_kid")
    real, gen, idx_g, idx_r = kid_case(g, case)
    seed, Nr, Ng, D, subset = ur.KID_CASES[case]
    r2, g2 = ur.make_features(seed, Nr, Ng, D)
    assert np.array_equal(real, r2) and np.array_equal(gen, g2)          # the recorded features are the recipe's
    assert idx_g.shape == idx_r.shape == (ur.KID_SUBSETS, subset) and int(g["seed"]) == ur.KID_SEED
    mmds, vars_, bound = kid64[case]
    assert np.all(np.abs(g[f"{case}_mmds"] - mmds) <= bound), (np.abs(g[f"{case}_mmds"] - mmds), bound)
    assert np.abs(g[f"{case}_mmds"] - mmds).max() == float(g[f"{case}_e_ref_mmd"])
    assert np.abs(g[f"{case}_vars"] - vars_).max() == float(g[f"{case}_e_ref_var"]) > 0
    assert np.array_equal(g[f"{case}_mean_std"], [g[f"{case}_mmds"].mean(), g[f"{case}_mmds"].std()])


def test_kid_cases_cover_replacement_and_permutation(golden):
    g = golden("unconstrained_kid")
    ig = g["replace_idx_g"]
    assert any(len(np.unique(row)) < len(row) for row in ig)                                 # duplicate rows inside a subset
    assert all(sorted(row) == list(range(70)) for row in g["permutation_idx_g"])             # replace=False over the whole set: a permutation
    assert any(len(np.unique(row)) < 50 for row in g["subset50_idx_g"])                       # 50 < 70: with replacement again (kid.py:16)


@pytest.mark.parametrize("case", list(ur.PR_CASES))
def test_precision_recall_restatement_reproduces_the_reference_exactly(golden, case):
    g = golden("unconstrained_pr")
    real, gen = ur.pr_features(case)
    assert np.array_equal(real, g[f"{case}_real"]) and np.array_equal(gen, g[f"{case}_gen"])
    for k in ur.PR_KS:
        prec, r_real, f_gen = ur.manifold_estimate(real, gen, k)
        rec, r_gen, f_real = ur.manifold_estimate(gen, real, k)
        assert prec == float(g[f"{case}_k{k}_precision"]) and rec == float(g[f"{case}_k{k}_recall"])
        assert np.array_equal(r_real, g[f"{case}_k{k}_radii_real"]) and np.array_equal(r_gen, g[f"{case}_k{k}_radii_gen"])
        assert np.array_equal(f_gen, g[f"{case}_k{k}_flags_gen"]) and np.array_equal(f_real, g[f"{case}_k{k}_flags_real"])
        assert 0 < prec < 1 and 0 < rec <= 1
    n = min(len(real), len(gen))
    pr3 = (ur.manifold_estimate(real[:n], gen[:n], 3)[0], ur.manifold_estimate(gen[:n], real[:n], 3)[0])
    assert pr3 == tuple(g[f"{case}_precision_and_recall"])


@pytest.mark.parametrize("case", list(ur.PR_CASES))
def test_no_row_of_the_fixtures_is_undecided(golden, case):
    """The condition the GPU test's == rests on: at tau = (D + 2) 2^-23 every row of B is inside some ball by more than the disagreement two
    summation orders can have, or outside all of them by more than that. Checked on every run: a fixture that loses it fails HERE."""
    g = golden("unconstrained_pr")
    real, gen = g[f"{case}_real"], g[f"{case}_gen"]
    n = min(len(real), len(gen))
    for k in ur.PR_KS:
        for A, B, rk in ((real, gen, f"{case}_k{k}_radii_real"), (gen, real, f"{case}_k{k}_radii_gen")):
            assert len(ur.undecided_rows(B, A, g[rk])) == 0, (case, k, rk)
    for A, B in ((real[:n], gen[:n]), (gen[:n], real[:n])):               # what precision_and_recall compares
        assert len(ur.undecided_rows(B, A, ur.knn_radii(A, 3))) == 0


def test_duplicate_rows_have_radius_zero_and_count_as_hits(golden):
    g = golden("unconstrained_pr")
    for k in (1, 3):
        assert np.all(g[f"duplicates_k{k}_radii_real"][:4] == 0.0)
        assert g[f"duplicates_k{k}_flags_gen"][0]                         # gen[0] == real[0]: d = 0 <= r = 0
    assert np.all(g["duplicates_k8_radii_real"][:4] > 0)
    assert float(g["duplicates_k3_precision"]) == 0.425


# ---- the index draws ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ur.KID_CASES))
def test_index_draws_equal_the_reference(golden, case):
    from regennet_amd.eval.unconstrained import draw_subset_indices
    g = golden("unconstrained_kid")
    seed, Nr, Ng, D, subset = ur.KID_CASES[case]
    np.random.seed(ur.KID_SEED)
    idx_g, idx_r = draw_subset_indices(Nr, Ng, ur.KID_SUBSETS, subset)
    assert idx_g.dtype == idx_r.dtype == np.int32
    assert np.array_equal(idx_g, g[f"{case}_idx_g"]) and np.array_equal(idx_r, g[f"{case}_idx_r"])


def test_a_subset_larger_than_the_set_raises_numpys_error():
    from regennet_amd.eval.unconstrained import draw_subset_indices
    seed, Nr, Ng, D, subset = ur.KID_VALUE_ERROR
    np.random.seed(ur.KID_SEED)
    with pytest.raises(ValueError, match="larger sample than population"):
        draw_subset_indices(Nr, Ng, ur.KID_SUBSETS, subset)


# ---- the C-ABI without a device -------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    from regennet_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "regennet_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None


class _Args:
    """Good arguments for the three calls, over host memory that stands for device memory (never dereferenced: every call here fails a check
    first; `device` = -1 is refused last, so a call with good arguments answers 'device < 0')."""

    def __init__(self):
        self.buf = (C.c_char * 4096)()
        base = C.addressof(self.buf)
        self.p = (base + 15) & ~15                     # 16-byte aligned
        self.kw = dict(device=-1, x=self.p, Nx=130, y=self.p, Ny=97, D=256, idx_x=self.p, idx_y=self.p, S=5, m=70, degree=3, gamma=1 / 256, coef0=1.0,
                       mmds=self.p, vars=self.p, work=self.p, work_bytes=None, a=self.p, b=self.p, N=100, M=90, k=3, radii=self.p, flags=self.p,
                       count=self.p)


def _call(lib, fn, kw):
    if fn == "rgn_poly_mmd":
        wb = kw["work_bytes"]
        if wb is None:
            need = C.c_uint64()
            rc = lib.rgn_poly_mmd_workspace(kw["S"], kw["m"], C.byref(need))
            wb = need.value if rc == 0 else 1 << 40
        return lib.rgn_poly_mmd(kw["device"], kw["x"], kw["Nx"], kw["y"], kw["Ny"], kw["D"], kw["idx_x"], kw["idx_y"], kw["S"], kw["m"], kw["degree"],
                                kw["gamma"], kw["coef0"], kw["mmds"], kw["vars"], kw["work"], wb, None)
    if fn == "rgn_knn_radius":
        return lib.rgn_knn_radius(kw["device"], kw["a"], kw["N"], kw["D"], kw["k"], kw["radii"], None)
    return lib.rgn_manifold_hits(kw["device"], kw["b"], kw["M"], kw["a"], kw["radii"], kw["N"], kw["D"], kw["flags"], kw["count"], None)


BAD_ARGS = [
    ("rgn_poly_mmd", {}, "device < 0"), ("rgn_knn_radius", {}, "device < 0"), ("rgn_manifold_hits", {}, "device < 0"),
    ("rgn_poly_mmd", {"D": 254}, "no multiple of 4"), ("rgn_poly_mmd", {"D": 1028}, "no multiple of 4 in [4, 1024]"), ("rgn_poly_mmd", {"D": 0}, "D = 0"),
    ("rgn_knn_radius", {"D": 30}, "no multiple of 4"), ("rgn_knn_radius", {"D": 2048}, "[4, 1024]"),
    ("rgn_manifold_hits", {"D": 7}, "no multiple of 4"), ("rgn_manifold_hits", {"D": 1100}, "[4, 1024]"),
    ("rgn_knn_radius", {"k": 100, "N": 100}, "outside [1, 15]"), ("rgn_knn_radius", {"k": 16}, "outside [1, 15]"), ("rgn_knn_radius", {"k": 0}, "outside [1, 15]"),
    ("rgn_knn_radius", {"k": 8, "N": 8}, "is not below N = 8"), ("rgn_knn_radius", {"k": 3, "N": 3}, "is not below N = 3"),
    ("rgn_knn_radius", {"N": 0}, "N = 0"), ("rgn_manifold_hits", {"M": 0}, "M = 0"), ("rgn_manifold_hits", {"N": -4}, "N = -4"),
    ("rgn_poly_mmd", {"m": 2}, "m = 2 outside [3, 4096]"), ("rgn_poly_mmd", {"m": 4097}, "outside [3, 4096]"), ("rgn_poly_mmd", {"S": 0}, "S = 0"),
    ("rgn_poly_mmd", {"S": 65536}, "outside [1, 65535]"), ("rgn_poly_mmd", {"Nx": 1}, "Nx < 2"), ("rgn_poly_mmd", {"degree": 0}, "degree = 0"),
    ("rgn_poly_mmd", {"degree": 9}, "degree = 9"), ("rgn_poly_mmd", {"gamma": float("nan")}, "not finite"),
    ("rgn_poly_mmd", {"x": None}, "null"), ("rgn_poly_mmd", {"idx_y": None}, "null"), ("rgn_poly_mmd", {"vars": None}, "null"), ("rgn_poly_mmd", {"work": None}, "null"),
    ("rgn_knn_radius", {"a": None}, "null"), ("rgn_knn_radius", {"radii": None}, "null"),
    ("rgn_manifold_hits", {"b": None}, "null"), ("rgn_manifold_hits", {"radii": None}, "null"), ("rgn_manifold_hits", {"count": None}, "null"),
    ("rgn_poly_mmd", {"work_bytes": 1000}, "needed (rgn_poly_mmd_workspace)"), ("rgn_poly_mmd", {"work_bytes": 0}, "needed (rgn_poly_mmd_workspace)"),
    ("rgn_poly_mmd", {"work": "+8"}, "work is not 16-byte aligned"), ("rgn_poly_mmd", {"x": "+4"}, "x or y is not 16-byte aligned"),
    ("rgn_knn_radius", {"a": "+4"}, "not 16-byte aligned"), ("rgn_manifold_hits", {"b": "+8"}, "not 16-byte aligned"),
]


@pytest.mark.parametrize("fn,change,text", BAD_ARGS, ids=[f"{f}-{'-'.join(f'{k}={v}' for k, v in c.items()) or 'good'}" for f, c, _ in BAD_ARGS])
def test_bad_arguments_are_refused_before_the_device_is_touched(fn, change, text):
    from regennet_amd import _lib
    lib, a = _lib.load(), _Args()
    kw = dict(a.kw)
    for k, v in change.items():
        kw[k] = a.p + int(v) if isinstance(v, str) else v
    assert _call(lib, fn, kw) == -1                     # RGN_ERR_INVALID_ARG
    err = lib.rgn_last_error(None).decode()
    assert err.startswith(fn + ": ") and text in err, err


def test_workspace_query():
    from regennet_amd import _lib
    lib = _lib.load()
    need = C.c_uint64()
    assert lib.rgn_poly_mmd_workspace(100, 1000, C.byref(need)) == 0
    assert need.value == 100 * (8 + 16) * 1024 * 8      # per subset (8 + nt) rows of 64 nt doubles, nt = ceil(m / 64)
    assert lib.rgn_poly_mmd_workspace(1, 3, C.byref(need)) == 0 and need.value == 9 * 64 * 8
    assert lib.rgn_poly_mmd_workspace(1, 2, C.byref(need)) == -1 and "rgn_poly_mmd_workspace: m = 2" in lib.rgn_last_error(None).decode()
    assert lib.rgn_poly_mmd_workspace(1, 70, None) == -1 and "null nbytes" in lib.rgn_last_error(None).decode()


def test_cpu_tensors_are_refused():
    from regennet_amd.eval import unconstrained as un
    real, gen = (torch.from_numpy(x) for x in ur.make_features(0, 40, 40, 16))
    calls = [lambda: un.calculate_kid(real, gen), lambda: un.polynomial_mmd_averages(real, gen, n_subsets=2, subset_size=10),
             lambda: un.manifold_estimate(real, gen, 3), lambda: un.precision_and_recall(gen, real), lambda: un.calculate_diversity(gen),
             lambda: un.evaluate_unconstrained_metrics(gen, real), lambda: un.knn_radius(real, 3)]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert un.precision_and_recall(gen[:0], real) is None              # no data: None, like the reference


# ---- mutants --------------------------------------------------------------------------------------------------------------------------------------
def _fp32_entries(real, gen, idx_g, idx_r):
    """The kernel's arithmetic on the host: fp32 dot products, s and k in fp32, every sum in fp64."""
    gam, out = np.float32(ur.kernel_gamma(real.shape[1])), []
    for ig, ir in zip(idx_g, idx_r):
        X, Y = real[ig], gen[ir]
        Ks = []
        for a, b in ((X, X), (X, Y), (Y, Y)):
            s = (a @ b.T) * gam + np.float32(1)
            Ks.append((s * s * s).astype(np.float64))
        out.append(ur.mmd2_and_variance(Ks[0], Ks[1], Ks[2], min(len(real), len(gen))))
    return np.array(out).T


def test_mutants_fall_outside_the_bounds(golden, kid64):
    """Every variant below is a plausible wrong kernel. Each must miss a bound the GPU test asserts - mmds: the derived bound; vars: 8 x e_ref_var;
    radii: tau r; flags and counts: equality - and the kernel's own arithmetic on the host must meet all of them."""
    gk, gp = golden("unconstrained_kid"), golden("unconstrained_pr")
    lines = ["KID: worst |mmds - restatement| / derived bound and worst |vars - restatement| / (8 e_ref_var) over the case's 5 subsets",
             "%-14s %-34s %12s %12s" % ("case", "variant", "mmds / bound", "vars / tol")]
    for case in ur.KID_CASES:
        real, gen, idx_g, idx_r = kid_case(gk, case)
        mmds, vars_, bound = kid64[case]
        tol = VAR_MARGIN * float(gk[f"{case}_e_ref_var"])
        rows = {"fp32 entries (the kernel's arithmetic)": _fp32_entries(real, gen, idx_g, idx_r),
                "the reference (recorded)": (gk[f"{case}_mmds"], gk[f"{case}_vars"]),
                "operands rounded to bf16": ur.poly_mmd(real, gen, idx_g, idx_r, bf16=True)[:2],
                "K_XX's diagonal not removed": ur.poly_mmd(real, gen, idx_g, idx_r, keep_diag=True)[:2],
                "K_XY's marginals swapped": ur.poly_mmd(real, gen, idx_g, idx_r, swap_marginals=True)[:2]}
        for name, (m, v) in rows.items():
            rm, rv = (np.abs(m - mmds) / bound).max(), np.abs(v - vars_).max() / tol
            lines.append("%-14s %-34s %12.3e %12.3e" % (case, name, rm, rv))
            if name.startswith(("fp32", "the reference")):
                assert rm <= 1 and rv <= 1, (case, name, rm, rv)
            elif name.startswith("K_XY"):
                assert rm <= 1 and rv > 1, (case, name, rm, rv)           # mmd2 reads K_XY's total only: the variance must catch it
            else:
                assert rm > 1 and rv > 1, (case, name, rm, rv)
    lines += ["", "precision / recall: rows whose flag differs from the golden's (gen in real | real in gen) and the worst |r - r64| / (tau r64)",
              "%-14s %2s %-34s %10s %10s %12s" % ("case", "k", "variant", "flags gen", "flags real", "radii / tau")]
    caught = {}
    for case in ur.PR_CASES:
        real, gen = gp[f"{case}_real"], gp[f"{case}_gen"]
        t = ur.tau(real.shape[1])
        for k in ur.PR_KS:
            r64 = np.concatenate((gp[f"{case}_k{k}_radii_real"], gp[f"{case}_k{k}_radii_gen"]))
            for name, kw in (("Gram-form distances (fp32)", dict(gram=True)), ("order statistic k - 1", dict(k_offset=-1)),
                             ("order statistic k + 1", dict(k_offset=1)), ("< in place of <=", dict(strict=True))):
                _, r_real, f_gen = ur.manifold_estimate(real, gen, k, **kw)
                _, r_gen, f_real = ur.manifold_estimate(gen, real, k, **kw)
                d_gen, d_real = int((f_gen != gp[f"{case}_k{k}_flags_gen"]).sum()), int((f_real != gp[f"{case}_k{k}_flags_real"]).sum())
                r = np.concatenate((r_real, r_gen))
                with np.errstate(divide="ignore", invalid="ignore"):
                    rr = np.nan_to_num(np.where(r64 > 0, np.abs(r - r64) / (t * r64), np.where(r == 0, 0.0, np.inf)), nan=np.inf).max()
                lines.append("%-14s %2d %-34s %10d %10d %12.3e" % (case, k, name, d_gen, d_real, rr))
                caught.setdefault(name, []).append((case, k, d_gen + d_real > 0, rr > 1))
    for name, rows in caught.items():
        if name.startswith("order"):                       # a neighbouring order statistic moves every radius: caught in every case by the radii
            assert all(by_r for _, _, _, by_r in rows), (name, rows)
            assert any(by_f for _, _, by_f, _ in rows), (name, rows)
        elif name.startswith("Gram"):                      # the duplicate case: radii that must be exactly 0 are not, and flags change
            assert all(by_r and by_f for c, k, by_f, by_r in rows if c == "duplicates" and k in (1, 3)), (name, rows)
        else:                                              # '<' loses exactly the ties: d = 0 against r = 0 on the duplicate case
            assert all(by_f for c, k, by_f, _ in rows if c == "duplicates" and k in (1, 3)), (name, rows)
            assert not any(by_f for c, k, by_f, _ in rows if c != "duplicates"), (name, rows)
    print("\n" + "\n".join(lines))
    path = os.environ.get("REGENNET_UNCONSTRAINED_MUTANTS")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
