"""fp64 numpy statement of the unconstrained evaluation's two metrics (the reference's eval/unconstrained/metrics/kid.py:8-126 and
precision_recall.py:30-53), the host error model for KID, the fixture recipe and the MUTANTS - host-model variants of either metric that a test
bound must be able to tell from the real thing (tests/test_unconstrained_cpu.py shows that it does). Test infrastructure; nothing here runs on a GPU.

Error model of one kernel-matrix entry k = (gamma dot + coef0)^degree computed from fp32 inputs with exact fp32 products, fp32 accumulation over D
in any order, and degree - 1 fp32 multiplications; u = 2^-24, s = gamma dot + coef0:

    |ds| <= gamma (D + 2) u sum_c |x_c y_c| + 2 u |s|                 (the D - 1 additions and the gamma product; then the coef0 addition)
    |dk| <= degree |s|^(degree - 1) |ds| + (degree - 1) u |s|^degree   (first order in ds; one rounding per multiplication)

mmd2 ('unbiased') is a FIXED linear functional sum_ij w_ij K_ij of the three matrices' entries - w = 1 / (m (m - 1)) off the diagonals of K_XX and
K_YY, 0 on them, -2 / m^2 on K_XY - so the fp32 rounding of the entries moves it by at most sum |w_ij| |dk_ij|; the fp64 sums add a few 2^-53
of sum |w_ij| |k_ij| (4 m 2^-53 is taken: the longest chain of additions is below 4 m long in any order of summation). Derived, not tuned.
var_est is a cancelling polynomial in the sums and has no cheap a-priori bound (the tests hold it to the reference's own fp32 deviation)."""
import numpy as np

U = 2.0 ** -24


def make_features(seed, Nr, Ng, D):
    """The fixture recipe: a six-dimensional manifold in D dimensions, shifted and widened for the generated set. -> (real, gen) fp32."""
    g = np.random.default_rng(seed)
    W = g.standard_normal((6, D)) / np.sqrt(6)
    real = g.standard_normal((Nr, 6)) @ W + 0.05 * g.standard_normal((Nr, D))
    gen = (1.3 * g.standard_normal((Ng, 6)) + 0.6) @ W + 0.05 * g.standard_normal((Ng, D))
    return real.astype(np.float32), gen.astype(np.float32)


# (seed, Nr, Ng, D, duplicates) of the precision / recall cases, each with k = 1, 3, 8
PR_CASES = {"n97x80": (0, 97, 80, 256, False), "n130": (2, 130, 130, 256, False), "d20": (3, 70, 97, 20, False), "tile_plus_one": (4, 33, 33, 256, False),
            "duplicates": (6, 40, 40, 256, True)}
PR_KS = (1, 3, 8)
# (seed, Nr, Ng, D, subset) of the KID cases: np.random.seed(KID_SEED), KID_SUBSETS subsets; `real` is codes_g (kid.py:133-136)
KID_CASES = {"replace": (5, 130, 97, 256, 70), "permutation": (5, 70, 97, 256, 70), "subset50": (5, 70, 97, 256, 50), "d20": (5, 130, 97, 20, 70)}
KID_SEED, KID_SUBSETS = 7, 5
KID_VALUE_ERROR = (5, 70, 97, 256, 80)             # a subset of 80 from a set of 70 without replacement: numpy's ValueError


def pr_features(case):
    seed, Nr, Ng, D, dup = PR_CASES[case]
    real, gen = make_features(seed, Nr, Ng, D)
    if dup:
        real[1:4] = real[0]
        gen[0] = real[0]
    return real, gen


def to_bf16(x):
    """fp32 -> the nearest bf16 (ties to even), as fp32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


# ---- KID ------------------------------------------------------------------------------------------------------------------------------------------
def kernel_gamma(D, gamma=None):
    """sklearn's `K *= gamma` on an fp32 matrix: the fp32 rounding of gamma (default 1 / D)."""
    return float(np.float32(1.0 / D if gamma is None else gamma))


def mmd2_and_variance(K_XX, K_XY, K_YY, var_at_m, keep_diag=False, swap_marginals=False):
    """_mmd2_and_variance (kid.py:43-126), mmd_est='unbiased', in the dtype of its inputs. Mutants: keep_diag - K_XX's diagonal is not removed;
    swap_marginals - K_XY's two marginals change places."""
    m = K_XX.shape[0]
    diag_X, diag_Y = np.diagonal(K_XX), np.diagonal(K_YY)
    if keep_diag:
        diag_X = np.zeros_like(diag_X)
    sum_diag2_X, sum_diag2_Y = diag_X.dot(diag_X), diag_Y.dot(diag_Y)
    Kt_XX_sums = K_XX.sum(axis=1) - diag_X
    Kt_YY_sums = K_YY.sum(axis=1) - diag_Y
    K_XY_sums_0, K_XY_sums_1 = K_XY.sum(axis=0), K_XY.sum(axis=1)
    if swap_marginals:
        K_XY_sums_0, K_XY_sums_1 = K_XY_sums_1, K_XY_sums_0
    Kt_XX_sum, Kt_YY_sum, K_XY_sum = Kt_XX_sums.sum(), Kt_YY_sums.sum(), K_XY_sums_0.sum()
    mmd2 = (Kt_XX_sum + Kt_YY_sum) / (m * (m - 1)) - 2 * K_XY_sum / (m * m)
    sqn = lambda a: np.ravel(a).dot(np.ravel(a))        # noqa: E731
    Kt_XX_2_sum, Kt_YY_2_sum, K_XY_2_sum = sqn(K_XX) - sum_diag2_X, sqn(K_YY) - sum_diag2_Y, sqn(K_XY)
    dot_XX_XY, dot_YY_YX = Kt_XX_sums.dot(K_XY_sums_1), Kt_YY_sums.dot(K_XY_sums_0)
    m1, m2 = m - 1, m - 2
    zeta1_est = (1 / (m * m1 * m2) * (sqn(Kt_XX_sums) - Kt_XX_2_sum + sqn(Kt_YY_sums) - Kt_YY_2_sum)
                 - 1 / (m * m1) ** 2 * (Kt_XX_sum ** 2 + Kt_YY_sum ** 2)
                 + 1 / (m * m * m1) * (sqn(K_XY_sums_1) + sqn(K_XY_sums_0) - 2 * K_XY_2_sum)
                 - 2 / m ** 4 * K_XY_sum ** 2
                 - 2 / (m * m * m1) * (dot_XX_XY + dot_YY_YX)
                 + 2 / (m ** 3 * m1) * (Kt_XX_sum + Kt_YY_sum) * K_XY_sum)
    zeta2_est = (1 / (m * m1) * (Kt_XX_2_sum + Kt_YY_2_sum)
                 - 1 / (m * m1) ** 2 * (Kt_XX_sum ** 2 + Kt_YY_sum ** 2)
                 + 2 / (m * m) * K_XY_2_sum
                 - 2 / m ** 4 * K_XY_sum ** 2
                 - 4 / (m * m * m1) * (dot_XX_XY + dot_YY_YX)
                 + 4 / (m ** 3 * m1) * (Kt_XX_sum + Kt_YY_sum) * K_XY_sum)
    var_est = 4 * (var_at_m - 2) / (var_at_m * (var_at_m - 1)) * zeta1_est + 2 / (var_at_m * (var_at_m - 1)) * zeta2_est
    return mmd2, var_est


def poly_mmd(codes_g, codes_r, idx_g, idx_r, degree=3, gamma=None, coef0=1.0, bf16=False, keep_diag=False, swap_marginals=False):
    """polynomial_mmd (kid.py:29-41) of every row of idx_g / idx_r [S, m], in fp64 from the fp32 features.
    -> (mmds [S], vars [S], bound [S]): `bound` is the error model's bound on |mmds_fp32-kernel-entries - mmds|. Mutant bf16: operands rounded to bf16."""
    D = codes_g.shape[1]
    gam, var_at_m = kernel_gamma(D, gamma), min(len(codes_g), len(codes_r))
    if bf16:
        codes_g, codes_r = to_bf16(codes_g), to_bf16(codes_r)
    G, R = np.asarray(codes_g, np.float64), np.asarray(codes_r, np.float64)
    S, m = idx_g.shape
    mmds, vars_, bound = np.zeros(S), np.zeros(S), np.zeros(S)
    off = 1.0 - np.eye(m)
    for i in range(S):
        X, Y = G[idx_g[i]], R[idx_r[i]]
        Ks, dKs = [], []
        for a, b in ((X, X), (X, Y), (Y, Y)):
            s = gam * (a @ b.T) + coef0
            ds = gam * (D + 2) * U * (np.abs(a) @ np.abs(b).T) + 2 * U * np.abs(s)
            Ks.append(s ** degree)
            dKs.append(degree * np.abs(s) ** (degree - 1) * ds + (degree - 1) * U * np.abs(s) ** degree)
        mmds[i], vars_[i] = mmd2_and_variance(Ks[0], Ks[1], Ks[2], var_at_m, keep_diag=keep_diag, swap_marginals=swap_marginals)
        w_in, w_x = 1.0 / (m * (m - 1)), 2.0 / (m * m)
        bound[i] = w_in * ((dKs[0] + dKs[2]) * off).sum() + w_x * dKs[1].sum()
        bound[i] += 4 * m * 2.0 ** -53 * (w_in * ((np.abs(Ks[0]) + np.abs(Ks[2])) * off).sum() + w_x * np.abs(Ks[1]).sum())
    return mmds, vars_, bound


# ---- precision / recall ---------------------------------------------------------------------------------------------------------------------------
def distances(B, A, gram=False):
    """d(B_i, A_j) [M, N] in fp64 from the fp32 rows, direct-difference form. Mutant gram: |a|^2 + |b|^2 - 2 a.b in fp32 as a kernel would form it -
    the squared norms summed in descending index order (a pre-pass of its own), the products by the matrix product's own order, no clamp: between identical rows the three terms no
    longer cancel exactly, and d comes out small and positive, or NaN where the difference is negative."""
    if gram:
        B32, A32 = np.asarray(B, np.float32), np.asarray(A, np.float32)
        nb, na = np.cumsum((B32 * B32)[:, ::-1], axis=1, dtype=np.float32)[:, -1], np.cumsum((A32 * A32)[:, ::-1], axis=1, dtype=np.float32)[:, -1]
        with np.errstate(invalid="ignore"):
            return np.sqrt((nb[:, None] + na[None, :]) - np.float32(2) * (B32 @ A32.T)).astype(np.float64)
    B64, A64 = np.asarray(B, np.float64), np.asarray(A, np.float64)
    return np.sqrt(((B64[:, None, :] - A64[None, :, :]) ** 2).sum(-1))


def knn_radii(A, k, gram=False):
    """precision_recall.py:34-42: r_i = np.partition(d(A_i, .), k)[k], j = i included."""
    return np.partition(distances(A, A, gram=gram), k, axis=1)[:, k]


def manifold_flags(B, A, radii, gram=False, strict=False):
    """precision_recall.py:44-53: flag_i = any_j (d(B_i, A_j) <= r_j). Mutant strict: < in place of <=."""
    d = distances(B, A, gram=gram)
    return ((d < radii[None, :]) if strict else (d <= radii[None, :])).any(axis=1)


def manifold_estimate(A, B, k, gram=False, strict=False, k_offset=0):
    """-> (n / len(B), radii [N], flags [M]). Mutant k_offset: the order statistic off by that much."""
    radii = knn_radii(A, k + k_offset, gram=gram)
    flags = manifold_flags(B, A, radii, gram=gram, strict=strict)
    return int(flags.sum()) / len(B), radii, flags


def tau(D):
    """First-order bound on the relative disagreement of two fp32 direct-difference distances summed in different orders: (D + 1) 2^-24 on each
    side, plus the square roots."""
    return (D + 2) * 2.0 ** -23


def undecided_rows(B, A, radii):
    """Rows of B whose membership could depend on the summation order: no A_j with d <= r_j (1 - tau), yet some with d <= r_j (1 + tau). The one
    exact tie - d = 0 against r = 0 between identical rows - counts as decided (both sides are exact in every order)."""
    t = tau(A.shape[1])
    d = distances(B, A)
    r = radii[None, :]
    sure_in = ((d <= r * (1 - t)) | ((d == 0) & (r == 0))).any(axis=1)
    maybe = (d <= r * (1 + t)).any(axis=1)
    return np.flatnonzero(maybe & ~sure_in)
