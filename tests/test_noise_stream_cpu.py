"""CPU: tests/philox_ref.py IS the stream include/regennet_hip.h documents - the Random123 known answers for Philox4x32-10, the layout
properties the header promises, two recorded draws at the ends of Box-Muller's domain - and the bounds of the GPU tests
(tests/test_noise_stream_gpu.py, tests/test_sampler_step_gpu.py) can tell a wrong implementation from a right one: each of three deliberately
wrong references moves away from the right one by far more than those bounds allow."""
import numpy as np
import torch

from tests import philox_ref as P
from tests import sampler_step_ref as R

F, T = 336, 60                      # the ntu models: 56 joints x 6 features, 60 frames

# Random123 kat_vectors, philox4x32 10 rounds: (counter, key, output)
KNOWN_ANSWERS = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

# Two draws at the ends of Box-Muller's domain, found once by sweeping the sample index at a fixed (seed, stream, feature, frame): about 2^23
# Philox calls per hit. `sample` is sample_offset + b. At U1_ONE the u1 word's top 24 bits are 0xFFFFFF (u1 = 1: both members of the pair are 0),
# at U1_MIN they are 0x000000 (u1 = 2^-24: the largest radius the stream can give, sqrt(48 ln 2) = 5.768).
EXTREME_SEED, EXTREME_STREAM, EXTREME_F, EXTREME_T = 0x5DEECE66D1234567, 3, 5, 6
U1_ONE_SAMPLE, U1_MIN_SAMPLE = 747079, 11731185
MAX_RADIUS = float(np.sqrt(48.0 * np.log(2.0)))
# what an MI355X returned for the (cos, sin) pair of the u1 = 2^-24 draw (rgn_randn_step, tests/test_noise_stream_gpu.py), as float32
DEVICE_U1_MIN_PAIR = (np.float32(5.484473), np.float32(-1.7865089))


def _u1_words(sample):
    ra, rb, member = P.words(EXTREME_SEED, sample, EXTREME_STREAM, EXTREME_F + 1, EXTREME_T + 2)
    return ra[EXTREME_F, EXTREME_T:EXTREME_T + 2], rb[EXTREME_F, EXTREME_T:EXTREME_T + 2], member[EXTREME_F, EXTREME_T:EXTREME_T + 2]


def test_philox4x32_10_known_answers():
    for ctr, key, want in KNOWN_ANSWERS:
        got = P.philox4x32_10(*ctr, *key)
        assert tuple(int(np.asarray(w).reshape(-1)[0]) for w in got) == want, [hex(int(np.asarray(w).reshape(-1)[0])) for w in got]
    # vectorised over the three at once: the same words
    c = [np.array([k[0][j] for k in KNOWN_ANSWERS], dtype=np.uint64) for j in range(4)]
    k = [np.array([k[1][j] for k in KNOWN_ANSWERS], dtype=np.uint64) for j in range(2)]
    got = P.philox4x32_10(*c, *k)
    for j in range(4):
        assert [int(v) for v in got[j]] == [ka[2][j] for ka in KNOWN_ANSWERS]


def test_a_swapped_multiplier_or_a_lost_round_misses_the_known_answers():
    ctr, key, want = KNOWN_ANSWERS[2]
    first = lambda r: tuple(int(np.asarray(w).reshape(-1)[0]) for w in r)
    assert first(P.philox4x32_10(*ctr, *key, m0=P.PHILOX_M1, m1=P.PHILOX_M0)) != want
    assert first(P.philox4x32_10(*ctr, *key, rounds=9)) != want
    assert first(P.philox4x32_10(*ctr, *key, rounds=10)) == want


def test_counter_layout_is_injective_and_xT_has_a_stream_of_its_own():
    """Distinct (sample, stream, element) -> distinct counters; stream 0xFFFFFFFF (x_T) is no loop index of a schedule (<= 1024 steps);
    sample 2^32 is not sample 0; the four elements of a counter are the frames 4j .. 4j + 3 of one feature."""
    seen = set()
    for sample in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63):
        for stream in (-1, 0, 1, 999, 1023):
            c0, c1, c2, c3, e = P.counters(sample, stream, F, T)
            assert len(np.unique(e)) == F * T and int(e.max()) < 2 ** 32
            slot = e & np.uint64(3)
            tup = set(zip(c0.ravel().tolist(), c1.ravel().tolist(), c2.ravel().tolist(), c3.ravel().tolist(), slot.ravel().tolist()))
            assert len(tup) == F * T, "an element's (counter, slot in the block) is its own"
            assert not (tup & seen), (sample, stream)
            seen |= tup
            assert int(c1[0, 0]) == (P.XT_STREAM if stream == -1 else stream)
    c = P.counters(0, 0, F, T)
    assert np.array_equal(c[0][:, 0::4], c[0][:, 3::4]) and not np.array_equal(c[0][:-1, 0], c[0][1:, 0])
    a, b = P.normals_f64(7, 0, 0, 4, 8), P.normals_f64(7, 2 ** 32, 0, 4, 8)
    assert not np.array_equal(a, b), "the high word of sample_offset + b is part of the counter"
    a, b = P.normals_f64(7, 0, 0, 4, 8), P.normals_f64(7 + 2 ** 32, 0, 0, 4, 8)
    assert not np.array_equal(a, b), "the high word of the seed is part of the key"
    xt = P.normals_f64(7, 0, -1, 4, 8)
    for i in (0, 1, 999, 1023):
        assert not np.array_equal(xt, P.normals_f64(7, 0, i, 4, 8))
    # a draw does not depend on the sequence length
    assert np.array_equal(P.normals_f64(7, 5, 3, 9, 57), P.normals_f64(7, 5, 3, 9, 60)[:, :57])


def test_uniforms_and_moments_of_the_reference():
    u1, u2, member = P.uniforms(1234, 0, 0, F, T)
    assert u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1
    assert np.array_equal(u1 * 2 ** 24, np.round(u1 * 2 ** 24)) and np.array_equal(member[0, :4], [0, 1, 0, 1])
    n = np.stack([P.normals_f64(1234, b, 0, F, T) for b in range(4)])
    assert abs(n.mean()) < 4 / n.size ** 0.5 and abs(n.var() - 1) < 0.02 and abs((n ** 4).mean() - 3) < 0.1
    n32 = np.stack([P.normals_f32(1234, b, 0, F, T) for b in range(4)])
    E = np.abs(n32 - n).max()
    assert 1e-7 < E < 4e-6, E           # float32 rounding of the formula: a few ulps of |n| <= 5.8


def test_recorded_extreme_draws():
    ra, rb, member = _u1_words(U1_ONE_SAMPLE)
    assert [int(v) >> 8 for v in ra] == [0xFFFFFF, 0xFFFFFF] and list(member) == [0, 1]
    n = P.normals_f64(EXTREME_SEED, U1_ONE_SAMPLE, EXTREME_STREAM, EXTREME_F + 1, EXTREME_T + 2)[EXTREME_F, EXTREME_T:EXTREME_T + 2]
    assert n[0] == 0.0 and n[1] == 0.0, n
    n32 = P.normals_f32(EXTREME_SEED, U1_ONE_SAMPLE, EXTREME_STREAM, EXTREME_F + 1, EXTREME_T + 2)[EXTREME_F, EXTREME_T:EXTREME_T + 2]
    assert n32[0] == 0.0 and n32[1] == 0.0, n32
    ra, rb, member = _u1_words(U1_MIN_SAMPLE)
    assert [int(v) >> 8 for v in ra] == [0, 0]
    n = P.normals_f64(EXTREME_SEED, U1_MIN_SAMPLE, EXTREME_STREAM, EXTREME_F + 1, EXTREME_T + 2)[EXTREME_F, EXTREME_T:EXTREME_T + 2]
    assert np.isfinite(n).all() and abs(np.hypot(n[0], n[1]) - MAX_RADIUS) < 1e-14 * MAX_RADIUS, n
    assert EXTREME_F < 336 and EXTREME_T + 1 < 60


def test_wrong_stream_variants_leave_the_tolerance():
    """The GPU test allows 4 E around normals_f64 (E: what float32 rounding costs the formula). A swapped multiplier and a flat element index
    both move the reference itself by ~1 at most elements: a device that implemented either would miss the bound everywhere."""
    seed, sample, stream = 0x1234ABCD00005678, 2 ** 32 - 1, 999
    ref = P.normals_f64(seed, sample, stream, F, 57)
    tol = 4 * np.abs(P.normals_f32(seed, sample, stream, F, 57) - ref).max()
    assert tol < 2e-5
    swapped = P.normals_f64(seed, sample, stream, F, 57, m0=P.PHILOX_M1, m1=P.PHILOX_M0)
    assert (np.abs(swapped - ref) > tol).mean() > 0.99
    flat = P.normals_f64(seed, sample, stream, F, 57, elem=P.flat_elem)
    assert np.array_equal(flat[0], ref[0]), "feature 0: both rules give element t"
    assert (np.abs(flat[1:] - ref[1:]) > tol).mean() > 0.99
    # ... and away from what the device returned at the recorded u1 = 2^-24 draw (feature 5: the flat rule gives another element)
    at = lambda n: n[EXTREME_F, EXTREME_T:EXTREME_T + 2]
    args = (EXTREME_SEED, U1_MIN_SAMPLE, EXTREME_STREAM, EXTREME_F + 1, 60)
    ref = P.normals_f64(*args)
    tol = 4 * np.abs(P.normals_f32(*args) - ref).max()
    dev = np.array(DEVICE_U1_MIN_PAIR, dtype=np.float64)
    assert np.abs(at(ref) - dev).max() <= tol
    assert np.abs(at(P.normals_f64(*args, m0=P.PHILOX_M1, m1=P.PHILOX_M0)) - dev).min() > 1000 * tol
    assert np.abs(at(P.normals_f64(*args, elem=P.flat_elem)) - dev).min() > 1000 * tol
    assert np.abs(at(P.normals_f64(*args, rounds=9)) - dev).min() > 1000 * tol
    dropped_high = P.normals_f64(seed, sample + 1 - 2 ** 32, stream, F, 57)       # (sample_offset + b) mod 2^32
    assert (np.abs(dropped_high - P.normals_f64(seed, sample + 1, stream, F, 57)) > tol).mean() > 0.99


def test_a_neighbouring_alphas_cumprod_prev_leaves_the_step_bound():
    """The step bound is 2^-22 A. With alphas_cumprod_prev taken one entry off, either way, the DDIM reference leaves it at every loop index but
    those where the line does not read the entry's value (index 0 of the later neighbour: abp = 1 either way)."""
    g = torch.Generator().manual_seed(0)
    x, x0, eps = (torch.randn(3, 56, 6, 57, generator=g) * s for s in (1.0, 0.5, 1.0))
    for name in R.SCHEDULES:
        _, tb = R.schedule(name)
        S = len(tb["betas"])
        for i in R.loop_indices(S):
            for eta in (0.0, 0.5, 1.0):
                ref, _ = R.step_ref(tb, i, x, x0, eps, "ddim", eta, False)
                A = R.terms(tb, i, x, x0, eps, "ddim", eta)
                for bad_tb in (R.prev_read_at_i(tb), R.prev_one_step_early(tb)):
                    if bad_tb["alphas_cumprod_prev"][i] == tb["alphas_cumprod_prev"][i]:
                        continue
                    bad, _ = R.step_ref(bad_tb, i, x, x0, eps, "ddim", eta, False)
                    ratio = (bad - ref).abs().double().numpy() / A
                    assert np.median(ratio) > 20 * R.BOUND, (name, i, eta, float(np.median(ratio)) / R.BOUND)


def test_step_reference_clamps_first_and_stays_under_its_own_terms():
    """pred_xstart is the clamped prediction, and |x'| <= A: A sums the absolute values of exactly the terms the reference adds."""
    for name in R.SCHEDULES:
        _, tb = R.schedule(name)
        S = len(tb["betas"])
        g = torch.Generator().manual_seed(1)
        x, x0, eps = (torch.randn(2, 5, 6, 8, generator=g) for _ in range(3))
        for i in R.loop_indices(S):
            for mode, eta in R.SAMPLERS.values():
                for clip in (False, True):
                    a, p = R.step_ref(tb, i, x, x0 * 1.5, eps, mode, eta, clip)
                    assert torch.equal(p, (x0 * 1.5).clamp(-1, 1) if clip else x0 * 1.5)
                    A = R.terms(tb, i, x, p, eps, mode, eta)
                    assert torch.isfinite(a).all() and (a.abs().double().numpy() <= A * (1 + 1e-5) + 1e-30).all(), (name, i, mode, eta, clip)


def test_the_step_reference_takes_correctly_rounded_square_roots():
    """ddim_sample's sqrt(1 - abp - sigma^2) cancels, so the reference is only as reproducible as its sqrt: the oracle's is the correctly rounded
    float32 one on every host (torch's CPU sqrt is a last place off on a fifth of these arguments on some)."""
    from oracle import regennet_oracle as orc
    a = np.random.default_rng(0).uniform(1e-6, 1.0, 200000).astype(np.float32)
    want = np.sqrt(a.astype(np.float64)).astype(np.float32)          # float32 -> float64 sqrt -> float32 rounds correctly (no double-rounding case for sqrt)
    assert np.array_equal(orc._sqrt(torch.from_numpy(a)).numpy(), want)
    assert np.array_equal(orc._sqrt(torch.from_numpy(a[:3]).view(3, 1, 1, 1).expand(3, 2, 2, 5)).numpy(), np.broadcast_to(want[:3].reshape(3, 1, 1, 1), (3, 2, 2, 5)))
    assert torch.isnan(orc._sqrt(torch.tensor([-1.0]))).all()
