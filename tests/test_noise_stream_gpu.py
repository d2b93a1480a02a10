"""GPU: rgn_randn / rgn_randn_step against the host statement of the stream (tests/philox_ref.py), element for element.

The existing checks of the stream are moments, sharding and determinism: a wrong constant, a lost round, another counter layout or a dropped
high word passes all of them. Here every element of a draw is compared with normals_f64 - Philox4x32-10 of the documented counter, Box-Muller in
float64 - so the words must be the documented ones (a different word gives an unrelated normal) and the hardware log2 / sqrt / sin / cos must
carry them to the normal within

    4 E,   E = max |normals_f32 - normals_f64| over the very elements compared

E is a host-only number: what rounding alone costs a float32 evaluation of the formula (numpy's transcendentals, ~0.5 ulp); the factor covers
hardware transcendentals documented at ~1 ulp. The device's own maximum is printed, never used."""
import functools

import numpy as np
import pytest
import torch

from regennet_amd import synth
from tests import philox_ref as P
from tests.helpers import build_hip
from tests.test_noise_stream_cpu import EXTREME_F, EXTREME_SEED, EXTREME_STREAM, EXTREME_T, MAX_RADIUS, U1_MIN_SAMPLE, U1_ONE_SAMPLE

pytestmark = pytest.mark.gpu

B, J, NF = 3, 56, 6
F = J * NF
SEED_HI = 0x9E3779B97F4A7C15          # a seed whose high word is not zero
_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for model in _MODELS.values():
        model._engine.close()
    _MODELS.clear()


def _engine(T):
    if T not in _MODELS:
        cfg = synth.get_config("ntu", layers=1, num_frames=T)
        _MODELS[T], _ = build_hip(cfg, synth.make_state_dict(cfg, seed=0), resp="ddim5")
    return _MODELS[T]._get_engine(B, T)[0]


def _device_draw(T, seed, sample_offset, loop_index, x_T_entry=False):
    eng = _engine(T)
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((B, J, NF, T), float("nan"), device="cuda")
    if x_T_entry:
        eng.randn(out, B, seed, sample_offset, st)
    else:
        eng.randn_step(out, B, seed, sample_offset, loop_index, st)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(B, F, T)


@functools.lru_cache(maxsize=None)
def _host_draw(T, seed, sample_offset, loop_index):
    """(normals_f64, E) for the B motions of a draw."""
    ref = P.batch_normals_f64(seed, sample_offset, loop_index, B, F, T)
    return ref, float(np.abs(P.batch_normals_f32(seed, sample_offset, loop_index, B, F, T) - ref).max())


CASES = [(T, seed, off, i) for T in (60, 57) for seed, off in ((1234, 0), (1234, 2 ** 32 - 2), (SEED_HI, 0), (SEED_HI, 2 ** 32 - 2))
         for i in (-1, 0, 1, 999)]


@pytest.mark.parametrize("T,seed,sample_offset,loop_index", CASES)
def test_every_element_of_a_draw_is_the_documented_stream(T, seed, sample_offset, loop_index):
    """T = 57 is no multiple of 4: the layout alone decides which frames share a Philox block. sample_offset = 2^32 - 2 with B = 3: motion 2 is
    sample 2^32, the carry into the counter's fourth word. Loop index -1 is x_T's stream word 0xFFFFFFFF."""
    got = _device_draw(T, seed, sample_offset, loop_index)
    ref, E = _host_draw(T, seed, sample_offset, loop_index)
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    print(f"\n[noise stream] T={T} seed={seed:#x} sample_offset={sample_offset} loop_index={loop_index}: E={E:.3e} allowed 4E={4 * E:.3e} "
          f"device max={err.max():.3e} ({err.max() / E:.2f} E) max|n|={np.abs(ref).max():.3f}")
    assert 5e-7 < E < 4e-6, "float32 rounding of a |n| <= 5.8 formula"
    worst = np.unravel_index(err.argmax(), err.shape)
    assert err.max() <= 4 * E, (worst, float(got[worst]), float(ref[worst]))
    if loop_index == -1:
        assert np.array_equal(_device_draw(T, seed, sample_offset, -1, x_T_entry=True), got), "rgn_randn is loop index -1"


def test_streams_of_the_cases_are_pairwise_different_on_the_device():
    """(the comparison above could not pass otherwise; this keeps the failure readable if a word is dropped)"""
    a = _device_draw(60, SEED_HI, 2 ** 32 - 2, 0)
    assert not np.array_equal(a[2], _device_draw(60, SEED_HI, 0, 0)[0]), "sample 2^32 is not sample 0"
    assert not np.array_equal(a, _device_draw(60, SEED_HI & 0xFFFFFFFF, 2 ** 32 - 2, 0)), "the seed's high word counts"
    assert not np.array_equal(a, _device_draw(60, SEED_HI, 2 ** 32 - 2, -1)), "x_T is not loop index 0"


@pytest.mark.parametrize("T", (60, 57))
def test_the_two_ends_of_box_muller(T):
    """u1 = 1 (log2 = 0: both members 0) and u1 = 2^-24 (the largest radius, sqrt(48 ln 2)): the recorded tuples of tests/test_noise_stream_cpu.py,
    as motion 1 of a batch. The device value is finite and within the tolerance of the draw it belongs to."""
    for name, sample in (("u1 = 1", U1_ONE_SAMPLE), ("u1 = 2^-24", U1_MIN_SAMPLE)):
        got = _device_draw(T, EXTREME_SEED, sample - 1, EXTREME_STREAM)
        ref, E = _host_draw(T, EXTREME_SEED, sample - 1, EXTREME_STREAM)
        pair, want = got[1, EXTREME_F, EXTREME_T:EXTREME_T + 2], ref[1, EXTREME_F, EXTREME_T:EXTREME_T + 2]
        print(f"\n[noise stream] T={T} {name}: device pair = ({pair[0]!r}, {pair[1]!r}) reference = ({want[0]!r}, {want[1]!r}) "
              f"radius {np.hypot(*pair.astype(np.float64)):.7f} (sqrt(48 ln 2) = {MAX_RADIUS:.7f}) E={E:.3e}")
        assert np.isfinite(got).all()
        assert np.abs(pair - want).max() <= 4 * E
        assert np.abs(got - ref).max() <= 4 * E
        if sample == U1_ONE_SAMPLE:
            assert want[0] == 0.0 and want[1] == 0.0
        else:
            assert abs(np.hypot(*want) - MAX_RADIUS) < 1e-12
