"""CPU: the in-painting surface that needs no GPU - the C-ABI declaration and binding of rgn_set_inpainting, the edit CLI's mask builders
and arguments, and the recorded fixtures' own consistency (tests/golden/inpaint_*.npz against tests/inpaint_cases.py)."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

from tests.helpers import digest
from tests.inpaint_cases import CASES, case_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_header_declares_and_binding_lists_rgn_set_inpainting():
    from regennet_amd import _lib
    header = open(os.path.join(ROOT, "include", "regennet_hip.h")).read()
    assert re.search(r"RGN_API int rgn_set_inpainting\(rgn_handle h, int32_t B, const uint8_t\* mask_dev, const float\* motion_dev, void\* stream\);", header)
    assert "rgn_set_inpainting" in _lib.SYMBOLS
    res, args = _lib.SYMBOLS["rgn_set_inpainting"]
    assert res is C.c_int and len(args) == 5


def test_null_handle_returns_invalid_arg():
    from regennet_amd import _lib
    lib = _lib.load()
    assert lib.rgn_set_inpainting(None, 1, None, None, None) == -1


def test_in_between_mask_literal():
    from regennet_amd.sample.edit import in_between_mask
    m = in_between_mask((2, 3, 2, 8), 0.25, 0.75)
    assert m.dtype == bool and m.shape == (2, 3, 2, 8)
    assert m[1, 2, 1].tolist() == [True, True, False, False, False, False, True, True]
    assert (m == m[0, 0, 0]).all()
    # int() truncation: T = 60 -> [15, 45), T = 150 -> [37, 112)  (150 * 0.25 = 37.5, 150 * 0.75 = 112.5)
    m60 = in_between_mask((1, 1, 1, 60), 0.25, 0.75)[0, 0, 0]
    assert np.flatnonzero(~m60).tolist() == list(range(15, 45))
    m150 = in_between_mask((1, 1, 1, 150), 0.25, 0.75)[0, 0, 0]
    assert np.flatnonzero(~m150).tolist() == list(range(37, 112))
    # prefix only
    p = in_between_mask((1, 1, 1, 150), 0.25, 1.0)[0, 0, 0]
    assert p[:37].all() and not p[37:].any()
    # T = 60, 0.1 .. 0.5 -> [6, 30)
    q = in_between_mask((1, 1, 1, 60), 0.1, 0.5)[0, 0, 0]
    assert np.flatnonzero(~q).tolist() == list(range(6, 30))


def test_rows_mask_and_row_spec():
    from regennet_amd.sample.edit import parse_rows, rows_mask
    assert parse_rows("0-21,55") == list(range(22)) + [55]
    assert parse_rows("3") == [3] and parse_rows("2, 0-1") == [0, 1, 2]
    m = rows_mask((2, 56, 6, 4), parse_rows("0-21,55"))
    assert m.dtype == bool and m[:, :22].all() and m[:, 55].all() and not m[:, 22:55].any()
    with pytest.raises(ValueError):
        rows_mask((1, 56, 6, 4), [56])
    with pytest.raises(ValueError):
        parse_rows("")


def test_edit_args_defaults_and_upper_body():
    from regennet_amd.sample.edit import build_mask
    from regennet_amd.utils.parser_util import edit_args
    a = edit_args([])
    assert a.edit_mode == "in_between" and a.prefix_end == 0.25 and a.suffix_start == 0.75 and a.keep_rows == "" and a.input_motions == ""
    assert a.guidance_param == 2.5 and a.num_samples == 10          # cgenerate's groups are all there
    a = edit_args(["--edit_mode", "rows", "--keep_rows", "0-21,55"])
    assert build_mask(a, (1, 56, 6, 60))[0, :, 0, 0].sum() == 23
    with pytest.raises(NotImplementedError, match="HumanML3D"):
        build_mask(edit_args(["--edit_mode", "upper_body"]), (1, 56, 6, 60))


def test_every_case_has_a_fixture_and_none_is_stray():
    have = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "inpaint_*.npz")))
    assert have == sorted(CASES)
    for name in have:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= 400 * 1024, name


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_matches_its_case(name):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    case, cfg, mask, target = case_inputs(name)
    assert digest(mask, target) == str(g["inpaint_digest"]), "mask / target rule drifted from the recorded fixture"
    assert int(g["B"]) == case["B"] and str(g["resp"]) == case["resp"] and str(g["mode"]) == case["mode"] and bool(g["guided"]) == case["guided"]
    if "rows" in case:
        final, mask, target = g["final_rows"], mask[g["rows"]], target[g["rows"]]
    else:
        final = g["final"]
    want = np.clip(target, -1, 1) if bool(g["clip"]) else target      # (the clamp follows the blend, gaussian_diffusion.py:323 / 330)
    assert mask.any() and np.array_equal(final[mask], want[mask]), "masked elements of the reference's result are the target, bit for bit"
    if not mask.all():
        assert not np.array_equal(final[~mask], target[~mask])
    if "x0" in g:   # the traced fixture: every step's pred_xstart carries the target too
        for k in range(g["x0"].shape[0]):
            assert np.array_equal(g["x0"][k][mask], want[mask]), k
