"""The host statement of the recogniser's fused kernels (tests/sg_stage_ref.py), pinned without a GPU: composed over a block plan it IS the
reference's forward (tests/small_graph_ref.py) to 1e-9 of the largest feature; the driver's slot tables follow the contract of rgn_internal.h; and the
bounds tests/test_sg_stage_gpu.py holds the kernels to - computed here from the host model alone, never typed in - tell every mutant of the statement
from the statement itself.

The detection table (profiles/sg_stage_mutants.txt) is what test_mutants_are_detected prints; the fold's own rounding (profiles/sg_stage_parity.txt)
is what test_stages_compose_to_the_reference prints."""
import os

import numpy as np
import pytest

from regennet_amd import synth
from tests import sg_stage_cases as C
from tests import sg_stage_ref as R
from tests import small_graph_ref as sgr

HERE = os.path.dirname(os.path.abspath(__file__))


def _plans():
    A56 = np.load(os.path.join(HERE, "golden", "stgcn.npz"))["A"]
    A15 = sgr.tree_graph(15, 3, np.random.Generator(np.random.PCG64(3000 + 37 * 15 + 3)))
    return {"ten_golden": (A56, sgr.TEN, 2, 12, 20), "six_v15": (A15, sgr.SIX, 1, 3, 21)}


@pytest.mark.parametrize("plan", ["ten_golden", "six_v15"])
def test_stages_compose_to_the_reference(plan):
    """gcn, tconv and tconv_s2 composed through the planes of rgn_stgcn_forward - pad frames, polyphase regions, the padded vertices of the 15-vertex
    graph - against small_graph_ref.forward: both are fp64 evaluations of one real function over sums of <= 2 432 terms, so 1e-9 of the largest
    feature is three orders above what separates them. With the folded tensors cast to fp32, as finalize stores them, the distance is the fold's
    own rounding: printed, the yardstick for the engine's 6e-6."""
    A, blocks, persons, cin, T = _plans()[plan]
    sd = synth.make_stgcn_state_dict(A, num_class=13, in_channels=cin, num_person=persons, seed=0, blocks=None if blocks is sgr.TEN else blocks)
    x = np.random.Generator(np.random.PCG64(11)).standard_normal((2, A.shape[1], cin, T)).astype(np.float32)
    rf, ry = (t.numpy() for t in sgr.forward(sd, x, blocks, persons))
    f, y = R.forward_stages(sd, x, blocks, persons)
    scale = np.abs(rf).max()
    err, erry = np.abs(f - rf).max() / scale, np.abs(y - ry).max() / np.abs(ry).max()
    f32f, _ = R.forward_stages(sd, x, blocks, persons, cast=np.float32)
    print(f"{plan}: largest feature {scale:.3f}; fp64 fold: features {err:.2e}, logits {erry:.2e} of the largest; fp32 fold: features {np.abs(f32f - rf).max() / scale:.2e}")
    assert err < 1e-9 and erry < 1e-9


def test_slot_tables_follow_the_contract():
    """sl_v / sl_a / slot_k as rgn_internal.h states them: slot s serves partition (slot_k >> 4 s) & 15, 15 = unused; a partition owns as many slots as its
    longest list; a shorter list is padded with (w, 0). The golden graph's longest lists are 1 / 6 / 1, the tree's 1 / 1 / 6 - all eight slots."""
    for name, longest in (("gcn_v56_64x64_split", [1, 6, 1]), ("gcn_v56_64x64_tree_split", [1, 1, 6]), ("gcn_v15_64x64_tree_split", [1, 1, 6])):
        st = C.stage(name)
        assert st.cnt == longest
        slot_k, sv, sa = st.slot_tables()
        parts = [(slot_k >> (4 * s)) & 15 for s in range(8)]
        assert parts == sum(([k] * n for k, n in enumerate(longest)), [])
        A = np.zeros_like(st.A)
        for w in range(st.V):
            for s in range(8):
                if sa[w, s] == 0:
                    assert sv[w, s] == w
                A[parts[s], sv[w, s], w] += sa[w, s]
        assert np.array_equal(A, st.A)
        real = C.BY_NAME[name]["V"]
        assert not st.A[:, real:, :].any() and not st.A[:, :, real:].any() and not st.b1[[r for r in range(st.b1.shape[0]) if r % st.V >= real]].any()


def test_walk_cases_have_more_than_512_tiles():
    walks = [c for c in C.CASES if C.is_walk(c)]
    assert {c["kernel"] for c in walks} == {"gcn", "tconv", "tconv_pre", "tconv_s2"}      # one per persistent kernel (launch_gemm_x3_sg runs a workgroup per tile)
    for c in walks:
        g = R.Geo(c["NM"], c["T"], R.padded_nodes(c["V"]), poly=c["kernel"] == "tconv_s2")
        rows = g.region if g.poly else g.rows
        assert -(-rows // c.get("BM", 256)) > 512, c["name"]


_SMALL = [c["name"] for c in C.CASES if not C.is_walk(c)]


@pytest.mark.parametrize("name", _SMALL)
def test_bounds_come_from_the_family(name):
    """Every bound is twice the worst fp32 member's statistic, every member lies inside it, and the family has a width."""
    fam, bd = C.family(name), C.bounds(name)
    print(f"{name}: bound {C.fmt_stats(bd)}")
    for m, st in zip(C.modes(name), fam):
        print(f"    {m:4s} {C.fmt_stats(st)}")
        assert C.violation(st, bd) <= 1.0 / C.FACTOR + 1e-12
    assert all(b > 0 and np.isfinite(b) for b in bd)


# Mutants a case cannot see, with the reason (everything else must violate a bound by >= 1.5 x in every case it applies to)
INVISIBLE = {}


def test_mutants_are_detected(capsys):
    lines, missed = [], []
    for name in _SMALL:
        bd, ref = C.bounds(name), C.reference(name)
        lines.append(f"{name}: bound {C.fmt_stats(bd)}")
        for mut in C.mutants(name):
            st = C.stats(name, C.evaluate(name, "f64", mut))
            v = C.violation(st, bd)
            ok = v >= C.DETECT
            why = INVISIBLE.get((C.BY_NAME[name]["kernel"], C.BY_NAME[name]["fmt"], mut))
            mark = "" if ok else (f"   (invisible: {why})" if why else "   MISSED")
            if not ok and not why:
                missed.append((name, mut, v))
            lines.append(f"    {mut:18s} {C.fmt_stats(st)}   x {v:12.2f}{mark}")
        del ref
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not missed, missed
