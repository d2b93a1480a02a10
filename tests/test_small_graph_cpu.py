"""CPU: small skeletons and block plans of the ST-GCN recogniser - the fp64 restatement tests/small_graph_ref.py against the reference's own outputs
(tests/golden/small_graph_uncond.npz, small_graph_ntu25.npz, written by tests/golden/make_golden_small_graph.py) and against the ten-block oracle; the key
names of the Python mirrors against the reference modules' (small_graph_keys.json); the plan rules of rgn_stgcn_set_blocks through the device-free
rgn_stgcn_check_blocks; the argument errors of the evaluation CLI.

On the commit before the feature the key and plan tests fail: STGCN has no `blocks`, there is no UnconstrainedSTGCN and no rgn_stgcn_check_blocks."""
import json
import os

import numpy as np
import pytest
import torch

from regennet_amd import synth
from tests import small_graph_ref as sgr

HERE = os.path.dirname(os.path.abspath(__file__))
ATOL, RTOL = 2e-5, 1e-5                       # the ST-GCN figures of tests/test_oracle_golden.py


def _load(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))


def _golden_sd(g, **kw):
    from tests.helpers import sd_digest
    sd = synth.make_stgcn_state_dict(g["A"], seed=int(g["seed"]), **kw)
    assert sd_digest(sd) == str(g["sd_digest"])
    return sd


@pytest.mark.parametrize("tag", ["a", "short", "one"])
def test_restatement_reproduces_the_unconstrained_extractor(tag):
    g = _load("small_graph_uncond")
    sd = _golden_sd(g, num_class=12, in_channels=3, num_person=1, blocks=sgr.SIX)
    f, y = sgr.forward(sd, g[f"x_{tag}"], sgr.SIX, num_person=1)
    ref_f = g[f"features_{tag}"].reshape(f.shape)
    np.testing.assert_allclose(f.numpy(), ref_f, atol=ATOL, rtol=RTOL)
    np.testing.assert_allclose(y.numpy(), g[f"yhat_{tag}"], atol=ATOL, rtol=RTOL)


@pytest.mark.parametrize("tag", ["a", "one"])
def test_restatement_reproduces_the_25_node_recogniser(tag):
    g = _load("small_graph_ntu25")
    sd = _golden_sd(g, num_class=12, in_channels=12, num_person=2)
    f, y = sgr.forward(sd, g[f"x_{tag}"], sgr.TEN, num_person=2)
    np.testing.assert_allclose(f.numpy(), g[f"features_{tag}"].reshape(f.shape), atol=ATOL, rtol=RTOL)
    np.testing.assert_allclose(y.numpy(), g[f"yhat_{tag}"], atol=ATOL, rtol=RTOL)


def test_restatement_equals_the_ten_block_oracle():
    from oracle import stgcn_oracle
    rng = np.random.Generator(np.random.PCG64(28))
    A = sgr.tree_graph(28, 3, rng)
    sd = synth.make_stgcn_state_dict(A, num_class=13, seed=28)
    x = rng.standard_normal((2, 28, 12, 24)).astype(np.float32)
    f, y = sgr.forward(sd, x, None, num_person=2)
    of, oy = stgcn_oracle.stgcn_forward(sd, x)
    np.testing.assert_allclose(f.numpy(), of.numpy(), atol=ATOL, rtol=RTOL)
    np.testing.assert_allclose(y.numpy(), oy.numpy(), atol=ATOL, rtol=RTOL)


def _keys(model):
    return {k: list(v.shape) for k, v in model.state_dict().items()}


def test_mirrors_expose_the_reference_modules_keys_and_shapes():
    from regennet_amd.eval import STGCN, UnconstrainedSTGCN
    from regennet_amd.eval.stgcn import SIX_BLOCKS
    with open(os.path.join(HERE, "golden", "small_graph_keys.json")) as f:
        ref = json.load(f)
    un = UnconstrainedSTGCN(in_channels=3, num_class=12, graph_args={"layout": "openpose", "strategy": "spatial"}, edge_importance_weighting=True, device="cpu")
    assert _keys(un) == ref["unconstrained"]
    six = STGCN(in_channels=3, num_class=12, num_person=1, num_nodes=15, blocks=SIX_BLOCKS)
    assert _keys(six) == ref["unconstrained"]
    ten = STGCN(in_channels=12, num_class=12, num_person=2, graph_args={"layout": "ntu-rgb+d"})
    assert _keys(ten) == ref["recognition_ntu25"]
    assert _keys(STGCN(in_channels=12, num_class=12, num_person=2, num_nodes=25, blocks=None)) == ref["recognition_ntu25"]
    assert un.num_person == 1 and un.A.shape == (3, 15, 15)


def test_synthetic_checkpoint_follows_the_plan():
    from regennet_amd.eval import STGCN
    A = synth.make_stgcn_graph(15)
    sd = synth.make_stgcn_state_dict(A, num_class=12, in_channels=3, num_person=1, seed=3, blocks=sgr.SIX)
    blocks = {int(k.split(".")[1]) for k in sd if k.startswith("st_gcn_networks.")}
    assert blocks == set(range(6)) and {int(k.split(".")[1]) for k in sd if k.startswith("edge_importance.")} == set(range(6))
    assert {i for i in range(6) if f"st_gcn_networks.{i}.residual.0.weight" in sd} == {3, 5}
    assert sd["st_gcn_networks.3.tcn.2.weight"].shape == (128, 128, 9, 1) and sd["st_gcn_networks.5.gcn.conv.weight"].shape == (768, 128, 1, 1)
    model = STGCN(in_channels=3, num_class=12, num_person=1, num_nodes=15, blocks=sgr.SIX)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    assert not missing and not unexpected
    # the default's draws are those of the ten-block plan spelled out
    d0, d1 = synth.make_stgcn_state_dict(A, seed=3), synth.make_stgcn_state_dict(A, seed=3, blocks=sgr.TEN)
    assert sorted(d0) == sorted(d1) and all(np.array_equal(d0[k], d1[k]) for k in d0)


PLAN_ERRORS = [
    ([(256, 1)], "n_blocks = 1"),
    ([(64, 1)] * 10 + [(256, 1)], "n_blocks = 11"),
    ([], "n_blocks = 0"),
    ([(64, 1), (96, 1), (256, 1)], "out_channels[1] = 96"),
    ([(32, 1), (256, 1)], "out_channels[0] = 32"),
    ([(128, 1), (64, 1), (256, 1)], "out_channels[1] = 64 decreases"),
    ([(64, 1), (128, 2)], "out_channels[1] = 128: the last block must have 256"),
    ([(64, 1), (128, 3), (256, 2)], "strides[1] = 3"),
    ([(64, 1), (128, 2), (256, 0)], "strides[2] = 0"),
    ([(64, 1), (64, 2), (256, 2)], "strides[1] = 2 on a block whose channel count does not change"),
    ([(64, 2), (256, 2)], "strides[0] = 2"),
]


@pytest.mark.parametrize("plan,text", PLAN_ERRORS)
def test_plan_rules_refuse_with_the_entry_named(plan, text):
    from regennet_amd import _lib
    from regennet_amd.eval import STGCN
    with pytest.raises(_lib.RgnError) as e:
        _lib.check_stgcn_blocks(plan)
    assert e.value.code == -1 and text in str(e.value), str(e.value)
    with pytest.raises(_lib.RgnError) as e:           # the module refuses the same plans when it is built
        STGCN(in_channels=3, num_class=12, num_person=1, num_nodes=15, blocks=plan)
    assert text in str(e.value)


def test_plan_rules_accept_what_the_engine_runs():
    from regennet_amd import _lib
    for plan in (sgr.TEN, sgr.SIX, sgr.FOUR, [(64, 1), (256, 2)], [(128, 1), (256, 1), (256, 1)], [(256, 1), (256, 1)]):
        _lib.check_stgcn_blocks(plan)


CLI_ERRORS = [
    ([], "--synthetic, --synthetic_motions"),
    (["--gen_features", "a.npy"], "--gen_features and --gt_features belong together"),
    (["--gen_motions", "a.npy", "--gt_motions", "b.npy"], "--gen_motions, --gt_motions and --recogniser belong together"),
    (["--recogniser", "c.pt"], "--gen_motions, --gt_motions and --recogniser belong together"),
    (["--synthetic", "--synthetic_motions"], "one source at a time"),
    (["--synthetic_motions", "--gen_features", "a.npy", "--gt_features", "b.npy"], "one source at a time"),
    (["--gen_features", "a.npy", "--gt_features", "b.npy", "--gen_motions", "a.npy", "--gt_motions", "b.npy", "--recogniser", "c.pt"], "one source at a time"),
]


@pytest.mark.parametrize("argv,text", CLI_ERRORS)
def test_cli_argument_errors(argv, text):
    from regennet_amd.eval import unconstrained
    with pytest.raises(SystemExit) as e:
        unconstrained.main(argv)
    assert text in str(e.value), str(e.value)


def test_motion_features_refuses_motions_that_do_not_fit_the_model():
    from regennet_amd.eval import UnconstrainedSTGCN, unconstrained
    un = UnconstrainedSTGCN(in_channels=3, num_class=12, graph_args={"layout": "openpose"}, device="cpu")
    with pytest.raises(ValueError, match="motions"):
        unconstrained.motion_features(np.zeros((2, 14, 3, 8), np.float32), un)
    with pytest.raises(ValueError, match="root_joint"):
        unconstrained.motion_features(np.zeros((2, 16, 3, 8), np.float32), un, root_joint=15)
    m = unconstrained.synthetic_motions(3, seed=1)
    assert m.shape == (3, 15, 3, 60) and m.dtype == np.float32 and np.array_equal(m, unconstrained.synthetic_motions(3, seed=1))
