"""GPU: the recogniser on skeletons of fewer than 28 joints and on block plans other than the reference's ten - the six-block extractor of the
unconstrained evaluation (15 joints) and the 25-joint layouts - against outputs of the reference itself (tests/golden/small_graph_*.npz) and the fp64
restatement tests/small_graph_ref.py. The bound is the project's own (tests/test_eval_gpu.py): 1e-4 * max(1, max |ref|) on features and logits, equal
argmax. Every test prints its parity figure before it asserts (profiles/small_graph_parity.txt is that output).

On the commit before the feature every test here fails: rgn_stgcn_finalize refuses fewer than 28 nodes and there is no block plan."""
import functools
import os

import numpy as np
import pytest
import torch

from regennet_amd import synth
from tests import small_graph_ref as sgr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BOUND = 1e-4
F16_BOUND = 1.5e-3
PLANS = {"six": sgr.SIX, "ten": sgr.TEN, "four": sgr.FOUR}


def _t(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _stgcn(sd, V, in_channels, persons, plan, num_class, opts=None):
    from regennet_amd.eval import STGCN
    model = STGCN(in_channels=in_channels, num_class=num_class, num_person=persons, num_nodes=V, device="cuda:0", blocks=None if plan == "ten" else PLANS[plan])
    missing, unexpected = model.load_state_dict(_t(sd), strict=True)
    assert not missing and not unexpected
    model.engine_options = dict(opts or {})
    return model.to("cuda:0").eval()


def _check(tag, feats, yhat, ref_f, ref_y, bound=BOUND):
    feats, yhat = np.asarray(feats, np.float64).reshape(np.asarray(ref_f).shape), np.asarray(yhat, np.float64)
    ref_f, ref_y = np.asarray(ref_f, np.float64), np.asarray(ref_y, np.float64)
    ef, ey = np.abs(feats - ref_f).max(), np.abs(yhat - ref_y).max()
    print(f"\n[small graph {tag}] max |features - ref| = {ef:.2e} (|ref| max {np.abs(ref_f).max():.2f}, bound {bound * max(1.0, np.abs(ref_f).max()):.2e}), "
          f"logits {ey:.2e} (|ref| max {np.abs(ref_y).max():.2f})")
    assert np.isfinite(feats).all() and np.isfinite(yhat).all()
    assert ef < bound * max(1.0, np.abs(ref_f).max()), (tag, ef)
    assert ey < bound * max(1.0, np.abs(ref_y).max()), (tag, ey)
    assert np.array_equal(yhat.argmax(1), ref_y.argmax(1)), tag


@functools.lru_cache(maxsize=None)
def _golden(name):
    from tests.helpers import sd_digest
    g = dict(np.load(os.path.join(HERE, "golden", name + ".npz")))
    kw = dict(num_class=12, in_channels=3, num_person=1, blocks=sgr.SIX) if name == "small_graph_uncond" else dict(num_class=12, in_channels=12, num_person=2)
    sd = synth.make_stgcn_state_dict(g["A"], seed=int(g["seed"]), **kw)
    assert sd_digest(sd) == str(g["sd_digest"])
    return g, sd


# ---- 1. the reference's own outputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "short", "one"])
def test_unconstrained_extractor_matches_the_reference(tag):
    """eval/unconstrained/models/stgcn.py on the 15-node graph: [5, 15, 3, 60], [2, 15, 3, 7] (fewer frames than the nine taps; T goes 7 -> 4 -> 2 through the
    two stride-2 blocks) and [1, 15, 3, 24] (features squeezed to [256])."""
    from regennet_amd.eval import UnconstrainedSTGCN
    g, sd = _golden("small_graph_uncond")
    model = UnconstrainedSTGCN(in_channels=3, num_class=12, graph_args={"layout": "openpose", "strategy": "spatial"}, edge_importance_weighting=True, device="cuda:0")
    missing, unexpected = model.load_state_dict(_t(sd), strict=True)
    assert not missing and not unexpected
    model = model.to("cuda:0").eval()
    batch = model({"x": torch.from_numpy(g[f"x_{tag}"]).cuda()})
    assert batch["features"].shape == torch.from_numpy(g[f"features_{tag}"]).shape           # N == 1 squeezes to [256]
    _check(f"uncond {tag}", batch["features"].cpu().numpy(), batch["yhat"].cpu().numpy(), g[f"features_{tag}"], g[f"yhat_{tag}"])


@pytest.mark.parametrize("tag", ["a", "one"])
def test_25_node_recogniser_matches_the_reference(tag):
    from regennet_amd.eval import STGCN
    g, sd = _golden("small_graph_ntu25")
    model = STGCN(in_channels=12, num_class=12, num_person=2, graph_args={"layout": "ntu-rgb+d", "strategy": "spatial"}, edge_importance_weighting=True, device="cuda:0")
    model.load_state_dict(_t(sd), strict=True)
    model = model.to("cuda:0").eval()
    batch = model({"output": torch.from_numpy(g[f"x_{tag}"]).cuda()})
    assert batch["features"].shape == torch.from_numpy(g[f"features_{tag}"]).shape
    _check(f"ntu25 {tag}", batch["features"].cpu().numpy(), batch["yhat"].cpu().numpy(), g[f"features_{tag}"], g[f"yhat_{tag}"])


# ---- 2. other skeletons against the restatement -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(V, hub, T, N, plan, persons, in_channels, bias=None):
    """(checkpoint, input, fp64 features, fp64 logits) of a random tree: computed once, shared, never modified."""
    rng = np.random.Generator(np.random.PCG64(3000 + 37 * V + hub))
    A = sgr.tree_graph(V, hub, rng)
    sd = synth.make_stgcn_state_dict(A, num_class=13, in_channels=in_channels, num_person=persons, seed=V, blocks=None if plan == "ten" else PLANS[plan])
    if bias is not None:
        for k in sd:
            if k.endswith("tcn.3.bias") or k == "data_bn.bias":
                sd[k] = np.full_like(sd[k], bias)
    x = rng.standard_normal((N, V, in_channels, T)).astype(np.float32)
    f, y = sgr.forward(sd, x, PLANS[plan], num_person=persons)
    return sd, x, f.numpy(), y.numpy()


CASES = [(15, 3, 24, 3, "six", 1, 3), (2, 1, 24, 2, "six", 1, 3), (16, 3, 24, 2, "ten", 2, 12), (17, 4, 30, 2, "ten", 2, 12), (21, 9, 24, 2, "ten", 2, 12),
         (24, 2, 9, 2, "ten", 2, 12), (25, 2, 150, 1, "ten", 2, 12), (27, 3, 20, 2, "six", 1, 6), (15, 3, 24, 2, "four", 1, 3)]


@pytest.mark.parametrize("V,hub,T,N,plan,persons,in_channels", CASES)
def test_other_small_skeletons_match_the_restatement(V, hub, T, N, plan, persons, in_channels):
    """Padded vertex counts 16 (V = 2, 15, 16: no padding at 16, bias period 32), 20, 24 (a hub beyond the 8 aggregation slots: two-launch form), 28; nine
    and 150 frames; one and two persons; 3, 6 and 6 + 6 channels; the six-, ten- and a four-block plan (two stride-2 blocks in a row)."""
    sd, x, ref_f, ref_y = _case(V, hub, T, N, plan, persons, in_channels)
    model = _stgcn(sd, V, in_channels, persons, plan, 13)
    batch = model({"output": torch.from_numpy(x).cuda()})
    _check(f"V={V} hub={hub} T={T} N={N} {plan}", batch["features"].cpu().numpy(), batch["yhat"].cpu().numpy(), ref_f, ref_y)


# ---- 3. pad rows never reach the features --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,plan,persons,in_channels", [(15, "six", 1, 3), (25, "ten", 2, 12)])
def test_pad_vertices_never_reach_the_features(V, plan, persons, in_channels):
    """tcn.3.bias = data_bn.bias = +5 everywhere: behind every temporal convolution a pad vertex's row holds relu(5 + ...), growing through the identity
    residuals. The features must not see it (the pool skips the pad rows; no aggregation list names them)."""
    sd, x, ref_f, ref_y = _case(V, 3, 24, 2, plan, persons, in_channels, bias=5.0)
    model = _stgcn(sd, V, in_channels, persons, plan, 13)
    batch = model({"output": torch.from_numpy(x).cuda()})
    _check(f"pad rows V={V} {plan}", batch["features"].cpu().numpy(), batch["yhat"].cpu().numpy(), ref_f, ref_y)


# ---- 4. many tiles ------------------------------------------------------------------------------------------------------------------------------------
def test_many_tiles_per_workgroup_on_the_15_node_graph():
    """V = 15, six blocks, T = 60, N = 96: 384 tiles of 256 rows in the first blocks - more than one tile per workgroup, windows in flight across tile
    boundaries. The whole batch against the same motions four at a time (bit for bit) and three motions against the restatement."""
    V, T, N = 15, 60, 96
    sd, _, _, _ = _case(V, 3, 24, 3, "six", 1, 3)
    model = _stgcn(sd, V, 3, 1, "six", 13)
    x = np.random.Generator(np.random.PCG64(96)).standard_normal((N, V, 3, T)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    big = model({"output": xd})
    feats, yhat = big["features"].reshape(N, -1).clone(), big["yhat"].clone()
    for i in range(0, N, 4):
        part = model({"output": xd[i:i + 4]})
        assert torch.equal(part["features"].reshape(-1, 256), feats[i:i + 4]), (i, (part["features"] - feats[i:i + 4]).abs().max().item())
        assert torch.equal(part["yhat"], yhat[i:i + 4]), i
    sel = [0, N // 2, N - 1]
    ref_f, ref_y = sgr.forward(sd, x[sel], sgr.SIX, num_person=1)
    _check("many tiles V=15 T=60 N=96", feats[sel].cpu().numpy(), yhat[sel].cpu().numpy(), ref_f.numpy(), ref_y.numpy())


# ---- 5. every selectable form ---------------------------------------------------------------------------------------------------------------------------
FORMS = [{"SG_NO_WINDOW": 1}, {"SG_NO_GCN_FUSE": 1}, {"SG_NO_TAIL_FUSE": 1}, {"SG_NO_POLY_TAIL": 1}, {"SG_NO_S2_WINDOW": 1}, {"SG_NO_BLOCK0_FUSE": 1}, {"SG_GCN_BN": 64}]


@pytest.mark.parametrize("opts", FORMS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
@pytest.mark.parametrize("V,plan,persons,in_channels", [(15, "six", 1, 3), (25, "ten", 2, 12)])
def test_every_selectable_form_on_small_graphs(V, plan, persons, in_channels, opts):
    hub, T, N = (3, 24, 3) if V == 15 else (2, 24, 2)
    sd, x, ref_f, ref_y = _case(V, hub, T, N, plan, persons, in_channels)
    model = _stgcn(sd, V, in_channels, persons, plan, 13, opts)
    batch = model({"output": torch.from_numpy(x).cuda()})
    _check(f"form {opts} V={V} {plan}", batch["features"].cpu().numpy(), batch["yhat"].cpu().numpy(), ref_f, ref_y)


# ---- 6. SG_F16 --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,plan,persons,in_channels", [(15, "six", 1, 3), (25, "ten", 2, 12)])
def test_fp16_form_on_a_small_graph_is_served_or_refused_aloud(V, plan, persons, in_channels):
    """SG_F16 on a small graph: parity at the project's fp16 bound, or RGN_ERR_UNSUPPORTED with the reason - never a silent change of arithmetic."""
    from regennet_amd import _lib
    hub, T, N = (3, 24, 3) if V == 15 else (2, 24, 2)
    sd, x, ref_f, ref_y = _case(V, hub, T, N, plan, persons, in_channels)
    model = _stgcn(sd, V, in_channels, persons, plan, 13, {"SG_F16": 1})
    try:
        batch = model({"output": torch.from_numpy(x).cuda()})
    except _lib.RgnError as e:
        print(f"\n[small graph f16 V={V}] refused: {e}")
        assert e.code == _lib.RGN_ERR_UNSUPPORTED and "fused kernels only" in str(e)
        return
    _check(f"f16 V={V} {plan}", batch["features"].cpu().numpy(), batch["yhat"].cpu().numpy(), ref_f, ref_y, bound=F16_BOUND)


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------------------------------
def _engine(sd, V, in_channels, persons, blocks, drop=()):
    from regennet_amd import _lib
    eng = _lib.StgcnEngine(in_channels, 13, persons, V, 24, 2, 0, blocks=blocks)
    for k, v in sd.items():
        if not k.endswith("num_batches_tracked") and k not in drop:
            eng.load_weight(k, np.asarray(v, np.float32))
    return eng


def test_plan_errors_through_the_handle():
    from regennet_amd import _lib
    sd6, _, _, _ = _case(15, 3, 24, 3, "six", 1, 3)
    sd10, _, _, _ = _case(16, 3, 24, 2, "ten", 2, 12)
    for plan, text in (([(256, 1)], "n_blocks = 1"), ([(64, 1), (96, 1), (256, 1)], "out_channels[1] = 96"), ([(64, 1), (64, 2), (256, 2)], "strides[1] = 2"),
                       ([(64, 1), (128, 2)], "the last block must have 256"), ([(128, 1), (64, 1), (256, 1)], "decreases")):
        with pytest.raises(_lib.RgnError) as e:
            _lib.StgcnEngine(3, 13, 1, 15, 24, 2, 0, blocks=plan)
        assert e.value.code == -1 and text in str(e.value) and "rgn_stgcn_set_blocks" in str(e.value), str(e.value)
    eng = _engine(sd6, 15, 3, 1, sgr.SIX)
    eng.finalize()
    with pytest.raises(_lib.RgnError) as e:                      # the plan is fixed once the weights are folded
        eng.set_blocks(sgr.SIX)
    assert e.value.code == -5 and "already finalized" in str(e.value)
    eng.close()
    eng = _engine(sd10, 16, 12, 2, sgr.SIX)                      # a six-block plan fed a ten-block checkpoint
    with pytest.raises(_lib.RgnError) as e:
        eng.finalize()
    assert e.value.code == -2 and "edge_importance.6" in str(e.value) and "6 blocks" in str(e.value), str(e.value)
    eng.close()
    eng = _engine(sd6, 15, 3, 1, sgr.SIX, drop=("st_gcn_networks.5.residual.0.weight",))
    with pytest.raises(_lib.RgnError) as e:
        eng.finalize()
    assert e.value.code == -4 and "st_gcn_networks.5.residual.0.weight" in str(e.value), str(e.value)
    eng.close()
    eng = _engine(sd6, 15, 3, 1, None)                           # the default plan asks for the ten blocks' keys
    with pytest.raises(_lib.RgnError) as e:
        eng.finalize()
    assert e.value.code == -4 and "st_gcn_networks.6.gcn.conv.weight" in str(e.value)
    eng.close()


# ---- 8. end to end ----------------------------------------------------------------------------------------------------------------------------------------------
def test_unconstrained_evaluation_from_motions():
    """evaluate_unconstrained_motions = centring + cut + compute_features + evaluate_unconstrained_metrics, exactly; a per-frame shift of every joint does
    not move the features beyond the bound."""
    from regennet_amd.eval import unconstrained as un
    dev = torch.device("cuda:0")
    model = un.synthetic_recogniser(dev)
    gen = un.synthetic_motions(64, seed=10)
    gt = np.concatenate((un.synthetic_motions(64, seed=11), np.ones((64, 1, 3, 60), np.float32)), axis=1)       # a 16th joint, as the dataset carries (evaluate.py:76)
    gen0, gt0 = gen.copy(), gt.copy()
    np.random.seed(5)
    got = un.evaluate_unconstrained_motions(gen, gt, model, kid_subsets=10, kid_subset_size=32)
    assert np.array_equal(gen, gen0) and np.array_equal(gt, gt0)                                                 # (the reference centres in place; this does not)

    def feats(m):
        m = torch.from_numpy(m[:, :15] - m[:, 8:9]).to(dev)
        return un.compute_features(model, (m[i:i + 64] for i in range(0, len(m), 64)), dev)[0]

    fg, fr = feats(gen), feats(gt)
    np.random.seed(5)
    want = un.evaluate_unconstrained_metrics(fg, fr, kid_subsets=10, kid_subset_size=32)
    print(f"\n[small graph e2e] {got}")
    assert got == want and set(got) == {"fid", "kid", "diversity_gen", "diversity_gt", "precision", "recall"}
    assert fg.shape == (64, 256) and np.isfinite(got["fid"]) and got["precision"] is not None
    shift = np.random.Generator(np.random.PCG64(1)).standard_normal((64, 1, 3, 60)).astype(np.float32)
    fs = un.motion_features(gen + shift, model)[0]
    err, top = (fs - fg).abs().max().item(), fg.abs().max().item()
    print(f"[small graph e2e] shifted motions: max |features - features| = {err:.2e} (|features| max {top:.2f})")
    assert err < BOUND * max(1.0, top)
    f1 = un.motion_features(gen[:1], model)[0]                                                                    # a batch of one still concatenates
    assert f1.shape == (1, 256) and torch.equal(f1, un.motion_features(gen[:3], model, batch_size=1)[0][:1])


def test_smpl_layout_of_the_evaluation_runs():
    """eval/a2m/stgcn/evaluate.py:11-12 with body_model='smpl': the 25-node layout through regennet_amd.eval.Evaluation."""
    from regennet_amd.eval import Evaluation
    g, sd = _golden("small_graph_ntu25")
    ev = Evaluation("ntu", "smpl", {"nfeats": 12, "num_classes": 12, "num_person": 2, "state_dict": _t(sd)}, torch.device("cuda:0"), seed=0)
    x = torch.from_numpy(g["x_a"]).cuda()
    acts, labels, acc = ev.compute_features_and_accuracy([{"output": x, "y": torch.from_numpy(g["yhat_a"]).max(dim=1).indices}])
    _check("smpl layout", acts.cpu().numpy(), ev.model({"output": x})["yhat"].cpu().numpy(), g["features_a"], g["yhat_a"])
    assert acc == 1.0 and labels.shape == (3,)
