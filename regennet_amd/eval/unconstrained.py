"""The metric set of the reference's UNCONSTRAINED evaluation (`eval/unconstrained/evaluate.py:57-110`) on device features: FID, KID
(`metrics/kid.py`), diversity without labels (`eval/a2m/action2motion/diversity.py:6-18`) and precision / recall of the generated feature
manifold (`metrics/precision_recall.py`). For a `cond_mode='no_cond'` model the labelled metrics of `eval/metrics.py` (accuracy,
multimodality) mean nothing; these are what the reference reports instead.

    python -m regennet_amd.eval.unconstrained --synthetic --num_samples 64
    python -m regennet_amd.eval.unconstrained --gen_features gen.npy --gt_features gt.npy [--fast] [--kid_subsets 100] [--kid_subset_size 1000]
    python -m regennet_amd.eval.unconstrained --gen_motions gen.npy --gt_motions gt.npy --recogniser CKPT      # motions [N, V, 3, T] through the extractor
    python -m regennet_amd.eval.unconstrained --synthetic_motions --num_samples 64                             # seeded motions, synthetic six-block checkpoint

From motions on (`evaluate_unconstrained_motions`, evaluate.py:57-83) the features come from the reference's six-block ST-GCN on its 15-node graph
(`regennet_amd.eval.stgcn.UnconstrainedSTGCN`), on the device like everything behind it.

The features stay on the device. KID runs all subsets in ONE call of rgn_poly_mmd (no kernel matrix is ever stored; the reference pulls the
features to the host for 300 sklearn kernel matrices), precision / recall in rgn_knn_radius + rgn_manifold_hits (the reference: a Python double
loop of torch.norm calls); only the S mmd values, the two counts and the scalars come back. The index draws use NumPy's GLOBAL generator in the
reference's order, so the same `np.random.seed` selects the same rows. There is no CPU fallback: features on the CPU raise."""
import ctypes as C
import os

import numpy as np
import torch

from .. import _lib
from .fid import calculate_activation_statistics, calculate_fid
from .metrics import pair_distance_sum


def _device_features(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: the unconstrained metrics run on an AMD GPU only: pass features that live on the device (no CPU fallback)")
    if t.dim() != 2:
        raise ValueError(f"{name}: features [N, D] expected, got {tuple(t.shape)}")
    return t.detach().to(torch.float32).contiguous()


def _ck(lib, code):
    if code != _lib.RGN_OK:
        raise _lib.RgnError(code, (lib.rgn_last_error(None) or b"").decode())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def draw_subset_indices(n_g, n_r, n_subsets, subset_size):
    """The rows kid.py:16-20 draws: per subset the `g` draw, then the `r` draw, from NumPy's global generator, both with
    `replace = subset_size < n_g` (the reference's own quirk: the SECOND set's draw takes the first set's flag). A subset larger than a set it is
    drawn from without replacement raises numpy's ValueError, as there. -> (idx_g, idx_r) int32 [n_subsets, subset_size]. Host only."""
    replace = subset_size < n_g
    idx_g = np.empty((n_subsets, subset_size), np.int32)
    idx_r = np.empty((n_subsets, subset_size), np.int32)
    for i in range(n_subsets):
        idx_g[i] = np.random.choice(n_g, subset_size, replace=replace)
        idx_r[i] = np.random.choice(n_r, subset_size, replace=replace)
    return idx_g, idx_r


def poly_mmd(codes_g, codes_r, idx_g, idx_r, degree=3, gamma=None, coef0=1):
    """rgn_poly_mmd: polynomial_mmd (kid.py:29-41) of every row of the host index arrays idx_g / idx_r [S, m] in one call.
    -> (mmds, vars) fp64 [S] on the features' device."""
    X, Y = _device_features(codes_g, "codes_g"), _device_features(codes_r, "codes_r")
    if X.device != Y.device or X.shape[1] != Y.shape[1]:
        raise ValueError(f"codes_g {tuple(X.shape)} on {X.device} and codes_r {tuple(Y.shape)} on {Y.device} do not belong together")
    ig, ir = np.ascontiguousarray(idx_g, dtype=np.int32), np.ascontiguousarray(idx_r, dtype=np.int32)
    if ig.ndim != 2 or ig.shape != ir.shape:
        raise ValueError(f"index arrays {ig.shape} and {ir.shape}: two [S, m] arrays expected")
    if ig.size and (ig.min() < 0 or ig.max() >= X.shape[0] or ir.min() < 0 or ir.max() >= Y.shape[0]):
        raise ValueError(f"an index outside its feature set ({X.shape[0]} and {Y.shape[0]} rows)")
    S, m = ig.shape
    D = int(X.shape[1])
    lib, dev = _lib.load(), X.device
    need = C.c_uint64()
    _ck(lib, lib.rgn_poly_mmd_workspace(S, m, C.byref(need)))
    with torch.cuda.device(dev):
        idx = torch.from_numpy(np.stack((ig, ir))).to(dev)          # one copy: [2, S, m]
        work = torch.empty(max(int(need.value), 16), dtype=torch.uint8, device=dev)
        out = torch.empty((2, S), dtype=torch.float64, device=dev)
        g = np.float32(1.0 / D if gamma is None else gamma)         # sklearn: K *= gamma on the fp32 matrix
        _ck(lib, lib.rgn_poly_mmd(dev.index, _lib._ptr(X), int(X.shape[0]), _lib._ptr(Y), int(Y.shape[0]), D, _lib._ptr(idx[0]), _lib._ptr(idx[1]), S, m,
                                  int(degree), float(g), float(np.float32(coef0)), _lib._ptr(out[0]), _lib._ptr(out[1]), _lib._ptr(work),
                                  int(work.numel()), _stream(dev)))
    return out[0], out[1]


def polynomial_mmd_averages(codes_g, codes_r, n_subsets=50, subset_size=1000, ret_var=True, degree=3, gamma=None, coef0=1):
    """kid.py:8-27. -> (mmds, vars) fp64 numpy [n_subsets] (mmds alone without ret_var)."""
    for name, t in (("codes_g", codes_g), ("codes_r", codes_r)):
        _device_features(t, name)
    idx_g, idx_r = draw_subset_indices(len(codes_g), len(codes_r), n_subsets, subset_size)
    mmds, vars_ = poly_mmd(codes_g, codes_r, idx_g, idx_r, degree=degree, gamma=gamma, coef0=coef0)
    return (mmds.cpu().numpy(), vars_.cpu().numpy()) if ret_var else mmds.cpu().numpy()


def calculate_kid(real_activations, generated_activations, n_subsets=100, subset_size=1000):
    """kid.py:133-136: (mean, std) of the subsets' mmd2, numpy's population std; `real` goes in as codes_g exactly as there."""
    kid_values = polynomial_mmd_averages(real_activations, generated_activations, n_subsets=n_subsets, subset_size=subset_size)
    return kid_values[0].mean(), kid_values[0].std()


def knn_radius(A_features, k):
    """rgn_knn_radius (precision_recall.py:34-42): fp32 [N], the k-th smallest distance of every row to the rows of its own set (itself included)."""
    A = _device_features(A_features, "A_features")
    lib, dev = _lib.load(), A.device
    with torch.cuda.device(dev):
        radii = torch.empty(A.shape[0], dtype=torch.float32, device=dev)
        _ck(lib, lib.rgn_knn_radius(dev.index, _lib._ptr(A), int(A.shape[0]), int(A.shape[1]), int(k), _lib._ptr(radii), _stream(dev)))
    return radii


def manifold_hits(B_features, A_features, radii):
    """rgn_manifold_hits (precision_recall.py:44-53): (flags uint8 [M], count int32 [1]) on the device."""
    B, A = _device_features(B_features, "B_features"), _device_features(A_features, "A_features")
    if B.device != A.device or B.shape[1] != A.shape[1] or tuple(radii.shape) != (A.shape[0],) or radii.dtype != torch.float32 or radii.device != A.device:
        raise ValueError(f"B {tuple(B.shape)}, A {tuple(A.shape)} and radii {tuple(radii.shape)} do not belong together")
    lib, dev, radii = _lib.load(), A.device, radii.contiguous()
    with torch.cuda.device(dev):
        flags = torch.empty(B.shape[0], dtype=torch.uint8, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        _ck(lib, lib.rgn_manifold_hits(dev.index, _lib._ptr(B), int(B.shape[0]), _lib._ptr(A), _lib._ptr(radii), int(A.shape[0]),
                                       int(A.shape[1]), _lib._ptr(flags), _lib._ptr(count), _stream(dev)))
    return flags, count


def manifold_estimate(A_features, B_features, k):
    """precision_recall.py:30-53: the share of B's rows inside the k-NN manifold of A."""
    radii = knn_radius(A_features, k)
    _, count = manifold_hits(B_features, A_features, radii)
    return int(count.item()) / len(B_features)


def precision_and_recall(generated_features, real_features):
    """precision_recall.py:12-28: k = 3, both sets cut to the shorter one. -> (precision, recall), or None without data."""
    k = 3
    data_num = min(len(generated_features), len(real_features))
    if data_num <= 0:
        print("there is no data")
        return None
    generated_features, real_features = generated_features[:data_num], real_features[:data_num]
    precision = manifold_estimate(real_features, generated_features, k)
    recall = manifold_estimate(generated_features, real_features, k)
    return precision, recall


def calculate_diversity(activations):
    """diversity.py:6-18: the mean distance of 200 np.random.randint pairs, as one batched distance sum on the device."""
    diversity_times = 200
    act = _device_features(activations, "activations")
    num_motions = len(act)
    first_indices = np.random.randint(0, num_motions, diversity_times)
    second_indices = np.random.randint(0, num_motions, diversity_times)
    return pair_distance_sum(act, first_indices, second_indices) / diversity_times


def evaluate_unconstrained_metrics(generated_features, real_features, fast=False, kid_subsets=100, kid_subset_size=1000, log=None):
    """evaluate.py:84-110 from the two feature sets on: the reference's dict {'fid', 'kid', 'diversity_gen', 'diversity_gt', 'precision',
    'recall'} ('kid' is the mean; precision and recall are None under `fast`). The random draws come in the reference's order: KID, the
    dataset's diversity, the generated set's. `log`: a callable that receives the reference's printed lines (with KID's std)."""
    log = log or (lambda line: None)
    gen, real = _device_features(generated_features, "generated_features"), _device_features(real_features, "real_features")
    generated_stats, real_stats = calculate_activation_statistics(gen), calculate_activation_statistics(real)
    fid = float(calculate_fid(generated_stats, real_stats))
    log(f"FID score: {fid}")
    kid = calculate_kid(real, gen, n_subsets=kid_subsets, subset_size=kid_subset_size)
    log("KID : %.3f (%.3f)" % kid)
    dataset_diversity = calculate_diversity(real)
    generated_diversity = calculate_diversity(gen)
    log(f"Diversity of generated motions: {generated_diversity.item()}")
    log(f"Diversity of dataset motions: {dataset_diversity.item()}")
    if fast:
        log("Skipping precision-recall calculation")
        precision = recall = None
    else:
        precision, recall = precision_and_recall(gen, real)
        log(f"precision: {precision}")
        log(f"recall: {recall}")
    return {"fid": fid, "kid": float(kid[0]), "diversity_gen": generated_diversity.item(), "diversity_gt": dataset_diversity.item(),
            "precision": precision, "recall": recall}


def initialize_model(device, modelpath, num_classes=12):
    """evaluate.py:21-32: the six-block extractor on the 15-node 'openpose' graph, 3 input channels, 12 classes, with the checkpoint at `modelpath`
    (a state_dict, or an already loaded dict of tensors / arrays)."""
    from .stgcn import UnconstrainedSTGCN
    model = UnconstrainedSTGCN(in_channels=3, num_class=num_classes, graph_args={"layout": "openpose", "strategy": "spatial"},
                               edge_importance_weighting=True, device=device)
    state_dict = modelpath if isinstance(modelpath, dict) else torch.load(modelpath, map_location="cpu")
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)) if not isinstance(v, torch.Tensor) else v for k, v in state_dict.items()})
    model = model.to(device)
    model.eval()
    return model


def compute_features(model, iterator, device):
    """evaluate.py:41-54: (activations [N, 256], predictions [N, num_class]) of the batches [n, V, C, T] of `iterator`, on the device."""
    activations, predictions = [], []
    with torch.no_grad():
        for batch in iterator:
            batch_for_model = {"x": torch.as_tensor(batch).to(device).float()}
            model(batch_for_model)
            activations.append(batch_for_model["features"].reshape(-1, 256).clone())     # (a batch of one is squeezed to [256] there and would not concatenate)
            predictions.append(batch_for_model["yhat"].clone())
    return torch.cat(activations, dim=0), torch.cat(predictions, dim=0)


def _batches(motions, batch_size):
    return (motions[lo:lo + batch_size] for lo in range(0, len(motions), batch_size))


def motion_features(motions, model, root_joint=8, batch_size=64, num_nodes=None):
    """evaluate.py:65-70 / :76-81 for one set: motions [N, >= V, C, T] cut to the model's V vertices (the dataset carries a 16th joint, :76), centred on
    the root joint per frame (:65, :77; not in place), through the extractor in batches. -> (features, predictions) on the model's device."""
    dev = model.A.device
    V = int(num_nodes or model.A.shape[1])
    m = torch.as_tensor(np.asarray(motions) if not isinstance(motions, torch.Tensor) else motions).to(device=dev, dtype=torch.float32)
    if m.dim() != 4 or m.shape[1] < V:
        raise ValueError(f"motions [N, >= {V}, C, T] expected, got {tuple(m.shape)}")
    if not 0 <= root_joint < V:
        raise ValueError(f"root_joint {root_joint} outside the model's {V} vertices")
    m = m[:, :V]
    m = m - m[:, root_joint:root_joint + 1]
    return compute_features(model, _batches(m, batch_size), dev)


def evaluate_unconstrained_motions(generated_motions, dataset_motions, model, fast=False, root_joint=8, batch_size=64, kid_subsets=100,
                                   kid_subset_size=1000, log=None):
    """evaluate.py:57-110 from motions on: both sets centred on the root joint per frame (:65, :77), the dataset cut to the model's vertex count
    (:76), features in batches of `batch_size` (:67, :78), then `evaluate_unconstrained_metrics` (unchanged) on the two feature sets."""
    gen, _ = motion_features(generated_motions, model, root_joint, batch_size)
    real, _ = motion_features(dataset_motions, model, root_joint, batch_size)
    return evaluate_unconstrained_metrics(gen, real, fast=fast, kid_subsets=kid_subsets, kid_subset_size=kid_subset_size, log=log)


def synthetic_motions(n, seed, V=15, T=60):
    """Seeded stand-ins for joint positions [n, V, 3, T]: a smooth random walk per joint around a fixed rest pose."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rest = np.random.Generator(np.random.PCG64(4711)).standard_normal((1, V, 3, 1))
    return (rest + 0.1 * np.cumsum(rng.standard_normal((n, V, 3, T)), axis=3)).astype(np.float32)


def synthetic_recogniser(dev, V=15, seed=0):
    """A synthetic six-block checkpoint on a synthetic V-node tree, loaded as `initialize_model` loads a real one."""
    from .. import synth
    from .stgcn import SIX_BLOCKS
    sd = synth.make_stgcn_state_dict(synth.make_stgcn_graph(V), num_class=12, in_channels=3, num_person=1, seed=seed, blocks=SIX_BLOCKS)
    return initialize_model(dev, sd)


def _synthetic_features(args, dev):
    """--synthetic: sample an unconstrained model twice (the second seed stands in for the ground truth) and pass both sets, concatenated with
    their actors as eval/a2m/stgcn_eval.py:71 does, through a synthetic recogniser."""
    from .. import synth
    from .stgcn import STGCN
    cfg = synth.get_config("ntu")
    model, diffusion = synth.build_model(cfg, synth.make_state_dict(cfg, seed=0), resp=args.timestep_respacing, device=str(dev))
    rec_sd = synth.make_stgcn_state_dict(synth.make_stgcn_graph(cfg["njoints"]), num_class=26, seed=0)
    rec = STGCN(in_channels=2 * cfg["nfeats"], num_class=26, num_person=2, num_nodes=cfg["njoints"], device=str(dev))
    rec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in rec_sd.items()}, strict=True)
    rec.to(dev).eval()
    feats = []
    for seed in (args.seed, args.seed + 1):
        parts = []
        for lo in range(0, args.num_samples, args.batch_size):
            nb = min(args.batch_size, args.num_samples - lo)
            cm = torch.from_numpy(synth.make_cmotion(cfg, nb, seed=1000 * (seed + 1) + lo)).to(dev)
            x = diffusion.p_sample_loop(model, (nb, cfg["njoints"], cfg["nfeats"], cfg["num_frames"]), clip_denoised=False,
                                        model_kwargs={"y": {"cmotion": cm}}, seed=seed, sample_offset=lo)
            parts.append(rec({"output": torch.cat((cm, x), dim=2)})["features"].reshape(nb, -1).clone())
        feats.append(torch.cat(parts))
    model._engine.close()
    return feats[0], feats[1]


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--synthetic", action="store_true", help="sample a synthetic unconstrained model; a second seed is the 'ground truth'")
    ap.add_argument("--gen_features", help="FILE.npy [N, D]: features of the generated motions")
    ap.add_argument("--gt_features", help="FILE.npy [N, D]: features of the dataset's motions")
    ap.add_argument("--gen_motions", help="FILE.npy [N, V, 3, T]: generated motions (joint positions), with --gt_motions and --recogniser")
    ap.add_argument("--gt_motions", help="FILE.npy [N, >= V, 3, T]: the dataset's motions (cut to the recogniser's V joints)")
    ap.add_argument("--recogniser", help="checkpoint (state_dict) of the six-block ST-GCN extractor (evaluate.py:21-32)")
    ap.add_argument("--synthetic_motions", action="store_true", help="seeded motions (a second seed is the 'ground truth') through a synthetic six-block checkpoint")
    ap.add_argument("--root_joint", type=int, default=8, help="the joint every frame is centred on (evaluate.py:65)")
    ap.add_argument("--num_samples", type=int, default=64)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--timestep_respacing", default="ddim5")
    ap.add_argument("--seed", type=int, default=10)
    ap.add_argument("--fast", action="store_true", help="skip precision / recall (evaluate.py:99-101)")
    ap.add_argument("--kid_subsets", type=int, default=100)
    ap.add_argument("--kid_subset_size", type=int, default=0, help="default: 1000 (kid.py), cut to the smaller feature set")
    ap.add_argument("--output_dir", default=".")
    args = ap.parse_args(argv)
    USAGE = ("--synthetic, --synthetic_motions, --gen_features A.npy with --gt_features B.npy, or --gen_motions A.npy with --gt_motions B.npy "
             "and --recogniser CKPT")
    motions, features = (args.gen_motions, args.gt_motions, args.recogniser), (args.gen_features, args.gt_features)
    modes = [bool(args.synthetic), bool(args.synthetic_motions), any(features), any(motions)]
    if sum(modes) > 1:
        raise SystemExit("one source at a time: " + USAGE)
    if any(motions) and not all(motions):
        raise SystemExit("--gen_motions, --gt_motions and --recogniser belong together: " + USAGE)
    if any(features) and not all(features):
        raise SystemExit("--gen_features and --gt_features belong together: " + USAGE)
    if sum(modes) == 0:
        raise SystemExit(USAGE)
    if not torch.cuda.is_available():
        raise SystemExit("the unconstrained metrics run on an AMD GPU only (no CPU fallback)")
    dev = torch.device("cuda:0")
    if args.synthetic:
        gen, gt = _synthetic_features(args, dev)
    elif args.synthetic_motions:
        rec = synthetic_recogniser(dev)
        gen, gt = (motion_features(synthetic_motions(args.num_samples, s), rec, args.root_joint, args.batch_size)[0] for s in (args.seed, args.seed + 1))
    elif all(motions):
        rec = initialize_model(dev, args.recogniser)
        gen, gt = (motion_features(np.load(p, allow_pickle=True), rec, args.root_joint, args.batch_size)[0] for p in (args.gen_motions, args.gt_motions))
    else:
        gen, gt = (torch.from_numpy(np.asarray(np.load(p), dtype=np.float32)).to(dev) for p in (args.gen_features, args.gt_features))
    np.random.seed(args.seed)
    size = args.kid_subset_size or min(1000, len(gen), len(gt))
    print(f"{len(gen)} generated and {len(gt)} dataset features of {gen.shape[1]} dimensions; KID over {args.kid_subsets} subsets of {size}")
    metrics = evaluate_unconstrained_metrics(gen, gt, fast=args.fast, kid_subsets=args.kid_subsets, kid_subset_size=size, log=print)
    os.makedirs(args.output_dir, exist_ok=True)
    path = os.path.join(args.output_dir, "metrics.npy")
    np.save(path, metrics)
    print(f"saved the metrics to [{os.path.abspath(path)}]")
    return metrics


if __name__ == "__main__":
    main()
