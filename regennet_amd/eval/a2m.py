"""The action2motion evaluation on device tensors: accuracy, FID, diversity and multimodality of HumanAct12-style motions under the GRU action
classifier - mirror of the reference's `eval/a2m/action2motion/{evaluate,accuracy}.py` and of the driver `eval/a2m/gru_eval.py`.

    python -m regennet_amd.eval.a2m --synthetic --num_samples 64
    python -m regennet_amd.eval.a2m --gen_xyz A.npy --gt_xyz B.npy [--gt2_xyz C.npy] --labels Y.npy --lengths L.npy --classifier CKPT

The classifier is `regennet_amd.eval.gru` (one HIP launch per batch, rgn_gru_forward); the pair metrics are `metrics.calculate_diversity_multimodality`
and FID is `fid.calculate_fid`, both on the features' device. The index draws use NumPy's global generator exactly like the reference."""
import os

import numpy as np
import torch

from .fid import calculate_activation_statistics, calculate_fid
from .gru import load_classifier
from .metrics import calculate_diversity_multimodality, pair_distance_sum

UNCONSTRAINED_JOINTS = [15, 12, 16, 18, 20, 17, 19, 21, 0, 1, 4, 7, 2, 5, 8]      # gru_eval.py:116: the 15-joint cut of the 24 SMPL joints


def calculate_accuracy_a2m(model, motion_loader, num_labels, classifier, device):
    """accuracy.py:4-14 for batches {"output_xyz", "lengths", "y"}: (accuracy, confusion [num_labels, num_labels] int64). Each batch draws a fresh
    hidden state, as the reference's classifier does."""
    confusion = torch.zeros(num_labels, num_labels, dtype=torch.long)
    with torch.no_grad():
        for batch in motion_loader:
            pred = classifier(batch["output_xyz"], lengths=batch["lengths"]).max(dim=1).indices.cpu()
            y = torch.as_tensor(batch["y"]).cpu().long().reshape(-1)
            confusion.index_put_((y, pred), torch.ones_like(y), accumulate=True)
    return (torch.trace(confusion) / torch.sum(confusion)).item(), confusion


class A2MEvaluation:
    """evaluate.py:9-84. `state_dict` (reference key names; arrays or tensors) or `model_path` (a reference checkpoint, its "model" entry) gives the
    classifier; `seed` fixes NumPy's index draws and torch's hidden-state draws of every `evaluate` call.

    ONE forward per batch serves both the accuracy and the features (`forward_both`), where the reference runs its two classifier objects over the
    loader one after the other (evaluate.py:52-59) - and so with two DIFFERENT torch.randn hidden states per batch. Here logits and features of a
    batch share one draw: the same distribution, not the same random stream as the reference's."""

    def __init__(self, device, state_dict=None, model_path=None, seed=None, classifier=None):
        dataset_opt = {"input_size_raw": 72, "joints_num": 24, "num_classes": 12}          # evaluate.py:11
        self.input_size_raw, self.num_classes, self.device, self.seed = dataset_opt["input_size_raw"], dataset_opt["num_classes"], device, seed
        if classifier is None:
            kw = {"state_dict": state_dict} if state_dict is not None else ({"model_path": model_path} if model_path else {})
            classifier = load_classifier(self.input_size_raw, self.num_classes, device, **kw)
        self.gru_classifier = classifier            # one module: MotionDiscriminatorForFID differs in what forward returns, not in weights
        self.hidden_layer, self.hidden_size = 2, 128                                        # models.py:69

    def _forward(self, batch):
        x = torch.as_tensor(batch["output_xyz"]).to(self.device)
        hidden = torch.randn(self.hidden_layer, x.shape[0], self.hidden_size, device=self.device)         # initHidden, models.py:40-41
        return self.gru_classifier.forward_both(x, lengths=torch.as_tensor(batch["lengths"]).to(self.device), hidden_unit=hidden)

    def compute_features(self, model, motionloader):
        """evaluate.py:21-34: (activations [N, 30], labels [N] or [] for cond_mode 'no_cond')."""
        return self.compute_features_and_accuracy(model, motionloader)[:2]

    def compute_features_and_accuracy(self, model, motionloader):
        """(activations, labels, accuracy): evaluate.py:21-34 and accuracy.py:4-14 from one forward per batch; accuracy is NaN for 'no_cond'."""
        with_labels = getattr(model, "cond_mode", None) != "no_cond"
        activations, labels = [], []
        confusion = torch.zeros(self.num_classes, self.num_classes, dtype=torch.long)
        with torch.no_grad():
            for batch in motionloader:
                feats, logits = self._forward(batch)
                activations.append(feats)
                if with_labels:
                    y = torch.as_tensor(batch["y"]).cpu().long().reshape(-1)
                    labels.append(y)
                    confusion.index_put_((y, logits.max(dim=1).indices.cpu()), torch.ones_like(y), accumulate=True)
        activations = torch.cat(activations, dim=0)
        if not with_labels:
            return activations, [], float("nan")
        return activations, torch.cat(labels, dim=0), (torch.trace(confusion) / torch.sum(confusion)).item()

    @staticmethod
    def calculate_activation_statistics(activations):
        """evaluate.py:36-41, in fp64 on the activations' device."""
        return calculate_activation_statistics(activations)

    def evaluate(self, model, loaders):
        """evaluate.py:43-84: {accuracy,diversity,multimodality,fid}_{gen,gt,gt2}. For cond_mode 'no_cond' accuracy and multimodality are NaN."""
        if self.seed is not None:
            np.random.seed(self.seed)
            torch.manual_seed(self.seed)
        no_cond = getattr(model, "cond_mode", None) == "no_cond"
        metrics, computedfeats = {}, {}
        for key, loader in loaders.items():
            feats, labels, metrics[f"accuracy_{key}"] = self.compute_features_and_accuracy(model, loader)
            computedfeats[key] = {"feats": feats, "labels": labels, "stats": self.calculate_activation_statistics(feats)}
            if no_cond:                                                                    # diversity.py:25-34, :64-65
                first = np.random.randint(0, feats.shape[0], 200)
                second = np.random.randint(0, feats.shape[0], 200)
                ret = (pair_distance_sum(feats.float(), first, second) / 200).item(), float("nan")
            else:
                ret = calculate_diversity_multimodality(feats, labels, self.num_classes)
            metrics[f"diversity_{key}"], metrics[f"multimodality_{key}"] = ret
        gtstats = computedfeats["gt"]["stats"]
        for key in computedfeats:
            metrics[f"fid_{key}"] = float(calculate_fid(gtstats, computedfeats[key]["stats"]))
        return metrics


class A2MLoader:
    """gru_eval.py:19-58 (NewDataloader): batches {"output", "output_xyz", "lengths", "y"} from an iterator of (motions, model_kwargs) - generated
    with diffusion.p_sample_loop (mode "gen") or the iterator's own motions ("gt") - with the joints from the project's device forward kinematics,
    model.rot2xyz(..., jointstype='smpl'). `batch_size` is the iterator's; num_samples = -1 takes everything."""

    def __init__(self, mode, model, diffusion, dataiterator, device, unconstrained=False, num_samples=-1, batch_size=None):
        assert mode in ["gen", "gt"]
        self.batches = []
        batch_size = batch_size or getattr(dataiterator, "batch_size")
        with torch.no_grad():
            for motions, model_kwargs in dataiterator:
                motions = motions.to(device)
                if num_samples != -1 and len(self.batches) * batch_size > num_samples:
                    continue
                batch = {}
                if mode == "gen":
                    batch["output"] = diffusion.p_sample_loop(model, motions.shape, clip_denoised=False, model_kwargs=model_kwargs)
                else:
                    batch["output"] = motions
                y = model_kwargs["y"]
                mask = y["mask"].reshape(motions.shape[0], -1).bool().to(device)
                batch["output_xyz"] = model.rot2xyz(x=batch["output"], mask=mask, pose_rep="rot6d", glob=True, translation=True, jointstype="smpl",
                                                    vertstrans=True, betas=None, beta=0, glob_rot=None, get_rotations_back=False)
                batch["lengths"] = y["lengths"].to(device)
                if "action" in y:
                    batch["y"] = y["action"].reshape(-1).long().cpu()
                self.batches.append(batch)
            rest = num_samples % batch_size if num_samples != -1 else 0
            if rest > 0 and self.batches:
                self.batches[-1] = {k: v[:rest] for k, v in self.batches[-1].items()}

    def __iter__(self):
        return iter(self.batches)


def array_loader(xyz, lengths, labels, batch_size, device):
    """Batches {"output_xyz" [n, 24, 3, T], "lengths", "y"} over arrays that are already joint positions."""
    xyz = torch.as_tensor(np.asarray(xyz, dtype=np.float32))
    lengths = torch.as_tensor(np.asarray(lengths)).long()
    labels = None if labels is None else torch.as_tensor(np.asarray(labels)).long().reshape(-1)
    out = []
    for lo in range(0, len(xyz), batch_size):
        b = {"output_xyz": xyz[lo:lo + batch_size].to(device), "lengths": lengths[lo:lo + batch_size].to(device)}
        if labels is not None:
            b["y"] = labels[lo:lo + batch_size]
        out.append(b)
    return out


def synthetic_xyz(n, seed, T=60, num_classes=12):
    """Seeded stand-ins for HumanAct12 joints: (xyz [n, 24, 3, T], lengths [n] in [T/2, T], labels [n]); a smooth walk per joint around a rest pose
    that is shifted by the label, so that the classes are not exchangeable."""
    rng = np.random.Generator(np.random.PCG64(seed))
    base = np.random.Generator(np.random.PCG64(4711))
    rest = base.standard_normal((1, 24, 3, 1))
    shift = 0.5 * base.standard_normal((num_classes, 24, 3, 1))
    y = rng.integers(0, num_classes, n)
    xyz = rest + shift[y] + 0.1 * np.cumsum(rng.standard_normal((n, 24, 3, T)), axis=3)
    return xyz.astype(np.float32), rng.integers(T // 2, T + 1, n).astype(np.int64), y.astype(np.int64)


def synthetic_loaders(num_samples, batch_size=64, seed=10, device="cuda:0"):
    """{"gen", "gt", "gt2"}: three seeded sets of `synthetic_xyz` (the first stands in for the generated motions)."""
    return {key: array_loader(*synthetic_xyz(num_samples, seed + i), batch_size, device) for i, key in enumerate(("gen", "gt", "gt2"))}


def evaluate_loaders(loaders, device, state_dict=None, model_path=None, num_seeds=1, cond_mode="action", unconstrained=False,
                     uncond_recogniser=None, log=print):
    """gru_eval.py:61-131 from the three loaders on: one A2MEvaluation.evaluate per seed (fixseed(seed) becomes the evaluation's own seeding), the
    reference's {"feats": {metric: [value per seed]}}; with `unconstrained` the generated joints' 15-joint cut (gru_eval.py:113-121) goes through
    `eval.unconstrained.evaluate_unconstrained_motions` against the same cut of the "gt" loader under `uncond_recogniser` (a six-block extractor),
    and its metrics are added with the suffix '_unconstrained'."""

    class _Model:
        pass

    _Model.cond_mode = cond_mode
    a2mmetrics = {}
    for seed in range(num_seeds):
        log(f"Evaluation number: {seed + 1}/{num_seeds}")
        a2mmetrics[seed] = A2MEvaluation(device, state_dict=state_dict, model_path=model_path, seed=seed).evaluate(_Model, loaders)
    metrics = {"feats": {key: [float(a2mmetrics[s][key]) for s in a2mmetrics] for key in a2mmetrics[0]}}
    if unconstrained:
        from .unconstrained import evaluate_unconstrained_motions
        cut = {k: torch.cat([b["output_xyz"][:, UNCONSTRAINED_JOINTS] for b in loaders[k]]) for k in ("gen", "gt")}
        n = min(len(cut["gen"]), len(cut["gt"]))
        um = evaluate_unconstrained_motions(cut["gen"], cut["gt"], uncond_recogniser, fast=True, kid_subset_size=min(1000, n))
        metrics["feats"].update({k + "_unconstrained": v for k, v in um.items()})
    return metrics


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--synthetic", action="store_true", help="seeded joint positions and a synthetic classifier checkpoint")
    ap.add_argument("--gen_xyz", help="FILE.npy [N, 24, 3, T]: joints of the generated motions")
    ap.add_argument("--gt_xyz", help="FILE.npy [N, 24, 3, T]: joints of the dataset's motions")
    ap.add_argument("--gt2_xyz", help="FILE.npy: a second draw of the dataset (default: --gt_xyz again)")
    ap.add_argument("--labels", help="FILE.npy [N] action labels, shared by the sets (omit for an unconditioned model)")
    ap.add_argument("--lengths", help="FILE.npy [N] valid frames per motion, shared by the sets (default: every frame)")
    ap.add_argument("--classifier", help="checkpoint of the GRU classifier (models.py:64: humanact12_gru.tar)")
    ap.add_argument("--unconstrained", action="store_true", help="add the unconstrained metric set over the 15-joint cut (gru_eval.py:105-121)")
    ap.add_argument("--uncond_recogniser", help="checkpoint of the six-block ST-GCN extractor for --unconstrained")
    ap.add_argument("--num_samples", type=int, default=64)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--num_seeds", type=int, default=1)
    ap.add_argument("--seed", type=int, default=10)
    ap.add_argument("--output_dir", default=".")
    args = ap.parse_args(argv)
    arrays = (args.gen_xyz, args.gt_xyz, args.classifier)
    if args.synthetic == any(arrays) or (any(arrays) and not all(arrays)):
        raise SystemExit("--synthetic, or --gen_xyz A.npy --gt_xyz B.npy --classifier CKPT [--gt2_xyz C.npy --labels Y.npy --lengths L.npy]")
    if not torch.cuda.is_available():
        raise SystemExit("the action2motion evaluation runs on an AMD GPU only (no CPU fallback)")
    dev = "cuda:0"
    recogniser, state_dict, cond_mode = None, None, "action"
    if args.synthetic:
        from .. import synth
        state_dict = synth.make_gru_state_dict(seed=0)
        loaders = synthetic_loaders(args.num_samples, args.batch_size, args.seed, dev)
        if args.unconstrained:
            from .unconstrained import synthetic_recogniser
            recogniser = synthetic_recogniser(torch.device(dev))
    else:
        sets = {"gen": np.load(args.gen_xyz), "gt": np.load(args.gt_xyz)}
        sets["gt2"] = np.load(args.gt2_xyz) if args.gt2_xyz else sets["gt"]
        labels = np.load(args.labels) if args.labels else None
        cond_mode = "action" if args.labels else "no_cond"
        loaders = {}
        for k, a in sets.items():
            ln = np.load(args.lengths) if args.lengths else np.full(len(a), a.shape[-1])
            loaders[k] = array_loader(a, ln[:len(a)], None if labels is None else labels[:len(a)], args.batch_size, dev)
        if args.unconstrained:
            if not args.uncond_recogniser:
                raise SystemExit("--unconstrained needs --uncond_recogniser CKPT")
            from .unconstrained import initialize_model
            recogniser = initialize_model(torch.device(dev), args.uncond_recogniser)
    metrics = evaluate_loaders(loaders, dev, state_dict=state_dict, model_path=args.classifier, num_seeds=args.num_seeds, cond_mode=cond_mode,
                               unconstrained=args.unconstrained, uncond_recogniser=recogniser)
    for k, v in metrics["feats"].items():
        print(f"{k:32s} {v}")
    os.makedirs(args.output_dir, exist_ok=True)
    path = os.path.join(args.output_dir, "metrics.npy")
    np.save(path, metrics)
    print(f"saved the metrics to [{os.path.abspath(path)}]")
    return metrics


if __name__ == "__main__":
    main()
