"""The HumanML3D / KIT text-to-motion evaluation on the device - counterpart of the reference's `eval/eval_humanml.py`
(evaluate_matching_score :19-69, evaluate_fid :72-95, evaluate_diversity :98-106, evaluate_multimodality :109-128, get_metric_statistics :131-135,
evaluation :138-226) over `regennet_amd.eval.t2m.EvaluatorMDMWrapper`.

The reference pulls every embedding to the host, builds each batch's distance matrix with numpy (the cancelling -2ab + a^2 + b^2 form), sorts it and
calls scipy for the Frechet distance. Here the embeddings stay on the device between the stages: R-precision and matching score come from
`rgn_t2m_match` (direct differences; rank of the true pair), FID from `eval/fid.py`, diversity and multimodality from `eval/metrics.pair_distance_sum`
on index pairs drawn exactly as the reference draws them (`np.random.choice(..., replace=False)` twice). The log lines and the returned `mean_dict`
are the reference's. A batch is the reference's 7-tuple (word_embeddings, pos_one_hots, caption, sent_lens, motions, m_lens, tokens).

    python -m regennet_amd.eval.humanml --synthetic --num_samples 64
    python -m regennet_amd.eval.humanml --gen_motions A.npy --gt_motions B.npy --lengths L.npy --word_embs W.npy --pos_ohot P.npy --cap_lens C.npy \\
        --evaluator t2m/text_mot_match/model/finest.tar

Tokenising, the GloVe vectors and CLIP stay the caller's (`CMDM.encode_text`): batches carry `word_embs`, `pos_ohot`, `cap_lens` and
`y['text_features']`.
"""
import os
from collections import OrderedDict
from datetime import datetime

import numpy as np
import torch

from .. import _lib
from .fid import calculate_activation_statistics, calculate_frechet_distance
from .metrics import pair_distance_sum

BATCH_SIZE = 32           # eval_humanml.py:232: "This must be 32! Don't change it! otherwise it will cause a bug in R precision calc!"
# eval_humanml.py:244-267: (num_samples_limit, run_mm, mm_num_samples, mm_num_repeats, mm_num_times, diversity_times, replication_times)
EVAL_MODES = {"debug": (1000, False, 0, 0, 0, 300, 5), "wo_mm": (1000, False, 0, 0, 0, 300, 20), "mm_short": (1000, True, 100, 30, 10, 300, 5)}


def _rng(seed):
    return np.random if seed is None else (seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed))


def top_k_from_rank(rank, top_k=3):
    """calculate_top_k (metrics.py:22-34) from the rank of the true pair: hit within the first k <=> rank < k. bool [N, top_k] on rank's device."""
    return rank[:, None] < torch.arange(1, top_k + 1, device=rank.device)[None, :]


def renormalise(x, mean, std, mean_for_eval, std_for_eval):
    """comp_v6_model_dataset.py:246-250: the generator's normalisation undone, the evaluator's applied; [..., T, D] on x's device"""
    dev = x.device
    mean, std, me, se = (torch.as_tensor(np.asarray(v), dtype=torch.float32, device=dev) for v in (mean, std, mean_for_eval, std_for_eval))
    return (x * std + mean - me) / se


def evaluate_matching_score(eval_wrapper, motion_loaders, file, ranks=None):
    """eval_humanml.py:19-69. activation_dict holds device tensors; `ranks`, a dict, receives each loader's per-row ranks (int32, device)."""
    match_score_dict, R_precision_dict, activation_dict = OrderedDict({}), OrderedDict({}), OrderedDict({})
    print("========== Evaluating Matching Score ==========")
    for motion_loader_name, motion_loader in motion_loaders.items():
        all_motion_embeddings, all_rank, all_size, matching_score_sum = [], [], 0, 0.0
        with torch.no_grad():
            for idx, batch in enumerate(motion_loader):
                word_embeddings, pos_one_hots, _, sent_lens, motions, m_lens, _ = batch
                text_embeddings, motion_embeddings = eval_wrapper.get_co_embeddings(word_embs=word_embeddings, pos_ohot=pos_one_hots, cap_lens=sent_lens,
                                                                                    motions=motions, m_lens=m_lens)
                diag, rank = _lib.t2m_match(text_embeddings, motion_embeddings, group=BATCH_SIZE)
                matching_score_sum = matching_score_sum + diag.double().sum()
                all_rank.append(rank)
                all_size += text_embeddings.shape[0]
                all_motion_embeddings.append(motion_embeddings)
            all_motion_embeddings = torch.cat(all_motion_embeddings, dim=0)
            all_rank = torch.cat(all_rank)
            matching_score = np.float64(float(matching_score_sum) / all_size)
            R_precision = top_k_from_rank(all_rank, 3).sum(dim=0).cpu().numpy() / all_size
            match_score_dict[motion_loader_name] = matching_score
            R_precision_dict[motion_loader_name] = R_precision
            activation_dict[motion_loader_name] = all_motion_embeddings
            if ranks is not None:
                ranks[motion_loader_name] = all_rank
        print(f"---> [{motion_loader_name}] Matching Score: {matching_score:.4f}")
        print(f"---> [{motion_loader_name}] Matching Score: {matching_score:.4f}", file=file, flush=True)
        line = f"---> [{motion_loader_name}] R_precision: "
        for i in range(len(R_precision)):
            line += "(top %d): %.4f " % (i + 1, R_precision[i])
        print(line)
        print(line, file=file, flush=True)
    return match_score_dict, R_precision_dict, activation_dict


def evaluate_fid(eval_wrapper, groundtruth_loader, activation_dict, file):
    """eval_humanml.py:72-95"""
    eval_dict = OrderedDict({})
    gt_motion_embeddings = []
    print("========== Evaluating FID ==========")
    with torch.no_grad():
        for idx, batch in enumerate(groundtruth_loader):
            _, _, _, sent_lens, motions, m_lens, _ = batch
            gt_motion_embeddings.append(eval_wrapper.get_motion_embeddings(motions=motions, m_lens=m_lens))
    gt_mu, gt_cov = calculate_activation_statistics(torch.cat(gt_motion_embeddings, dim=0))
    for model_name, motion_embeddings in activation_dict.items():
        mu, cov = calculate_activation_statistics(motion_embeddings)
        fid = np.float64(float(calculate_frechet_distance(gt_mu, gt_cov, mu, cov)))
        print(f"---> [{model_name}] FID: {fid:.4f}")
        print(f"---> [{model_name}] FID: {fid:.4f}", file=file, flush=True)
        eval_dict[model_name] = fid
    return eval_dict


def calculate_diversity(activation, diversity_times, seed=None):
    """metrics.py:73-81 on a device tensor [N, D]"""
    assert activation.dim() == 2 and activation.shape[0] > diversity_times
    rng = _rng(seed)
    first_indices = rng.choice(activation.shape[0], diversity_times, replace=False)
    second_indices = rng.choice(activation.shape[0], diversity_times, replace=False)
    return np.float64(float(pair_distance_sum(activation, first_indices, second_indices)) / diversity_times)


def calculate_multimodality(activation, multimodality_times, seed=None):
    """metrics.py:84-92 on a device tensor [texts, repeats, D]"""
    assert activation.dim() == 3 and activation.shape[1] > multimodality_times
    rng = _rng(seed)
    n, R, D = activation.shape
    first_dices = rng.choice(R, multimodality_times, replace=False)
    second_dices = rng.choice(R, multimodality_times, replace=False)
    base = np.arange(n)[:, None] * R
    total = pair_distance_sum(activation.reshape(n * R, D), (base + first_dices[None, :]).ravel(), (base + second_dices[None, :]).ravel())
    return np.float64(float(total) / (n * multimodality_times))


def evaluate_diversity(activation_dict, file, diversity_times, seed=None):
    """eval_humanml.py:98-106"""
    eval_dict = OrderedDict({})
    print("========== Evaluating Diversity ==========")
    for model_name, motion_embeddings in activation_dict.items():
        diversity = calculate_diversity(motion_embeddings, diversity_times, seed)
        eval_dict[model_name] = diversity
        print(f"---> [{model_name}] Diversity: {diversity:.4f}")
        print(f"---> [{model_name}] Diversity: {diversity:.4f}", file=file, flush=True)
    return eval_dict


def evaluate_multimodality(eval_wrapper, mm_motion_loaders, file, mm_num_times, seed=None):
    """eval_humanml.py:109-128; an mm batch is (motions [1, repeats, T, D], m_lens [1, repeats])"""
    eval_dict = OrderedDict({})
    print("========== Evaluating MultiModality ==========")
    for model_name, mm_motion_loader in mm_motion_loaders.items():
        mm_motion_embeddings = []
        with torch.no_grad():
            for idx, batch in enumerate(mm_motion_loader):
                motions, m_lens = batch
                mm_motion_embeddings.append(eval_wrapper.get_motion_embeddings(motions[0], m_lens[0]).unsqueeze(0))
        if len(mm_motion_embeddings) == 0:
            multimodality = 0
        else:
            multimodality = calculate_multimodality(torch.cat(mm_motion_embeddings, dim=0), mm_num_times, seed)
        print(f"---> [{model_name}] Multimodality: {multimodality:.4f}")
        print(f"---> [{model_name}] Multimodality: {multimodality:.4f}", file=file, flush=True)
        eval_dict[model_name] = multimodality
    return eval_dict


def get_metric_statistics(values, replication_times):
    """eval_humanml.py:131-135"""
    mean = np.mean(values, axis=0)
    std = np.std(values, axis=0)
    conf_interval = 1.96 * std / np.sqrt(replication_times)
    return mean, conf_interval


def evaluation(eval_wrapper, gt_loader, eval_motion_loaders, log_file, replication_times, diversity_times, mm_num_times, run_mm=False, seed=None,
               ranks=None):
    """eval_humanml.py:138-226. `seed` makes the index draws of diversity and multimodality those of `np.random.seed(seed)` in front of the reference's
    call; `ranks`, a list, receives one {loader: per-row ranks} dict per replication."""
    rng = None if seed is None else np.random.RandomState(seed)
    with open(log_file, "w") as f:
        all_metrics = OrderedDict({"Matching Score": OrderedDict({}), "R_precision": OrderedDict({}), "FID": OrderedDict({}),
                                   "Diversity": OrderedDict({}), "MultiModality": OrderedDict({})})
        for replication in range(replication_times):
            motion_loaders, mm_motion_loaders = {}, {}
            motion_loaders["ground truth"] = gt_loader
            for motion_loader_name, motion_loader_getter in eval_motion_loaders.items():
                motion_loader, mm_motion_loader = motion_loader_getter()
                motion_loaders[motion_loader_name] = motion_loader
                mm_motion_loaders[motion_loader_name] = mm_motion_loader

            def stamp():
                print(f"Time: {datetime.now()}")
                print(f"Time: {datetime.now()}", file=f, flush=True)

            print(f"==================== Replication {replication} ====================")
            print(f"==================== Replication {replication} ====================", file=f, flush=True)
            stamp()
            rk = {}
            mat_score_dict, R_precision_dict, acti_dict = evaluate_matching_score(eval_wrapper, motion_loaders, f, ranks=rk)
            if ranks is not None:
                ranks.append(rk)
            stamp()
            fid_score_dict = evaluate_fid(eval_wrapper, gt_loader, acti_dict, f)
            stamp()
            div_score_dict = evaluate_diversity(acti_dict, f, diversity_times, rng)
            mm_score_dict = {}
            if run_mm:
                stamp()
                mm_score_dict = evaluate_multimodality(eval_wrapper, mm_motion_loaders, f, mm_num_times, rng)
            print("!!! DONE !!!")
            print("!!! DONE !!!", file=f, flush=True)
            for name, d in (("Matching Score", mat_score_dict), ("R_precision", R_precision_dict), ("FID", fid_score_dict), ("Diversity", div_score_dict),
                            ("MultiModality", mm_score_dict)):
                for key, item in d.items():
                    all_metrics[name].setdefault(key, []).append(item)

        mean_dict = {}
        for metric_name, metric_dict in all_metrics.items():
            print("========== %s Summary ==========" % metric_name)
            print("========== %s Summary ==========" % metric_name, file=f, flush=True)
            for model_name, values in metric_dict.items():
                mean, conf_interval = get_metric_statistics(np.array(values), replication_times)
                mean_dict[metric_name + "_" + model_name] = mean
                if isinstance(mean, np.float64) or isinstance(mean, np.float32):
                    print(f"---> [{model_name}] Mean: {mean:.4f} CInterval: {conf_interval:.4f}")
                    print(f"---> [{model_name}] Mean: {mean:.4f} CInterval: {conf_interval:.4f}", file=f, flush=True)
                elif isinstance(mean, np.ndarray):
                    line = f"---> [{model_name}]"
                    for i in range(len(mean)):
                        line += "(top %d) Mean: %.4f CInt: %.4f;" % (i + 1, mean[i], conf_interval[i])
                    print(line)
                    print(line, file=f, flush=True)
        return mean_dict


def array_loader(word_embs, pos_ohot, cap_lens, motions, m_lens, batch_size=BATCH_SIZE, device="cuda:0"):
    """Recorded arrays as the reference's batches: a list of 7-tuples of device tensors (captions and tokens None)."""
    t = [torch.as_tensor(np.asarray(a)).to(device) for a in (word_embs, pos_ohot, cap_lens, motions, m_lens)]
    n = len(t[3])
    return [(t[0][i:i + batch_size].float(), t[1][i:i + batch_size].float(), None, t[2][i:i + batch_size].long(), t[3][i:i + batch_size].float(),
             t[4][i:i + batch_size].long(), None) for i in range(0, n, batch_size)]


def mm_array_loader(motions, m_lens, repeats, device="cuda:0"):
    """[texts * repeats, T, D] recorded motions (a text's repeats adjacent) as the multimodality loader's batches"""
    m, ln = torch.as_tensor(np.asarray(motions)).float().to(device), torch.as_tensor(np.asarray(m_lens)).long().to(device)
    return [(m[i:i + repeats][None], ln[i:i + repeats][None]) for i in range(0, len(m) - repeats + 1, repeats)]


class GeneratedT2MLoader:
    """CompMDMGeneratedDataset (comp_v6_model_dataset.py:146-262) without the host round trip: samples every batch with `p_sample_loop`
    (clip_denoised=False), the batches drawn for multimodality `mm_num_repeats` times, and renormalises (x std + mean - mean_for_eval) / std_for_eval
    on the device. `batches` is a list of dicts {'shape' (bs, njoints, nfeats, T) or 'motion', 'y': model kwargs with 'lengths' and 'text_features'
    (or 'text' with model.encode_text assigned), 'word_embs', 'pos_ohot', 'cap_lens'}. The sampler's limits are the engine's: it refuses what
    rgn_create refuses. `motion_loader()` / `mm_loader()` give what `evaluation` iterates."""

    def __init__(self, model, diffusion, batches, mm_num_samples, mm_num_repeats, max_motion_length, num_samples_limit, scale=1.0, mean=0.0, std=1.0,
                 mean_for_eval=0.0, std_for_eval=1.0, seed=None):
        batches = list(batches)
        bs = len(batches[0]["cap_lens"])
        assert mm_num_samples < sum(len(b["cap_lens"]) for b in batches)
        real_num_batches = len(batches) if num_samples_limit is None else min(len(batches), num_samples_limit // bs + 1)
        mm_idxs = np.sort(_rng(seed).choice(real_num_batches, mm_num_samples // bs + 1, replace=False)) if mm_num_samples > 0 else []
        self.max_motion_length = max_motion_length
        self.batches, self.mm_batches = [], []
        dev = next(model.parameters()).device
        model.eval()
        with torch.no_grad():
            done = 0
            for i, b in enumerate(batches[:real_num_batches]):
                if num_samples_limit is not None and done >= num_samples_limit:
                    break
                y = dict(b["y"])
                if scale != 1.0:
                    y["scale"] = torch.ones(bs, device=dev) * scale
                shape = tuple(b["shape"]) if "shape" in b else tuple(b["motion"].shape)
                lengths = torch.as_tensor(y["lengths"]).to(dev).long()
                is_mm = i in mm_idxs
                reps = []
                for t in range(mm_num_repeats if is_mm else 1):
                    sample = diffusion.p_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=0, init_image=None,
                                                     progress=False, dump_steps=None, noise=None, const_noise=False)
                    motion = renormalise(sample.reshape(shape[0], shape[1] * shape[2], shape[3]).permute(0, 2, 1), mean, std, mean_for_eval, std_for_eval)
                    reps.append(motion)
                    if t == 0:
                        self.batches.append((torch.as_tensor(b["word_embs"]).to(dev).float(), torch.as_tensor(b["pos_ohot"]).to(dev).float(),
                                             y.get("text"), torch.as_tensor(b["cap_lens"]).to(dev).long(), motion, lengths, None))
                        done += bs
                if is_mm:
                    stack = torch.stack(reps, dim=1)                 # [bs, repeats, T, D]
                    self.mm_batches += [(stack[k][None], lengths[k].repeat(len(reps))[None]) for k in range(bs)]

    def motion_loader(self):
        return self.batches

    def mm_loader(self):
        return self.mm_batches

    def __call__(self):
        return self.batches, self.mm_batches


def synthetic_sets(num_samples, seed=10, T=64, Lw=12):
    """Seeded stand-ins: (evaluator state dicts, ground-truth inputs dict, generated motions) at the HumanML3D geometry"""
    from .. import synth
    sds = synth.make_t2m_state_dicts(seed=seed)
    gt = synth.make_t2m_inputs(num_samples, T, Lw, seed=seed + 1)
    gen = (0.7 * gt["motions"] + 0.7 * synth.make_t2m_inputs(num_samples, T, Lw, seed=seed + 2)["motions"]).astype(np.float32)
    return sds, gt, gen


def main(argv=None):
    import argparse

    from .t2m import EvaluatorMDMWrapper
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--synthetic", action="store_true", help="seeded motions, texts and a synthetic evaluator checkpoint")
    ap.add_argument("--gen_motions", help="FILE.npy [N, T, dim_pose]: generated motions, in the evaluator's normalisation")
    ap.add_argument("--gt_motions", help="FILE.npy [N, T, dim_pose]: the dataset's motions")
    ap.add_argument("--lengths", help="FILE.npy [N] valid frames per motion, shared by the sets")
    ap.add_argument("--word_embs", help="FILE.npy [N, Lw, 300]")
    ap.add_argument("--pos_ohot", help="FILE.npy [N, Lw, 15]")
    ap.add_argument("--cap_lens", help="FILE.npy [N]")
    ap.add_argument("--mm_motions", help="FILE.npy [texts * mm_repeats, T, dim_pose]: repeats of a text adjacent (with --mm_lengths, --mm_repeats)")
    ap.add_argument("--mm_lengths")
    ap.add_argument("--mm_repeats", type=int, default=30)
    ap.add_argument("--evaluator", help="the evaluator's checkpoint (finest.tar)")
    ap.add_argument("--dataset", default="humanml", choices=["humanml", "kit"])
    ap.add_argument("--eval_mode", default="debug", choices=sorted(EVAL_MODES))
    ap.add_argument("--replication_times", type=int, help="override the mode's count")
    ap.add_argument("--num_samples", type=int, default=64)
    ap.add_argument("--batch_size", type=int, default=BATCH_SIZE)
    ap.add_argument("--seed", type=int, default=10)
    ap.add_argument("--output_dir", default=".")
    args = ap.parse_args(argv)
    if args.batch_size != BATCH_SIZE:
        raise SystemExit("--batch_size must be 32: R-precision is defined on groups of 32 (eval_humanml.py:232)")
    arrays = (args.gen_motions, args.gt_motions, args.lengths, args.word_embs, args.pos_ohot, args.cap_lens, args.evaluator)
    if args.synthetic == any(arrays) or (any(arrays) and not all(arrays)):
        raise SystemExit("--synthetic, or --gen_motions A.npy --gt_motions B.npy --lengths L.npy --word_embs W.npy --pos_ohot P.npy --cap_lens C.npy "
                         "--evaluator finest.tar")
    if not torch.cuda.is_available():
        raise SystemExit("the text-to-motion evaluation runs on an AMD GPU only (no CPU fallback)")
    dev = "cuda:0"
    num_samples_limit, run_mm, _, _, mm_num_times, diversity_times, replication_times = EVAL_MODES[args.eval_mode]
    if args.synthetic:
        sds, gt, gen = synthetic_sets(args.num_samples, args.seed)
        wrapper = EvaluatorMDMWrapper(args.dataset, dev, state_dicts=sds)
        texts = (gt["word_embs"], gt["pos_ohot"], gt["cap_lens"])
        gt_motions, lengths = gt["motions"], gt["m_lens"]
        replication_times = 1
        mm = mm_array_loader(gen[:16], lengths[:16], 4, dev)
        run_mm, mm_num_times = True, 2
    else:
        wrapper = EvaluatorMDMWrapper(args.dataset, dev, checkpoint=args.evaluator)
        texts = tuple(np.load(p) for p in (args.word_embs, args.pos_ohot, args.cap_lens))
        gen, gt_motions, lengths = np.load(args.gen_motions), np.load(args.gt_motions), np.load(args.lengths)
        mm = mm_array_loader(np.load(args.mm_motions), np.load(args.mm_lengths), args.mm_repeats, dev) if args.mm_motions else []
        run_mm = run_mm and bool(mm)
    if args.replication_times:
        replication_times = args.replication_times
    n = min(len(gen), len(gt_motions), num_samples_limit)
    n -= n % BATCH_SIZE                                              # whole groups of 32, as the reference's drop_last loaders give
    diversity_times = min(diversity_times, n - 1)
    gt_loader = array_loader(*(a[:n] for a in texts), gt_motions[:n], lengths[:n], BATCH_SIZE, dev)
    gen_loader = array_loader(*(a[:n] for a in texts), gen[:n], lengths[:n], BATCH_SIZE, dev)
    os.makedirs(args.output_dir, exist_ok=True)
    log_file = os.path.join(args.output_dir, f"eval_humanml_{args.eval_mode}.log")
    print(f"Will save to log file [{log_file}]")
    mean_dict = evaluation(wrapper, gt_loader, {"vald": lambda: (gen_loader, mm)}, log_file, replication_times, diversity_times, mm_num_times,
                           run_mm=run_mm, seed=args.seed)
    path = os.path.join(args.output_dir, "metrics.npy")
    np.save(path, mean_dict)
    print(f"saved the metrics to [{os.path.abspath(path)}]")
    return mean_dict


if __name__ == "__main__":
    main()
