"""fp64 restatement of the text-to-motion evaluator (the reference's data_loaders/humanml/networks/modules.py: MovementConvEncoder :79-98,
TextEncoderBiGRUCo :311-350, MotionEncoderBiGRUCo :353-386) and of the matching part of data_loaders/humanml/utils/metrics.py, written out in numpy - the
yardstick of tests/test_t2m_{cpu,gpu}.py and of tests/golden/make_golden_t2m.py.

`mutant` names ONE deliberate error. Operand mutants round one operand to bf16 before every product it enters: "W_hh", "W_ih", "h" (the recurrent
state), "x" (the recurrence's input rows, i.e. input_emb's output), "conv" (the convolutions' weights). Structural mutants: "rev_start" (the reverse
direction starts at the last frame of the padded array instead of frame L - 1), "hidden0" (hidden[0] starts both directions), "bhn_outside"
(n = tanh(gi_n + r W_hn h + b_hn): b_hn outside r). The parity bound has to tell each from the right arithmetic."""
import os

import numpy as np

from tests.gru_ref import bf16_round, bound  # noqa: F401  (the project's one parity rule)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

REAL = dict(dim_pose=263, movement_hidden=512, movement_latent=512, motion_hidden=1024, dim_word=300, dim_pos_ohot=15, text_hidden=512, coemb=512)
SMALL = dict(dim_pose=23, movement_hidden=64, movement_latent=64, motion_hidden=64, dim_word=12, dim_pos_ohot=5, text_hidden=64, coemb=64)
# name: (geometry, N, T, Lw, weight scale, scale of the heads' last Linear)
CASES = {
    "t2m": (REAL, 33, 196, 22, 1.0, 1.0),
    "kit": (dict(REAL, dim_pose=251), 17, 196, 22, 1.0, 1.0),
    "small": (SMALL, 17, 20, 6, 1.0, 1.5),
    "odd_T": (SMALL, 5, 7, 3, 1.0, 1.5),
    "one": (REAL, 1, 4, 1, 1.0, 1.0),
    "hot": (REAL, 16, 64, 10, 3.0, 1.0),
}
CASE_SEEDS = {name: 300 + i for i, name in enumerate(CASES)}
OUTPUTS = ("movements", "motion_emb", "text_emb")
BF16_MUTANTS = ("W_hh", "W_ih", "h", "x", "conv")
STRUCTURAL_MUTANTS = ("rev_start", "hidden0", "bhn_outside")

# the metric case: EVAL_N generated and EVAL_N ground-truth motions with one set of texts, at the real geometry (weights of case "t2m")
EVAL_N, EVAL_T, EVAL_LW, EVAL_SEED = 64, 64, 12, 400
EVAL_POOL = 192
# rows of the pool, in two groups of 32, chosen so that the fp64 embeddings alone satisfy the margin condition of make_golden_t2m.record_eval in every
# row of both loaders
EVAL_ROWS = [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 13, 15, 17, 18, 20, 21, 23, 24, 25, 26, 27, 30, 31, 32, 33, 36, 37, 39, 40, 41, 42,
             7, 12, 14, 16, 19, 22, 28, 29, 34, 35, 38, 44, 46, 48, 49, 50, 51, 52, 53, 55, 56, 58, 60, 62, 63, 66, 67, 68, 69, 71, 73, 74]
EVAL_DIVERSITY_TIMES, EVAL_MM_TIMES, EVAL_MM_TEXTS, EVAL_MM_REPEATS = 30, 3, 4, 6
# the matching cases: (N, D, seed, noise); text = motion + noise. N = 70 leaves a short last group. The seeds are ones at which the fp64 distances
# alone satisfy the margin condition of make_golden_t2m.record_match in every row.
MATCH_CASES = {"d512": (70, 512, 1053, 9.0), "d4": (70, 4, 502, 0.6)}


def geometry(name):
    return dict(CASES[name][0], unit_length=4)


def case_inputs(name):
    """(state dicts {'movement_encoder', 'text_encoder', 'motion_encoder'}, inputs dict) of a case, regenerated from its seed."""
    from regennet_amd import synth
    geo, N, T, Lw, scale, out_scale = CASES[name]
    seed = CASE_SEEDS[name]
    sds = synth.make_t2m_state_dicts(seed=seed, scale=scale, out_scale=out_scale, **geo)
    inp = synth.make_t2m_inputs(N, T, Lw, seed=seed + 1000, lengths="mixed", dim_pose=geo["dim_pose"], dim_word=geo["dim_word"],
                                dim_pos_ohot=geo["dim_pos_ohot"])
    return sds, inp


def eval_pool():
    """(state dicts of case "t2m", pool of ground-truth inputs, pool of generated motions): EVAL_POOL rows, of which the metric case takes EVAL_ROWS"""
    from regennet_amd import synth
    geo = CASES["t2m"][0]
    sds = synth.make_t2m_state_dicts(seed=CASE_SEEDS["t2m"], **geo)
    gt = synth.make_t2m_inputs(EVAL_POOL, EVAL_T, EVAL_LW, seed=EVAL_SEED, lengths="mixed")
    gen = synth.make_t2m_inputs(EVAL_POOL, EVAL_T, EVAL_LW, seed=EVAL_SEED + 1, lengths="mixed")["motions"]
    return sds, gt, (0.7 * gt["motions"] + 0.7 * gen).astype(np.float32)


def eval_inputs():
    """The metric case: (state dicts of case "t2m", ground-truth inputs, generated motions [EVAL_N, EVAL_T, 263] with the same lengths and texts)."""
    sds, gt, gen = eval_pool()
    rows = np.asarray(EVAL_ROWS)
    return sds, {k: v[rows] for k, v in gt.items()}, gen[rows]


def eval_order(cap_lens, m_lens):
    """(order, aligned): the rows of the metric case as its loaders serve them - text rows sorted by length inside each batch of 32, as the reference's
    collate leaves them (pack_padded_sequence demands it) - and as the wrapper returns them, each batch sorted by motion length, longest first
    (evaluator_wrapper.py:160). Both as indices into the input rows."""
    order = np.concatenate([b0 + np.argsort(-cap_lens[b0:b0 + 32], kind="stable") for b0 in range(0, len(cap_lens), 32)])
    aligned = np.concatenate([order[b0:b0 + 32][np.argsort(m_lens[order[b0:b0 + 32]].tolist())[::-1]] for b0 in range(0, len(order), 32)])
    return order, aligned


def eval_mm(gen, m_lens):
    """the multimodality loader's batches: EVAL_MM_TEXTS x (motions [EVAL_MM_REPEATS, T, 263], lengths [EVAL_MM_REPEATS])"""
    R = EVAL_MM_REPEATS
    return [(gen[i * R:(i + 1) * R], np.asarray(m_lens[i * R:(i + 1) * R])) for i in range(EVAL_MM_TEXTS)]


EVAL_METRICS = ("Matching Score_ground truth", "Matching Score_vald", "Diversity_ground truth", "Diversity_vald", "MultiModality_vald")


def eval_metrics64(replication_times=2):
    """fp64 restatement of what eval_humanml.evaluation returns for the metric case (its mean_dict without R-precision and FID): embeddings from the
    fp64 encoders, distances by direct differences, rows in the order the wrapper returns them, and the index pairs of diversity and multimodality
    drawn as the reference draws them after np.random.seed(EVAL_SEED): per replication, diversity of 'ground truth' then 'vald'
    (np.random.choice(n, times, replace=False) twice each), then multimodality."""
    sds, gt, gen = eval_inputs()
    _, aligned = eval_order(gt["cap_lens"], gt["m_lens"])
    t64 = text_side(sds, gt["word_embs"], gt["pos_ohot"], gt["cap_lens"])
    emb = {"ground truth": motion_side(sds, gt["motions"], gt["m_lens"])[1], "vald": motion_side(sds, gen, gt["m_lens"])[1]}
    mm = []
    for motions, lens in eval_mm(gen, gt["m_lens"]):
        idx = np.argsort(lens.tolist())[::-1].copy()          # get_motion_embeddings sorts each multimodality batch too
        mm.append(motion_side(sds, motions, lens)[1][idx])
    mm = np.stack(mm)
    out = {k: [] for k in EVAL_METRICS}
    rng = np.random.RandomState(EVAL_SEED)
    for _ in range(replication_times):
        for name, e in emb.items():
            out["Matching Score_" + name].append(np.sqrt(((t64 - e) ** 2).sum(1)).mean())
        for name, e in emb.items():
            act = e[aligned]
            first, second = rng.choice(len(act), EVAL_DIVERSITY_TIMES, replace=False), rng.choice(len(act), EVAL_DIVERSITY_TIMES, replace=False)
            out["Diversity_" + name].append(np.sqrt(((act[first] - act[second]) ** 2).sum(1)).mean())
        first, second = rng.choice(mm.shape[1], EVAL_MM_TIMES, replace=False), rng.choice(mm.shape[1], EVAL_MM_TIMES, replace=False)
        out["MultiModality_vald"].append(np.sqrt(((mm[:, first] - mm[:, second]) ** 2).sum(2)).mean())
    return {k: float(np.mean(v)) for k, v in out.items()}


def movement_rows(N):
    """the rows whose movements a fixture stores (lengths T, 40, 4, 41 and the last row)"""
    return sorted(set(r for r in (0, 1, 2, 3, N - 1) if r < N))


def match_inputs(name):
    """(text, motion) fp32 [N, D]: motion rows normal, text = motion + noise sized so that about half the true pairs rank first in their group."""
    N, D, seed, noise = MATCH_CASES[name]
    rng = np.random.Generator(np.random.PCG64(seed))
    motion = rng.standard_normal((N, D)).astype(np.float32)
    text = (motion + noise * rng.standard_normal((N, D))).astype(np.float32)
    return text, motion


def _f64(sd):
    return {k: np.asarray(v, np.float64) for k, v in sd.items()}


def _lrelu(v):
    return np.where(v >= 0, v, 0.2 * v)


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def _conv(x, W, b):
    """Conv1d(k 4, s 2, p 1) over frames: x [N, T, C], W [O, C, 4] -> [N, (T - 2) // 2 + 1, O]"""
    N, T, C = x.shape
    To = (T - 2) // 2 + 1
    xp = np.zeros((N, T + 2, C))
    xp[:, 1:T + 1] = x
    out = np.zeros((N, To, W.shape[0])) + b
    for tap in range(4):
        out += xp[:, tap:tap + 2 * To:2] @ W[:, :, tap].T
    return out


def movements(sd, x, mutant=None):
    """MovementConvEncoder on x [N, T, dim_pose - 4] -> [N, T2, Dm], every frame."""
    sd = _f64(sd)
    rd = (lambda a: bf16_round(a)) if mutant == "conv" else (lambda a: a)
    h = _lrelu(_conv(np.asarray(x, np.float64), rd(sd["main.0.weight"]), sd["main.0.bias"]))
    h = _lrelu(_conv(h, rd(sd["main.3.weight"]), sd["main.3.bias"]))
    return h @ sd["out_net.weight"].T + sd["out_net.bias"]


def bigru_head(sd, emb, lens, mutant=None):
    """gru + output_net of either encoder: emb [N, L, H] (input_emb's output), lens [N] in [1, L] -> [N, D]. Packed-sequence semantics: the forward
    direction runs t = 0 .. len - 1 from hidden[0], the reverse one t = len - 1 .. 0 from hidden[1]."""
    sd = _f64(sd)
    N, Lmax, H = emb.shape
    lens = np.asarray(lens)
    rd = (lambda name, a: bf16_round(a) if mutant == name else a)
    x = rd("x", emb)
    last = []
    for d, sfx in enumerate(("_l0", "_l0_reverse")):
        Wi, Wh = rd("W_ih", sd["gru.weight_ih" + sfx]), rd("W_hh", sd["gru.weight_hh" + sfx])
        bi, bh = sd["gru.bias_ih" + sfx], sd["gru.bias_hh" + sfx]
        h = np.repeat(sd["hidden"][0 if mutant == "hidden0" else d], N, axis=0)
        steps = Lmax if (d == 1 and mutant == "rev_start") else int(lens.max())
        for s in range(steps):
            if d == 0:
                t, live = np.full(N, s), s < lens
            elif mutant == "rev_start":
                t, live = np.full(N, Lmax - 1 - s), np.ones(N, bool)
            else:
                t, live = np.maximum(lens - 1 - s, 0), s < lens
            gi = x[np.arange(N), t] @ Wi.T + bi
            gh = rd("h", h) @ Wh.T
            r = _sigmoid(gi[:, :H] + gh[:, :H] + bh[:H])
            z = _sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H] + bh[H:2 * H])
            if mutant == "bhn_outside":
                n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:] + bh[2 * H:])
            else:
                n = np.tanh(gi[:, 2 * H:] + r * (gh[:, 2 * H:] + bh[2 * H:]))
            hn = (1.0 - z) * n + z * h
            h = np.where(live[:, None], hn, h)
        last.append(h)
    y = np.concatenate(last, axis=1) @ sd["output_net.0.weight"].T + sd["output_net.0.bias"]
    mu = y.mean(axis=1, keepdims=True)
    var = ((y - mu) ** 2).mean(axis=1, keepdims=True)
    y = _lrelu((y - mu) / np.sqrt(var + 1e-5) * sd["output_net.1.weight"] + sd["output_net.1.bias"])
    return y @ sd["output_net.3.weight"].T + sd["output_net.3.bias"]


def motion_side(sds, motions, m_lens, mutant=None):
    """(movements [N, T2, Dm] of every frame, motion embeddings [N, D]) of get_motion_embeddings (evaluator_wrapper.py:175-187), input order."""
    mov = movements(sds["movement_encoder"], np.asarray(motions)[..., :-4], mutant)
    sd = _f64(sds["motion_encoder"])
    emb = mov @ sd["input_emb.weight"].T + sd["input_emb.bias"]
    return mov, bigru_head(sd, emb, np.asarray(m_lens) // 4, mutant)


def text_side(sds, word_embs, pos_ohot, cap_lens, mutant=None):
    sd = _f64(sds["text_encoder"])
    x = np.asarray(word_embs, np.float64) + (np.asarray(pos_ohot, np.float64) @ sd["pos_emb.weight"].T + sd["pos_emb.bias"])
    emb = x @ sd["input_emb.weight"].T + sd["input_emb.bias"]
    return bigru_head(sd, emb, cap_lens, mutant)


def live_mask(m_lens, T2):
    """[N, T2] bool: the movement frames the recurrence reads, j < m_lens // 4"""
    return np.arange(T2)[None, :] < (np.asarray(m_lens) // 4)[:, None]


def match(text, motion, group=32):
    """(diag [N], rank [N], margin) in fp64: d[i, j] = ||text_i - motion_j|| inside consecutive groups; rank = #{j: d[i, j] < d[i, i]};
    margin = min over rows and j != i of |d[i, j] - d[i, i]|."""
    text, motion = np.asarray(text, np.float64), np.asarray(motion, np.float64)
    N = text.shape[0]
    diag, rank, margin = np.zeros(N), np.zeros(N, np.int64), np.inf
    for g0 in range(0, N, group):
        t, m = text[g0:g0 + group], motion[g0:g0 + group]
        d = np.sqrt(((t[:, None, :] - m[None, :, :]) ** 2).sum(-1))
        own = np.diagonal(d).copy()
        diag[g0:g0 + group] = own
        rank[g0:g0 + group] = (d < own[:, None]).sum(1)
        gap = np.abs(d - own[:, None])
        np.fill_diagonal(gap, np.inf)
        margin = min(margin, gap.min())
    return diag, rank, float(margin)


def match_bound(scale):
    """the device's error allowance on a distance of size `scale`: 2^-20 of it"""
    return 2.0 ** -20 * float(scale)


def load_fixture(name):
    return dict(np.load(os.path.join(GOLDEN, f"t2m_{name}.npz")))
