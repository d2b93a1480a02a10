"""CPU: what the text-to-motion evaluator promises without a GPU - the fp64 restatement reproduces the reference's recorded outputs, the parity bound of
tests/test_t2m_gpu.py separates the right arithmetic from the nearest wrong ones (bf16 operands, three structural errors), the modules carry the
reference's state-dict names, every argument check answers without a device, and the host side of regennet_amd.eval.humanml reproduces what the
reference's eval_humanml.py returned and logged on the embeddings a fixture stores."""
import ctypes
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import t2m_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _f64(name, mutant=None):
    sds, inp = t2m_ref.case_inputs(name)
    mov, motion = t2m_ref.motion_side(sds, inp["motions"], inp["m_lens"], mutant)
    text = None if mutant == "conv" else t2m_ref.text_side(sds, inp["word_embs"], inp["pos_ohot"], inp["cap_lens"], mutant)
    return inp, mov, motion, text


@pytest.mark.parametrize("name", list(t2m_ref.CASES))
def test_restatement_reproduces_the_reference(name):
    """|fp64 restatement - the reference's fp32 outputs| is ref_err by construction; recomputed here from the seeds it must come out within it again
    (the weights, inputs and the restatement are this checkout's, the outputs the reference's)."""
    fx = t2m_ref.load_fixture(name)
    inp, mov, motion, text = _f64(name)
    geo, N, T, Lw, _, _ = t2m_ref.CASES[name]
    assert np.array_equal(inp["m_lens"], fx["m_lens"]) and np.array_equal(inp["cap_lens"], fx["cap_lens"]) and int(fx["seed"]) == t2m_ref.CASE_SEEDS[name]
    assert inp["m_lens"].min() >= 4 and inp["m_lens"].max() <= T and inp["cap_lens"].min() >= 1 and inp["cap_lens"].max() <= Lw
    if name == "t2m":
        assert list(inp["m_lens"][:6]) == [196, 40, 4, 41, 42, 43] and sorted(set(inp["cap_lens"])) == list(range(1, 23))
    slack = 1.0 + 1e-6
    rows = t2m_ref.movement_rows(N)
    live = t2m_ref.live_mask(inp["m_lens"], mov.shape[1])[rows]
    assert np.abs(mov[rows] - fx["movements"])[live].max() <= fx["ref_err"][0] * slack
    assert np.abs(motion - fx["motion_emb"]).max() <= fx["ref_err"][1] * slack
    assert np.abs(text - fx["text_emb"]).max() <= fx["ref_err"][2] * slack
    for e in (fx["motion_emb"], fx["text_emb"]):
        assert 1.0 <= np.abs(e).max() <= 4.0


@pytest.mark.parametrize("name", ["t2m", "hot"])
def test_mutants_lie_outside_the_bound(name):
    """One bf16 rounding of any one operand, or any one of three structural errors, misses the GPU test's bound on every embedding it enters: the
    bound does tell wrong arithmetic from right."""
    fx = t2m_ref.load_fixture(name)
    _, _, motion, text = _f64(name)
    bm, bt = t2m_ref.bound(fx["ref_err"][1]), t2m_ref.bound(fx["ref_err"][2])
    for mutant in t2m_ref.BF16_MUTANTS + t2m_ref.STRUCTURAL_MUTANTS:
        _, _, mm, tm = _f64(name, mutant)
        em = np.abs(mm - motion).max()
        et = None if tm is None else np.abs(tm - text).max()
        print(f"{name} {mutant:12s}: motion_emb off by {em:.2e} (bound {bm:.2e}), text_emb by {'-' if et is None else format(et, '.2e')} (bound {bt:.2e})")
        assert em > bm, (mutant, em, bm)
        assert et is None or et > bt, (mutant, et, bt)


def test_state_dict_names_and_shapes_are_the_references():
    from regennet_amd.eval import t2m
    keys = json.load(open(os.path.join(t2m_ref.GOLDEN, "t2m_keys.json")))
    mods = {"movement_encoder": t2m.MovementConvEncoder(259, 512, 512), "text_encoder": t2m.TextEncoderBiGRUCo(300, 15, 512, 512, "cpu"),
            "motion_encoder": t2m.MotionEncoderBiGRUCo(512, 1024, 512, "cpu")}
    assert {p: {k: list(v.shape) for k, v in m.state_dict().items()} for p, m in mods.items()} == keys
    from regennet_amd import synth
    sds = synth.make_t2m_state_dicts()
    assert {p: {k: list(v.shape) for k, v in sd.items()} for p, sd in sds.items()} == keys
    for p, m in mods.items():
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sds[p].items()})          # strict


def test_the_new_symbols_are_declared_and_bound():
    from regennet_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "regennet_hip.h")).read()
    names = ["rgn_t2m_create", "rgn_t2m_destroy", "rgn_t2m_last_error", "rgn_t2m_load_weight", "rgn_t2m_finalize", "rgn_t2m_workspace",
             "rgn_t2m_motion_embeddings", "rgn_t2m_text_embeddings", "rgn_t2m_length_status", "rgn_t2m_match", "rgn_t2m_movements",
             "rgn_t2m_encode_movements"]
    for n in names:
        assert n in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % n, header) and getattr(lib, n) is not None, n


def _create(**over):
    from regennet_amd import _lib
    lib = _lib.load()
    c = dict(t2m_ref.REAL, unit_length=4, device=0)
    c.update(over)
    h = ctypes.c_void_p()
    rc = lib.rgn_t2m_create(ctypes.byref(_lib.RgnT2mConfig(**c)), ctypes.byref(h))
    err = (lib.rgn_t2m_last_error(None) or b"").decode()
    if rc == 0:
        assert lib.rgn_t2m_destroy(h) == 0
    return rc, err


REFUSED = [(dict(dim_pose=4), "dim_pose"), (dict(dim_pose=1025), "dim_pose"), (dict(movement_hidden=32), "movement_hidden"),
           (dict(movement_hidden=1088), "movement_hidden"), (dict(movement_latent=100), "movement_latent"), (dict(motion_hidden=0), "motion_hidden"),
           (dict(motion_hidden=1056), "motion_hidden"), (dict(text_hidden=96), "text_hidden"), (dict(dim_word=0), "dim_word"), (dict(dim_word=301), "dim_word"),
           (dict(dim_pos_ohot=0), "dim_pos_ohot"), (dict(coemb=510), "coemb"), (dict(coemb=1028), "coemb"), (dict(unit_length=2), "unit_length")]
ACCEPTED = [dict(), dict(dim_pose=251), dict(t2m_ref.SMALL), dict(dim_pose=5, movement_hidden=64, movement_latent=1024, motion_hidden=1024, text_hidden=1024,
                                                                   dim_word=4, dim_pos_ohot=1, coemb=4)]


def test_rgn_t2m_create_refuses_what_no_kernel_serves_and_accepts_the_rest():
    for over, word in REFUSED:
        rc, err = _create(**over)
        assert rc == -7 and err.startswith("rgn_t2m_create: ") and word in err, (over, rc, err)
    for over in ACCEPTED:
        rc, err = _create(**over)
        assert rc == 0 or (rc == -6 and "no HIP device" in err), (over, rc, err)


_P = ctypes.c_void_p(64)      # stands for device memory: never dereferenced
CALLS = [
    ("rgn_t2m_motion_embeddings", (None, 3, 196, _P, _P, _P, _P, 1 << 20, None), "null handle"),
    ("rgn_t2m_motion_embeddings", (None, 0, 196, _P, _P, _P, _P, 1 << 20, None), "N < 1"),
    ("rgn_t2m_motion_embeddings", (None, 3, 3, _P, _P, _P, _P, 1 << 20, None), "T outside [4, 4096]"),
    ("rgn_t2m_motion_embeddings", (None, 3, 4097, _P, _P, _P, _P, 1 << 20, None), "T outside [4, 4096]"),
    ("rgn_t2m_motion_embeddings", (None, 3, 196, None, _P, _P, _P, 1 << 20, None), "null motions"),
    ("rgn_t2m_motion_embeddings", (None, 3, 196, _P, None, _P, _P, 1 << 20, None), "m_lens"),
    ("rgn_t2m_motion_embeddings", (None, 3, 196, _P, _P, None, _P, 1 << 20, None), "output"),
    ("rgn_t2m_motion_embeddings", (None, 3, 196, _P, _P, _P, None, 1 << 20, None), "null workspace"),
    ("rgn_t2m_text_embeddings", (None, 3, 22, _P, _P, _P, _P, _P, 1 << 20, None), "null handle"),
    ("rgn_t2m_text_embeddings", (None, -1, 22, _P, _P, _P, _P, _P, 1 << 20, None), "N < 1"),
    ("rgn_t2m_text_embeddings", (None, 3, 0, _P, _P, _P, _P, _P, 1 << 20, None), "Lw outside [1, 256]"),
    ("rgn_t2m_text_embeddings", (None, 3, 257, _P, _P, _P, _P, _P, 1 << 20, None), "Lw outside [1, 256]"),
    ("rgn_t2m_text_embeddings", (None, 3, 22, None, _P, _P, _P, _P, 1 << 20, None), "null word_embs"),
    ("rgn_t2m_text_embeddings", (None, 3, 22, _P, None, _P, _P, _P, 1 << 20, None), "pos_ohot"),
    ("rgn_t2m_text_embeddings", (None, 3, 22, _P, _P, None, _P, _P, 1 << 20, None), "cap_lens"),
    ("rgn_t2m_text_embeddings", (None, 3, 22, _P, _P, _P, _P, None, 1 << 20, None), "null workspace"),
    ("rgn_t2m_movements", (None, 3, 196, 263, None, None, _P, _P, 1 << 20, None), "null motions"),
    ("rgn_t2m_movements", (None, 3, 196, 263, _P, None, _P, _P, 1 << 20, None), "null handle"),
    ("rgn_t2m_encode_movements", (None, 3, 0, _P, _P, _P, _P, 1 << 20, None), "T2 outside"),
    ("rgn_t2m_encode_movements", (None, 3, 49, _P, None, _P, _P, 1 << 20, None), "m_lens"),
    ("rgn_t2m_match", (0, None, _P, 4, 4, 4, _P, _P, None), "null text"),
    ("rgn_t2m_match", (0, _P, _P, 0, 4, 4, _P, _P, None), "N < 1"),
    ("rgn_t2m_match", (0, _P, _P, 4, 6, 4, _P, _P, None), "D must be a multiple of 4"),
    ("rgn_t2m_match", (0, _P, _P, 4, 1028, 4, _P, _P, None), "D must be a multiple of 4"),
    ("rgn_t2m_match", (0, _P, _P, 4, 4, 0, _P, _P, None), "group outside [1, 32]"),
    ("rgn_t2m_match", (0, _P, _P, 4, 4, 33, _P, _P, None), "group outside [1, 32]"),
    ("rgn_t2m_workspace", (None, 1, 4, 1, None), "null handle"),
]


@pytest.mark.parametrize("fn,args,text", CALLS)
def test_every_argument_check_answers_without_a_device(fn, args, text):
    from regennet_amd import _lib
    lib = _lib.load()
    assert getattr(lib, fn)(*args) == -1
    err = (lib.rgn_t2m_last_error(None) or b"").decode()
    assert err.startswith(fn + ": ") and text in err, err


def test_null_handles_are_refused():
    from regennet_amd import _lib
    lib = _lib.load()
    assert lib.rgn_t2m_create(None, None) == -1 and b"null" in lib.rgn_t2m_last_error(None)
    v = ctypes.c_int32(0)
    assert lib.rgn_t2m_destroy(None) == -1 and lib.rgn_t2m_finalize(None) == -1 and lib.rgn_t2m_length_status(None, ctypes.byref(v)) == -1


def test_the_host_rules_and_the_workspace_plan():
    """tools/t2m_args_check.cpp, linked against the library: every refusal with its text, every accepted geometry as far as the device, and the workspace
    plan aligned, disjoint and monotone in N, T and Lw (the plan is host code of rgn_t2m_check.h; a handle needs a device, the plan does not)."""
    import __graft_entry__ as g
    g.build()
    exe = os.path.join(ROOT, "build", "t2m_args_check_plain")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", os.path.join(ROOT, "tools", "t2m_args_check.cpp"), "-L" + os.path.dirname(g.LIB), "-l:" + os.path.basename(g.LIB),
                           "-Wl,-rpath," + os.path.dirname(g.LIB),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "UNEXPECTED" not in r.stdout and "0 unexpected" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
    m = re.search(r"(\d+) workspace plans checked \(largest \d+ bytes\), (\d+) consecutive steps swept", r.stdout)
    assert m and int(m.group(1)) == 90 and int(m.group(2)) > 9000 and "null handles refused" in r.stdout


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_gpu_means_loud_failure_not_fallback():
    from regennet_amd.eval import t2m
    m = t2m.MotionEncoderBiGRUCo(64, 64, 64, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 3, 64), torch.tensor([3, 2]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t2m.MovementConvEncoder(19, 64, 64)(torch.zeros(2, 8, 19))


# ---- the host side of regennet_amd.eval.humanml on the embeddings the metric fixture stores -------------------------------------------------------------
class _StubWrapper:
    """looks the recorded embeddings up by the motion's first value and applies the reference's row order, as EvaluatorMDMWrapper does"""

    def __init__(self, fx, gt, gen):
        self.table = {}
        for motions, emb in ((gt["motions"], fx["emb_gt"]), (gen, fx["emb_gen"])):
            for m, e in zip(motions, emb):
                self.table[float(m[0, 0])] = e
        self.text = {float(w[0, 0]): e for w, e in zip(gt["word_embs"], fx["text"])}

    def get_motion_embeddings(self, motions, m_lens):
        idx = np.argsort(torch.as_tensor(m_lens).tolist())[::-1].copy()
        return torch.from_numpy(np.stack([self.table[float(m[0, 0])] for m in motions]))[idx]

    def get_co_embeddings(self, word_embs, pos_ohot, cap_lens, motions, m_lens):
        idx = np.argsort(torch.as_tensor(m_lens).tolist())[::-1].copy()
        return torch.from_numpy(np.stack([self.text[float(w[0, 0])] for w in word_embs]))[idx], self.get_motion_embeddings(motions, m_lens)


def _host_match(text, motion, group=32):
    diag, rank, _ = t2m_ref.match(text.numpy(), motion.numpy(), group)
    return torch.from_numpy(diag).float(), torch.from_numpy(rank).int()


def _mask(lines):
    return [re.sub(r"-?\d+\.\d+", "#", ln) for ln in lines if not ln.startswith("Time:")]


def test_evaluation_reproduces_the_reference_on_recorded_embeddings(tmp_path, monkeypatch, capsys):
    from regennet_amd import _lib
    from regennet_amd.eval import humanml
    fx = dict(np.load(os.path.join(t2m_ref.GOLDEN, "t2m_eval.npz")))
    _, gt, gen = t2m_ref.eval_inputs()
    w = _StubWrapper(fx, gt, gen)
    monkeypatch.setattr(_lib, "t2m_match", _host_match)
    order, aligned = t2m_ref.eval_order(gt["cap_lens"], gt["m_lens"])
    texts = (gt["word_embs"][order], gt["pos_ohot"][order], gt["cap_lens"][order])
    gt_loader = humanml.array_loader(*texts, gt["motions"][order], gt["m_lens"][order], device="cpu")
    gen_loader = humanml.array_loader(*texts, gen[order], gt["m_lens"][order], device="cpu")
    mm = [(torch.from_numpy(m)[None], torch.from_numpy(l)[None]) for m, l in t2m_ref.eval_mm(gen, gt["m_lens"])]
    ranks = []
    log = tmp_path / "eval.log"
    mean = humanml.evaluation(w, gt_loader, {"vald": lambda: (gen_loader, mm)}, str(log), replication_times=2, diversity_times=t2m_ref.EVAL_DIVERSITY_TIMES,
                              mm_num_times=t2m_ref.EVAL_MM_TIMES, run_mm=True, seed=t2m_ref.EVAL_SEED, ranks=ranks)
    assert _mask(log.read_text().splitlines()) == _mask(str(fx["log"]).splitlines())                   # the reference's format strings, line by line
    assert len(mean) == sum(k.startswith("mean_") for k in fx) == 9
    for k, v in mean.items():
        ref = fx["mean_" + k.replace(" ", "_")]
        if k.startswith("FID"):
            # both sets are rank-deficient (64 samples of 512 features): the reference's scipy sqrtm leaves |FID(gt, gt)| = 2.1e-5 where the value is
            # 0 - its own error at this rank - and the host eigen-solver differs from it by 7e-6 on FID_vald; both are held to 8 x that residue. (On
            # the device the generated set meets the project's 1e-6 relative tolerance: tests/test_t2m_gpu.py.)
            assert abs(float(v) - (0.0 if k == "FID_ground truth" else float(ref))) <= 8 * abs(float(fx["mean_FID_ground_truth"])), (k, v, ref)
        elif k in t2m_ref.EVAL_METRICS:      # on the reference's own fp32 embeddings: its error against fp64, under the parity rule
            f64 = float(fx["f64_" + k.replace(" ", "_")])
            assert abs(float(v) - f64) <= t2m_ref.bound(fx["ref_err_" + k.replace(" ", "_")]), (k, v, f64)
        else:
            assert np.array_equal(v, ref), (k, v, ref)
    # rank -> top-k: the recorded ranks give the recorded R-precision, and the loaders' ranks are the recorded ones in the wrapper's row order
    for tag, name in (("gt", "ground truth"), ("gen", "vald")):
        hits = humanml.top_k_from_rank(torch.from_numpy(fx[f"rank_{tag}"]), 3).numpy()
        assert np.array_equal(hits.mean(0), fx["mean_R_precision_" + name.replace(" ", "_")])
        assert np.array_equal(ranks[0][name].numpy(), fx[f"rank_{tag}"][aligned])
    m, ci = humanml.get_metric_statistics(np.array([[1.0, 2.0], [3.0, 6.0]]), 2)
    assert np.allclose(m, [2.0, 4.0]) and np.allclose(ci, 1.96 * np.array([1.0, 2.0]) / np.sqrt(2))


def test_renormalisation_and_eval_modes():
    from regennet_amd.eval import humanml
    rng = np.random.Generator(np.random.PCG64(3))
    x, mean, std, me, se = (rng.standard_normal(s).astype(np.float32) for s in ((4, 9, 7), (7,), (7,), (7,), (7,)))
    got = humanml.renormalise(torch.from_numpy(x), mean, std, me, se).numpy()
    assert np.allclose(got, (x * std + mean - me) / se, rtol=1e-6, atol=1e-6)          # comp_v6_model_dataset.py:248-249
    assert humanml.EVAL_MODES == {"debug": (1000, False, 0, 0, 0, 300, 5), "wo_mm": (1000, False, 0, 0, 0, 300, 20), "mm_short": (1000, True, 100, 30, 10, 300, 5)}
    assert humanml.BATCH_SIZE == 32
    with pytest.raises(SystemExit, match="32"):
        humanml.main(["--synthetic", "--batch_size", "64"])


class _StubDiffusion:
    """p_sample_loop returns a known tensor: call c gives c + (b, feature, frame) coded in the value"""

    def __init__(self):
        self.calls = []

    def p_sample_loop(self, model, shape, clip_denoised=True, model_kwargs=None, **kw):
        assert clip_denoised is False and kw.get("skip_timesteps") == 0 and kw.get("noise") is None
        c = len(self.calls)
        self.calls.append(model_kwargs["y"])
        b, f, t = np.meshgrid(np.arange(shape[0]), np.arange(shape[1] * shape[2]), np.arange(shape[3]), indexing="ij")
        return torch.from_numpy((1000.0 * c + 100.0 * b + f + 0.01 * t).astype(np.float32)).reshape(shape)


def test_generated_loader_follows_the_reference_dataset():
    """GeneratedT2MLoader against comp_v6_model_dataset.py:146-262 with a stub sampler: which batches are sampled and how often, the sample's
    [bs, njoints, nfeats, T] -> [bs, T, features] turn, the renormalisation, the multimodality stacking, num_samples_limit and the guidance scale."""
    from regennet_amd.eval import humanml
    bs, J, T, Lw = 4, 7, 8, 3
    rng = np.random.Generator(np.random.PCG64(1))
    mean, std, me, se = (rng.standard_normal(J).astype(np.float32) for _ in range(4))
    batches = [{"shape": (bs, J, 1, T), "word_embs": rng.standard_normal((bs, Lw, 12)).astype(np.float32), "pos_ohot": np.zeros((bs, Lw, 5), np.float32),
                "cap_lens": np.array([3, 2, 2, 1]), "y": {"lengths": torch.tensor([8, 6, 5, 4]) + i, "text_features": torch.zeros(bs, 4), "text": [f"t{i}"] * bs}}
               for i in range(4)]
    seed, repeats = 3, 3
    mm_idx = np.sort(np.random.RandomState(seed).choice(3, 2 // bs + 1, replace=False))          # real_num_batches = 8 // 4 + 1 = 3
    diff = _StubDiffusion()
    ld = humanml.GeneratedT2MLoader(torch.nn.Linear(1, 1), diff, batches, mm_num_samples=2, mm_num_repeats=repeats, max_motion_length=T,
                                    num_samples_limit=8, scale=2.5, mean=mean, std=std, mean_for_eval=me, std_for_eval=se, seed=seed)
    sampled = [i for i in range(2)]                           # the loop stops once num_samples_limit motions exist (:179-180)
    calls = sum(repeats if i in mm_idx else 1 for i in sampled)
    assert len(diff.calls) == calls and all(torch.equal(y["scale"], torch.full((bs,), 2.5)) for y in diff.calls)
    loader, mm = ld()
    assert loader is ld.motion_loader() and mm is ld.mm_loader() and len(loader) == 2
    c = 0
    for i, batch in zip(sampled, loader):
        word, pos, text, cap, motion, lens, _ = batch
        assert np.array_equal(word.numpy(), batches[i]["word_embs"]) and torch.equal(cap, torch.tensor([3, 2, 2, 1])) and text == [f"t{i}"] * bs
        assert torch.equal(lens, batches[i]["y"]["lengths"]) and motion.shape == (bs, T, J)
        b, t, f = np.meshgrid(np.arange(bs), np.arange(T), np.arange(J), indexing="ij")
        raw = (1000.0 * c + 100.0 * b + f + 0.01 * t).astype(np.float32)                 # the first repeat's sample, frames x features
        assert np.allclose(motion.numpy(), (raw * std + mean - me) / se, rtol=1e-6, atol=1e-5)
        c += repeats if i in mm_idx else 1
    hit = [i for i in sampled if i in mm_idx]
    assert hit and len(mm) == bs * len(hit)
    for motions, lens in mm:                                  # (1, repeats, T, features), the repeats of ONE text; lengths repeated alike
        assert motions.shape == (1, repeats, T, J) and lens.shape == (1, repeats) and len(set(lens[0].tolist())) == 1
        step = (motions[0, 1] - motions[0, 0]).numpy() * se / std
        assert np.allclose(step, 1000.0, rtol=1e-4)           # consecutive repeats are consecutive sampler calls of the same row
    with pytest.raises(AssertionError):
        humanml.GeneratedT2MLoader(torch.nn.Linear(1, 1), _StubDiffusion(), batches[:1], mm_num_samples=4, mm_num_repeats=2, max_motion_length=T,
                                   num_samples_limit=None)                               # :151: mm_num_samples < len(dataset)
