"""The host statement of the plain 16-bit phase (tests/plain_stage_ref.py), pinned without a GPU: composed with every rounding off it is the oracle's
decoder; the restated GELU polynomial keeps the figure rgn_device.h documents; and the bounds tests/test_plain_stage_gpu.py holds the kernels to -
computed here from the host model alone, never typed in - tell every mutant of the statement from the statement itself.

The detection table (profiles/plain_stage_mutants.txt) is what test_mutants_are_detected prints."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import regennet_oracle as orc
from regennet_amd import synth
from tests import plain_stage_cases as C
from tests import plain_stage_ref as R

EXACT = dict(off=("*",), mut=("gelu:erf", "keep:b_k"))   # no rounding anywhere, the reference's GELU, k with its bias


@functools.lru_cache(maxsize=None)
def _model(frames):
    """(sd, cfg, x, t, y, oracle output, the stack's input rows [B T, d] and the folded cross-attention rows per layer [L][B, d]) of a 2-layer NTU model."""
    cfg = synth.get_config("ntu", layers=2, num_frames=frames)
    sd = synth.make_state_dict(cfg, seed=0)
    B, T = 3, frames
    rng = np.random.Generator(np.random.PCG64(5))
    x = torch.from_numpy(rng.standard_normal((B, cfg["njoints"], cfg["nfeats"], T)).astype(np.float32))
    t = torch.tensor([999, 500, 3])
    y = {"cmotion": torch.from_numpy(synth.make_cmotion(cfg, B, seed=1)[..., :T])}
    if y["cmotion"].shape[-1] < T:
        y["cmotion"] = torch.from_numpy(rng.standard_normal((B, cfg["njoints"], cfg["nfeats"], T)).astype(np.float32))
    ref = orc.cmdm_forward(sd, cfg, x, t, y).double().numpy()
    # the front end of cmdm_forward (oracle/regennet_oracle.py), restated in float64: what the decoder stack is fed
    g = lambda k: torch.from_numpy(np.asarray(sd[k])).double()   # noqa: E731
    pe = g("sequence_pos_encoder.pe")
    emb = F.linear(F.silu(F.linear(pe[t], g("embed_timestep.time_embed.0.weight"), g("embed_timestep.time_embed.0.bias"))),
                   g("embed_timestep.time_embed.2.weight"), g("embed_timestep.time_embed.2.bias"))[:, 0]          # [B, d]
    flat = lambda v: v.double().permute(3, 0, 1, 2).reshape(T, B, -1)   # noqa: E731
    xs = F.linear(flat(x), g("input_process.poseEmbedding.weight"), g("input_process.poseEmbedding.bias"))
    cs = F.linear(flat(y["cmotion"]), g("cmo_process.poseEmbedding.weight"), g("cmo_process.poseEmbedding.bias"))
    h = F.linear(torch.cat((xs, cs), -1), g("fuse_process.weight"), g("fuse_process.bias")) + pe[:T]              # [T, B, d]
    h = h.permute(1, 0, 2).reshape(B * T, -1)
    per = []
    for l in range(cfg["layers"]):
        p = f"seqTransDecoder.layers.{l}.multihead_attn."
        d = cfg["latent_dim"]
        v = F.linear(emb, g(p + "in_proj_weight")[2 * d:], g(p + "in_proj_bias")[2 * d:])
        per.append(F.linear(v, g(p + "out_proj.weight"), g(p + "out_proj.bias")).numpy())
    return sd, cfg, ref, h.numpy(), per


def _finish(sd, cfg, h, B, T):
    out = h @ np.asarray(sd["output_process.poseFinal.weight"], dtype=np.float64).T + np.asarray(sd["output_process.poseFinal.bias"], dtype=np.float64)
    return out.reshape(B, T, cfg["njoints"], cfg["nfeats"]).transpose(0, 2, 3, 1)


def _chain_short(c, h, w, T, per):
    att = R.attn_stage(c, h, w["Wqkv"], w["bqkv"], T)
    return R.tail_stage(c, att, h, w, T, pervec=per)


def _chain_layer(c, h, w, T, per):
    return R.layer_stage(c, h, w, T, pervec=per)


def _chain_long(c, h, w, T, per):
    """The kernel-per-stage chain of a long sequence: k_qkv_attn_long, then k_rowgemm three times."""
    att = R.attn_stage_long(c, h, w["Wqkv"], w["bqkv"], T)
    hp = R.rowgemm_stage(c, att, w["Wo"], w["bo"], "ln", Tq=T, resid=h, ga=w["g1"], ba=w["b1"], gb=w["g2"], bb=w["b2"], pervec=per)
    hid = R.rowgemm_stage(c, hp, w["W1"], w["bf1"], "act1")
    return R.rowgemm_stage(c, hid, w["W2"], w["bf2"], "ln", resid=hp, ga=w["g3"], ba=w["b3"])


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("chain,frames", [(_chain_short, 60), (_chain_layer, 60), (_chain_long, 70)], ids=["attn+tail", "layer", "long+rowgemm"])
def test_stages_compose_to_the_oracle(chain, frames, fmt):
    """Roundings off, fp64, erf GELU: the stage functions, layer after layer, ARE the reference's decoder (through the oracle) - 2e-5 is three times
    the 7e-6 that separates the fp64 stages from the oracle's fp32 evaluation (TOL["f32"] is an order looser)."""
    sd, cfg, ref, h, per = _model(frames)
    c = R.Ctx(fmt, "f64", **EXACT)
    for l in range(cfg["layers"]):
        h = chain(c, h, R.layer_weights(sd, l), frames, per[l]).numpy()
    err = float(np.abs(_finish(sd, cfg, h, 3, frames) - ref).max())
    print(f"max |stages - oracle| = {err:.3e}")
    assert err < 2e-5


def test_act2_is_the_packed_in_proj():
    """k_rowgemm's third epilogue: q | k | v of the packed in_proj, q times 1 / sqrt(dh) - the operands of the oracle's attention."""
    sd, cfg, ref, h, per = _model(70)
    w = R.layer_weights(sd, 0)
    qkv = R.rowgemm_stage(R.Ctx("bf16", "f64", off=("*",)), h, w["Wqkv"], w["bqkv"], "act2").numpy()
    want = h @ w["Wqkv"].astype(np.float64).T + w["bqkv"]
    want[:, :R.D] *= float(R.qscale_f32())
    assert np.abs(qkv - want).max() < 1e-12


def test_gelu_p13_keeps_its_documented_error():
    """rgn_device.h: 'max abs error of the GELU < 3.3e-4 over [-8, 8]: 3.21e-4 in fp64, 3.22e-4 evaluated in fp32'. (The comment said 3.2e-4 before this
    test measured it; the polynomial is unchanged.) The fp32 evaluation here has a multiply and an add where the kernel has an FMA."""
    x = torch.linspace(-8.0, 8.0, 1_600_001, dtype=torch.float64)
    for dt, documented in ((torch.float64, 3.21e-4), (torch.float32, 3.22e-4)):
        err = float((R.gelu_p13(x.to(dt)).double() - R.gelu_erf(x)).abs().max())
        print(f"gelu2_p13 vs erf GELU over [-8, 8] in {dt}: max abs error {err:.4e}")
        assert err < 3.3e-4 and abs(err - documented) < 0.005e-4
    # the other polynomial (k_rowgemm's epilogue): 'GELU error relative to |x| < 8.7e-5 over [-8, 8]: 8.2e-5 in fp64, 8.6e-5 evaluated in fp32'
    for dt, documented in ((torch.float64, 8.2e-5), (torch.float32, 8.6e-5)):
        err15 = float(((R.gelu_p15(x.to(dt)).double() - R.gelu_erf(x)).abs() / x.abs().clamp_min(1e-30)).max())
        print(f"gelu2_p15 vs erf GELU over [-8, 8] in {dt}: max error relative to |x| {err15:.4e}")
        assert err15 < 8.7e-5 and abs(err15 - documented) < 0.05e-5


@pytest.mark.parametrize("name", [c["name"] for c in C.CASES])
def test_bounds_come_from_the_family(name):
    """Every bound is twice the worst fp32 member's statistic (share floored at 0.5 %), every member lies inside it, and the fp64 statement is not
    itself an fp32 member (the family has a width)."""
    fam, bd = C.family(name), C.bounds(name)
    print(f"{name}: bound {C.fmt_stats(bd)}")
    for acc, st in zip(R.ACCS[1:], fam):
        print(f"    {acc:13s} {C.fmt_stats(st)}")
        assert C.violation(st, bd) <= 1.0 / C.FACTOR + 1e-12 or st[0] * C.FACTOR <= C.SHARE_FLOOR
    assert bd[0] >= C.SHARE_FLOOR and bd[1] > 0 and bd[2] > 0


def _detection(name):
    bd, ref = C.bounds(name), C.reference(name)
    return [(lab, st, C.violation(st, bd)) for lab, off, mut in C.mutants(name) for st in [R.stats(C.evaluate(name, "f64", off, mut), ref)]]


def test_mutants_are_detected(capsys):
    """Every applicable mutant of every case violates one of the case's three bounds by a factor >= 1.5 (plain_stage_cases.mutants: which apply, and
    why the others do not). The entry of C.WEAK is held to 'in at least one case of the kernel and format': see there."""
    lines, missed, weak_hit = [], [], set()
    for c in C.CASES:
        name, bd = c["name"], C.bounds(c["name"])
        lines.append(f"{name}: bound {C.fmt_stats(bd)}")
        for lab, st, v in _detection(name):
            key = (c["kernel"], c["fmt"], lab)
            ok = v >= C.DETECT
            if key in C.WEAK:
                weak_hit |= {key} if ok else set()
                mark = "" if ok else "   (below 1.5: C.WEAK)"
            else:
                mark = "" if ok else "   MISSED"
                if not ok:
                    missed.append((name, lab, v))
            lines.append(f"    {lab:18s} {C.fmt_stats(st)}   x {v:9.2f}{mark}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not missed, missed
    assert weak_hit == set(C.WEAK), set(C.WEAK) - weak_hit
