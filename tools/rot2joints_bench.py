"""Time the regressed joint types (rgn_rot2joints) beside what a user runs without them, on the GPU:

    python tools/rot2joints_bench.py [--out profiles/rot2joints_bench.txt] [--rounds 5] [--reps 10]

Synthetic body of SMPL's size (synth.make_body(24, 6890)), 21 vertex joints and 9 regressed joints (synth.make_joint_regressors: 6 weights a row;
and once a DENSE regressor, every vertex weighed), the 'vibe' map (49 rows), rot6d, translation, no mask, one person; B = 256, T = 60 and B = 1.
Two figures per row, measured in ONE process in ALTERNATING windows (a, b, a, b, ...; each window: `reps` back-to-back calls from Python between
one pair of device events, after a warm-up of both), so that a drift of the box hits both alike; per figure the median over the rounds and the
spread (min .. max) of the per-call time:
  (a) rot2joints   BodyEngine.rot2joints: the vertices of S skinned in registers, weighed into joints, never written
  (b) by hand      BodyEngine.rot2verts into [B, V, 3, T], then in torch: gather the vertex joints, einsum the regressor over the vertex array,
                   Engine.rot2xyz for the chain joints, subtract the root, index by the map, add the translation
with the workspace and output bytes of both. The two results are checked against each other to fp32 rounding; parity with the reference is
tests/test_rot2joints_gpu.py. Nothing here is a pass / fail check of speed."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from regennet_amd import _lib, synth  # noqa: E402
from tools.rot2xyz_shaped_bench import alternate  # noqa: E402

J, V, NP, JR, SUPPORT = 24, 6890, 21, 9, 6
SHAPES = [(256, 60), (1, 60)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", default=5, type=int)
    ap.add_argument("--reps", default=10, type=int)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs a GPU: numbers that were not measured on one are reported as 'not measured'"
    from tests.helpers import build_hip
    cfg = synth.get_config("tiny")
    model, _ = build_hip(cfg, synth.make_state_dict(cfg, seed=0), resp="5")
    eng, _ = model._get_engine(2, cfg["num_frames"])
    dev = torch.device("cuda:0")
    body = synth.make_body(J, V, seed=J)
    regs = synth.make_joint_regressors(body, npicks=NP, nreg=JR, support=SUPPORT)
    dense = np.random.Generator(np.random.PCG64(9)).uniform(-1, 1, (JR, V)).astype(np.float32) / V
    stream = torch.cuda.current_stream().cuda_stream
    flags = _lib.R2X_TRANSLATION | _lib.R2X_GLOB | _lib.R2X_VERTSTRANS
    rest, parents = body["rest_joints"].astype(np.float64), body["parents"]
    jmap, root = regs["joint_maps"]["vibe"], regs["map_roots"]["vibe"]
    assert int(jmap[root]) == 0
    midx = torch.from_numpy(jmap.astype(np.int64)).to(dev)
    vj = torch.from_numpy(regs["vertex_joints"].astype(np.int64)).to(dev)
    rest0 = torch.from_numpy(rest[0].astype(np.float32)).to(dev).view(1, 1, 3, 1)
    fmt = lambda m: f"{m[0]:9.3f} ({m[1]:.3f} .. {m[2]:.3f})"            # noqa: E731
    lines = [f"rgn_rot2joints on {torch.cuda.get_device_name(0)} (synthetic body: {J} joints, {V} vertices; {NP} vertex joints, {JR} regressed joints; 'vibe': "
             f"{len(jmap)} rows; rot6d, translation, no mask, one person); ms per call from Python, {args.rounds} alternating windows of {args.reps} calls: "
             f"median (min .. max)",
             f"{'regressor':>10s} {'|S|':>5s} {'B':>4s} {'T':>3s} | {'(a) rot2joints':>28s} {'work B':>10s} {'out B':>9s} | {'(b) rot2verts + torch':>28s} "
             f"{'work B':>10s} {'verts B':>11s} | {'b / a':>6s}"]
    for label, reg in (("6 a row", regs["J_regressor_extra"]), ("dense", dense)):
        beng = _lib.BodyEngine(body["mesh"], J, 0)
        beng.set_joint_regressors(regs["vertex_joints"], reg)
        nS = int(((reg != 0).any(0) | np.isin(np.arange(V), regs["vertex_joints"])).sum())
        regd = torch.from_numpy(reg).to(dev)
        for B, T in SHAPES:
            rng = np.random.Generator(np.random.PCG64(B + T))
            x = torch.from_numpy(rng.standard_normal((B, J + 1, 6, T)).astype(np.float32)).to(dev)
            oa = torch.empty((B, len(jmap), 3, T), device=dev)
            verts, jx = torch.empty((B, V, 3, T), device=dev), torch.empty((B, J, 3, T), device=dev)
            wa = torch.empty(beng.joints_workspace_bytes(B, T, 1), dtype=torch.uint8, device=dev)
            wb = torch.empty(beng.workspace_bytes(B, T, 1), dtype=torch.uint8, device=dev)
            res = {}

            def a():
                beng.rot2joints(x, None, rest, parents, 0, 1, flags, None, None, jmap, root, oa, None, wa, stream)

            def b():
                beng.rot2verts(x, None, rest, parents, 0, 1, _lib.R2X_TRANSLATION | _lib.R2X_GLOB, None, None, verts, None, wb, stream)
                eng.rot2xyz(x, None, rest, parents, 0, 1, _lib.R2X_TRANSLATION | _lib.R2X_GLOB, None, jx, None, stream)      # chain joints - joint 0
                extra = torch.einsum("jv,bvct->bjct", regd, verts)
                allj = torch.cat([jx, verts[:, vj] - rest0, extra - rest0], dim=1)
                tr = x[:, -1, :3]
                res["b"] = allj[:, midx] + (tr - tr[:, :, :1])[:, None]

            ta, tb = alternate([(a, args.reps), (b, args.reps)], args.rounds)
            err = float((oa - res["b"]).abs().max())
            assert err < 1e-4, err                                   # (the timed calls computed the same thing)
            lines.append(f"{label:>10s} {nS:5d} {B:4d} {T:3d} | {fmt(ta):>28s} {wa.numel():10d} {oa.numel() * 4:9d} | {fmt(tb):>28s} {wb.numel():10d} "
                         f"{verts.numel() * 4:11d} | {tb[0] / ta[0]:6.2f}   max|a - b| {err:.1e}")
            del oa, verts, jx, wa, wb, res
        beng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
