"""Time the unconstrained evaluation's metrics at the reference's own sizes: N = 1000, 4096 and 16384 features of D = 256, KID over 100 subsets of
1000, precision / recall with k = 3 - the fused calls (rgn_poly_mmd; rgn_knn_radius + rgn_manifold_hits) against a composition of torch calls on
the same GPU (index_select + bmm + elementwise operations for KID, which materialises the [100, 1000, 1000] x 3 kernel matrices; cdist + kthvalue +
compare for precision / recall; cdist in its default mode, which forms large distance matrices from a matrix product), each with the peak device memory it allocates, and - at N = 1000 only, --host_reference DIR - the reference's own
functions on the host, in a child process with a time limit of its own (skipped with a note if it does not finish). Figures only: nothing is gated.

    python tools/unconstrained_bench.py [--out profiles/unconstrained_bench.txt] [--sizes 1000,4096,16384] [--host_reference DIR --host_limit 600]

Method: every shape is warmed up twice; a timed window is `reps` back-to-back calls between two device events with a synchronise at the end, reps
chosen so that the window lasts about 0.3 s; the two versions alternate over 5 rounds and the median window is reported (with min and max)."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, torch, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def compare(torch, fns, rounds=5):
    """fns: {name: callable}. -> {name: (median ms, min, max, peak bytes)}; the versions alternate."""
    reps, peak = {}, {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
        reps[name] = max(1, int(300.0 / max(timed(fn, torch, 1), 1e-3)))
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(timed(fn, torch, reps[name]))
    return {name: (float(np.median(v)), min(v), max(v), peak[name]) for name, v in ms.items()}


def host_reference(ref_dir, limit, n, subsets, subset_size):
    """The reference's calculate-kid loop and precision_and_recall on the host, in a child with a time limit."""
    code = f"""
import importlib.util, os, sys, time
import numpy as np, torch
sys.path.insert(0, {ROOT!r})
from tests import unconstrained_ref as ur
def load(name):
    spec = importlib.util.spec_from_file_location('ref_' + name, os.path.join({ref_dir!r}, 'eval', 'unconstrained', 'metrics', name + '.py'))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod); return mod
real, gen = ur.make_features(0, {n}, {n}, 256)
np.random.seed(0)
t = time.time(); load('kid').polynomial_mmd_averages(real, gen, n_subsets={subsets}, subset_size={subset_size}); print('host KID %.1f s' % (time.time() - t), flush=True)
t = time.time(); load('precision_recall').precision_and_recall(torch.from_numpy(gen), torch.from_numpy(real)); print('host precision / recall %.1f s' % (time.time() - t), flush=True)
"""
    try:
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=limit)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("host ")]
        return lines or [f"host reference failed (exit {p.returncode}): {p.stderr.strip().splitlines()[-1] if p.stderr.strip() else ''}"]
    except subprocess.TimeoutExpired as e:
        done = [ln for ln in (e.stdout or b"").decode().splitlines() if ln.startswith("host ")]
        return done + [f"host reference: not finished within its limit of {limit} s - skipped"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unconstrained_bench.txt"))
    ap.add_argument("--sizes", default="1000,4096,16384")
    ap.add_argument("--subsets", type=int, default=100)
    ap.add_argument("--subset_size", type=int, default=1000)
    ap.add_argument("--host_reference", default="", help="the reference's checkout: time its own functions on the host at the first size")
    ap.add_argument("--host_limit", type=int, default=600)
    ap.add_argument("--host_only", action="store_true", help="only the host reference (no GPU needed); appends to --out")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    lines = []
    if not a.host_only:
        import torch

        from regennet_amd.eval import unconstrained as un
        from tests import unconstrained_ref as ur
        assert torch.cuda.is_available(), "the benchmark needs a GPU"
        lines.append(f"{torch.cuda.get_device_name(0)}; D = 256, KID over {a.subsets} subsets of {a.subset_size}, precision / recall with k = 3; ms per call: median (min .. max) of 5 windows of ~0.3 s")
        for n in sizes:
            real, gen = (torch.from_numpy(x).cuda() for x in ur.make_features(0, n, n, 256))
            np.random.seed(0)
            idx_g, idx_r = un.draw_subset_indices(n, n, a.subsets, a.subset_size)
            ig, ir = torch.from_numpy(idx_g).cuda().long(), torch.from_numpy(idx_r).cuda().long()
            gam = 1.0 / 256

            def kid_fused():
                return un.poly_mmd(real, gen, idx_g, idx_r)

            def kid_torch():
                X = real.index_select(0, ig.reshape(-1)).reshape(a.subsets, a.subset_size, -1)
                Y = gen.index_select(0, ir.reshape(-1)).reshape(a.subsets, a.subset_size, -1)
                Ks = [(torch.bmm(p, q.transpose(1, 2)) * gam + 1.0) ** 3 for p, q in ((X, X), (X, Y), (Y, Y))]
                m = a.subset_size
                dX, dY = Ks[0].diagonal(dim1=1, dim2=2), Ks[2].diagonal(dim1=1, dim2=2)
                sums = [K.double().sum(2) for K in Ks]
                return (sums[0].sum(1) - dX.double().sum(1) + sums[2].sum(1) - dY.double().sum(1)) / (m * (m - 1)) - 2 * sums[1].sum(1) / (m * m)   # (mmd2 only: var_est's further sums are not even charged)

            def pr_fused():
                return un.precision_and_recall(gen, real)

            def pr_torch():
                out = []
                for A, B in ((real, gen), (gen, real)):
                    r = torch.cdist(A, A).kthvalue(4, dim=1).values      # k = 3, 0-based
                    out.append((torch.cdist(B, A) <= r[None, :]).any(1).sum().item() / len(B))
                return out

            fused_mmd, torch_mmd = kid_fused()[0].cpu().numpy(), kid_torch().cpu().numpy()
            res = compare(torch, {"KID fused": kid_fused, "KID torch": kid_torch, "P&R fused": pr_fused, "P&R torch": pr_torch})
            lines.append(f"N = {n}")
            for name, (med, lo, hi, peak) in res.items():
                lines.append("  %-10s %10.3f ms (%.3f .. %.3f)   peak device memory of the call %8.1f MiB" % (name, med, lo, hi, peak / 2 ** 20))
            lines.append("  KID  torch / fused = %.2f   (max |mmd2 fused - torch| = %.2e; the torch composition's kernel matrices are fp32 bmm results and it forms mmd2 only)"
                         % (res["KID torch"][0] / res["KID fused"][0], np.abs(fused_mmd - torch_mmd).max()))
            lines.append("  P&R  torch / fused = %.2f   (fused %s, torch %s)" % (res["P&R torch"][0] / res["P&R fused"][0], pr_fused(), tuple(pr_torch())))
            if res["KID fused"][0] >= res["KID torch"][0]:
                lines.append("  the fused KID kernel does NOT beat the torch composition at this size")
            print("\n".join(lines[-8:]), flush=True)
            del real, gen
            torch.cuda.empty_cache()
    if a.host_reference:
        t = time.time()
        lines.append(f"the reference's own functions on the host at N = {sizes[0]} ({os.cpu_count()} CPUs visible):")
        lines += ["  " + ln for ln in host_reference(a.host_reference, a.host_limit, sizes[0], a.subsets, a.subset_size)]
        print("\n".join(lines[-3:]), f"({time.time() - t:.0f} s)", flush=True)
    else:
        lines.append("the reference's functions on the host: not measured in this run (no --host_reference)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.host_only else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
