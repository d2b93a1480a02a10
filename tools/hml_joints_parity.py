"""Record the parity of rgn_hml_to_joints:  python tools/hml_joints_parity.py [--out profiles/hml_joints_parity.txt]

Per fixture of tests/golden/hml_*.npz and per synthetic shape of tests/test_hml_gpu.py: the largest |kernel - fp64 restatement| over its bound
2^-23 |ref| + (T + 16) 2^-52 A on the GPU; per fixture also the largest |reference's fp32 run - restatement| over ITS bound gamma_T(2^-24) A, and by how
many of those bounds every structural mutant of tests/hml_ref.py misses the fixture. The bounds are derived in tests/hml_ref.py; the tests assert them,
this tool only writes the figures down."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from regennet_amd.sample.render import postprocessing_engine  # noqa: E402
from regennet_amd.utils.hml import hml_to_joints  # noqa: E402
from tests import hml_ref  # noqa: E402
from tests.test_hml_gpu import FIXTURES, SHAPES, load_fixture  # noqa: E402


def over(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err > 0, err / bound, 0.0).max())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs a GPU: numbers that were not measured on one are reported as 'not measured'"
    _, eng = postprocessing_engine(torch.device("cuda", 0))

    def kernel(x, mean, std):
        return hml_to_joints(torch.from_numpy(x).cuda(), mean, std, engine=eng).cpu().numpy().astype(np.float64)

    lines = [f"rgn_hml_to_joints on {torch.cuda.get_device_name(0)}: |kernel - fp64 restatement| against 2^-23 |ref| + (T + 16) 2^-52 A, the reference's fp32 run "
             "against gamma_T(2^-24) A, and the structural mutants against the latter, each at the element with the largest error / bound",
             f"{'case':<22s} {'kernel err':>11s} {'/ bound':>8s} | {'ref fp32 err':>12s} {'/ bound':>8s} | mutants miss the fixture by (bounds)"]
    smallest = (np.inf, "", "")
    for name in FIXTURES:
        x, mean, std, expected = load_fixture(name)
        B, D, _, T = x.shape
        ref, A = hml_ref.hml_joints_ref(x, mean, std), hml_ref.error_model(x, mean, std)
        kerr = np.abs(kernel(x, mean, std) - ref)
        rerr, rb = np.abs(expected - ref), hml_ref.gamma32(T) * A
        miss = {m: hml_ref.miss_ratio(hml_ref.hml_joints_ref(x, mean, std, mutant=m), expected.astype(np.float64), rb)
                for m, applies in hml_ref.MUTANTS.items() if applies(B, D, T, mean is not None)}
        for m, r in miss.items():
            smallest = min(smallest, (r, m, name))
        lines.append(f"{name:<22s} {kerr.max():11.3e} {over(kerr, hml_ref.gpu_bound(ref, A, T)):8.4f} | {rerr.max():12.3e} {over(rerr, rb):8.4f} | "
                     + ", ".join(f"{m} {r:.0f}" for m, r in miss.items()))
    for B, J, T, raw in SHAPES:
        x, mean, std = hml_ref.make_inputs(B, hml_ref.rows_of(J), T, seed=100 + 7 * T + J, raw=raw)
        ref, A = hml_ref.hml_joints_ref(x, mean, std), hml_ref.error_model(x, mean, std)
        kerr = np.abs(kernel(x, mean, std) - ref)
        lines.append(f"{f'B{B} J{J} T{T}' + (' raw' if raw else ''):<22s} {kerr.max():11.3e} {over(kerr, hml_ref.gpu_bound(ref, A, T)):8.4f} |")
    lines.append(f"smallest mutant ratio: {smallest[0]:.0f} ({smallest[1]} on {smallest[2]}); required: 100")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
