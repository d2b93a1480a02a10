"""Speed of the recogniser on small skeletons (figures: profiles/small_graph_bench.txt).

    python tools/small_graph_bench.py [--rounds 5] [--window_ms 400] [--only NAME]

Device events around batches of forwards, a warm-up first, as many repetitions per timing as fill `--window_ms`; the compared forms ALTERNATE inside one
call (form A, form B, form A, ... per round), so that clock and cache state drift over both alike. Reported per form: median and min .. max of the
rounds, in ms per forward. Cases:

  uncond N=64 / N=1024   the unconstrained evaluator: V = 15 (padded to 16), six blocks, one person, 3 channels, T = 60   default | SG_NO_WINDOW = 1
  smpl N=256             the 25-joint evaluator: V = 25 (padded to 28), ten blocks, two persons, 12 channels, T = 60      default | SG_NO_WINDOW = 1 | V = 28

The V = 28 handle is the baseline of the ten-block case: 28-node graphs dispatch exactly as before this tool's kernel existed (stride-1 temporal
convolutions as row-shifted GEMMs + k_sg_post), and V = 25 pads to 28, so the row count and the work are the same. Its own spread over the rounds is what
"not slower" is judged against."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from regennet_amd import synth  # noqa: E402
from regennet_amd.eval.stgcn import SIX_BLOCKS, STGCN  # noqa: E402


def build(V, in_channels, persons, blocks, opts):
    sd = synth.make_stgcn_state_dict(synth.make_stgcn_graph(V), num_class=12, in_channels=in_channels, num_person=persons, seed=V, blocks=blocks)
    m = STGCN(in_channels=in_channels, num_class=12, num_person=persons, num_nodes=V, device="cuda:0", blocks=blocks)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m.engine_options = dict(opts)
    return m.to("cuda:0").eval()


def timed(model, x, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        model({"output": x})
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def run_case(name, forms, N, T, rounds, window_ms):
    """forms: [(label, V, in_channels, persons, blocks, opts)]"""
    models = [(label, build(V, C, M, blocks, opts), torch.randn(N, V, C, T, device="cuda:0")) for label, V, C, M, blocks, opts in forms]
    reps = []
    for _, m, x in models:                                  # warm-up (engine build, first launches), then size the repetitions
        for _ in range(3):
            m({"output": x})
        torch.cuda.synchronize()
        reps.append(max(3, int(window_ms / max(timed(m, x, 3), 1e-3))))
    times = [[] for _ in models]
    for _ in range(rounds):
        for i, (_, m, x) in enumerate(models):              # the forms alternate inside a round
            times[i].append(timed(m, x, reps[i]))
    print(f"{name}: N = {N}, T = {T}, {rounds} rounds")
    base = statistics.median(times[0])
    for (label, _, _), t, r in zip(models, times, reps):
        med = statistics.median(t)
        print(f"  {label:34s} median {med:8.4f} ms  min {min(t):8.4f}  max {max(t):8.4f}  spread {100 * (max(t) - min(t)) / med:5.2f} %  x{med / base:5.3f} of the first  ({r} forwards per timing)")
    for _, m, _ in models:
        m._engine.close()
        m._engine, m._stale = None, True
    return times


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window_ms", type=float, default=400.0)
    ap.add_argument("--only", default="", help="run the case whose name starts with this")
    args = ap.parse_args(argv)
    un = lambda label, opts: (label, 15, 3, 1, SIX_BLOCKS, opts)
    cases = [
        ("uncond N=64", [un("k_sg_tconv_pre (default)", {}), un("SG_NO_WINDOW = 1", {"SG_NO_WINDOW": 1})], 64, 60),
        ("uncond N=1024", [un("k_sg_tconv_pre (default)", {}), un("SG_NO_WINDOW = 1", {"SG_NO_WINDOW": 1})], 1024, 60),
        ("smpl N=256", [("V = 28 (unchanged dispatch)", 28, 12, 2, None, {}), ("V = 25 k_sg_tconv_pre (default)", 25, 12, 2, None, {}),
                        ("V = 25 SG_NO_WINDOW = 1", 25, 12, 2, None, {"SG_NO_WINDOW": 1}), ("V = 28 again", 28, 12, 2, None, {})], 256, 60),
    ]
    for name, forms, N, T in cases:
        if name.startswith(args.only):
            run_case(name, forms, N, T, args.rounds, args.window_ms)


if __name__ == "__main__":
    main()
