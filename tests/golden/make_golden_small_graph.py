"""Golden vectors of the recogniser on SMALL skeletons, recorded by RUNNING THE REFERENCE's own modules on the CPU (build machine only).

    python tests/golden/make_golden_small_graph.py

Builds the reference's two ST-GCN modules through _ref_import (neither needs a licensed asset: the 'openpose' and 'ntu-rgb+d' graphs are written out in
stgcnutils/graph.py), loads synthetic checkpoints of regennet_amd.synth into them (strict) and writes DATA only:

  small_graph_uncond.npz   eval/unconstrained/models/stgcn.py::STGCN, layout 'openpose' (15 nodes), 3 channels, 12 classes, six blocks
  small_graph_ntu25.npz    eval/a2m/recognition/models/stgcn.py::STGCN, layout 'ntu-rgb+d' (25 nodes), two persons, 12 channels, ten blocks
  small_graph_keys.json    state_dict key names and shapes of both modules

Each npz holds the module's own adjacency buffer `A`, the checkpoint's digest (tests/helpers.sd_digest), the inputs and the module's features / yhat."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
from regennet_amd import synth  # noqa: E402
from tests.helpers import sd_digest  # noqa: E402

SIX = [(64, 1), (64, 1), (64, 1), (128, 2), (128, 1), (256, 2)]
UNCOND_INPUTS = {"a": (5, 15, 3, 60), "short": (2, 15, 3, 7), "one": (1, 15, 3, 24)}
NTU25_INPUTS = {"a": (3, 25, 12, 24), "one": (1, 25, 12, 60)}


def record(model, key, shapes, seed, **sd_kw):
    A = model.A.numpy().copy()
    sd = synth.make_stgcn_state_dict(A, seed=seed, **sd_kw)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    assert not missing and not unexpected
    model.eval()
    out = {"A": A, "sd_digest": np.str_(sd_digest(sd)), "seed": np.int64(seed), "tags": np.array(sorted(shapes))}
    rng = np.random.Generator(np.random.PCG64(seed + 77))
    for tag, shape in shapes.items():
        x = rng.standard_normal(shape).astype(np.float32)
        with torch.no_grad():
            b = model({key: torch.from_numpy(x)})
        out[f"x_{tag}"], out[f"features_{tag}"], out[f"yhat_{tag}"] = x, b["features"].numpy().copy(), b["yhat"].numpy().copy()
        print(f"[{key} {tag}] x {shape} features {tuple(b['features'].shape)} max |f| {b['features'].abs().max():.3f} yhat {tuple(b['yhat'].shape)}", flush=True)
    return out, {k: list(v.shape) for k, v in model.state_dict().items()}


if __name__ == "__main__":
    _ref_import.install()
    from eval.a2m.recognition.models.stgcn import STGCN as RecSTGCN
    from eval.unconstrained.models.stgcn import STGCN as UncondSTGCN
    torch.manual_seed(0)
    un = UncondSTGCN(in_channels=3, num_class=12, graph_args={"layout": "openpose", "strategy": "spatial"}, edge_importance_weighting=True, device="cpu")
    o1, k1 = record(un, "x", UNCOND_INPUTS, 15, num_class=12, in_channels=3, num_person=1, blocks=SIX)
    np.savez_compressed(os.path.join(HERE, "small_graph_uncond.npz"), **o1)
    rec = RecSTGCN(in_channels=12, num_class=12, num_person=2, graph_args={"layout": "ntu-rgb+d", "strategy": "spatial"}, edge_importance_weighting=True, device="cpu")
    o2, k2 = record(rec, "output", NTU25_INPUTS, 25, num_class=12, in_channels=12, num_person=2)
    np.savez_compressed(os.path.join(HERE, "small_graph_ntu25.npz"), **o2)
    with open(os.path.join(HERE, "small_graph_keys.json"), "w") as f:
        json.dump({"unconstrained": k1, "recognition_ntu25": k2}, f, indent=1, sort_keys=True)
        f.write("\n")
