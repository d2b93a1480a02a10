"""Golden vectors of the GRU action classifier, recorded by RUNNING THE REFERENCE's own modules on the CPU (build machine only).

    python tests/golden/make_golden_gru.py

Imports the reference's eval/a2m/action2motion/models.py through _ref_import, loads the synthetic checkpoints of regennet_amd.synth.make_gru_state_dict
into MotionDiscriminator and MotionDiscriminatorForFID (strict) and runs them with an explicit hidden_unit. Writes DATA only, one gru_<case>.npz per
case of tests/gru_ref.CASES: the reference's `features` and `logits` (fp32), `lengths`, the seeds, `ref_err` = max |reference fp32 - fp64 restatement|
per output (features, logits), and `min_gap`, the smallest top-2 logit gap in fp64 (asserted >= 1e-4, so a device test may demand argmax equality on
every row). Inputs and weights are NOT stored: tests regenerate them from the seeds (tests/gru_ref.case_inputs). gru_keys.json records the key names and
shapes of the reference module's state dict at the HumanAct12 geometry."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
from tests import gru_ref  # noqa: E402


def main():
    _ref_import.install()
    from eval.a2m.action2motion import models as ref_models

    torch.set_num_threads(1)
    for name, (I, H, L, C, N, T, scale, _) in gru_ref.CASES.items():
        sd, x, lengths, h0 = gru_ref.case_inputs(name)
        tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
        outs = []
        for cls in (ref_models.MotionDiscriminatorForFID, ref_models.MotionDiscriminator):
            m = cls(I, H, L, device="cpu", output_size=C)
            m.load_state_dict(tsd, strict=True)
            m.eval()
            with torch.no_grad():
                outs.append(m(torch.from_numpy(x), lengths=torch.from_numpy(lengths), hidden_unit=torch.from_numpy(h0)).numpy())
            if name == "ha12" and cls is ref_models.MotionDiscriminator:
                keys = {k: list(v.shape) for k, v in m.state_dict().items()}
                with open(os.path.join(HERE, "gru_keys.json"), "w") as f:
                    json.dump(keys, f, indent=1, sort_keys=True)
        feats, logits = outs
        f64, l64 = gru_ref.gru_forward(sd, x, lengths, h0)
        ref_err = np.array([np.abs(feats - f64).max(), np.abs(logits - l64).max()])
        top = np.sort(l64, axis=1)
        min_gap = float((top[:, -1] - top[:, -2]).min())
        assert min_gap >= 1e-4, (name, min_gap)
        np.savez(os.path.join(HERE, f"gru_{name}.npz"), features=feats.astype(np.float32), logits=logits.astype(np.float32), lengths=lengths,
                 seed=np.int64(gru_ref.CASE_SEEDS[name]), ref_err=ref_err, min_gap=np.float64(min_gap))
        print(f"{name:9s} N {N:3d} T {T:3d}  ref_err features {ref_err[0]:.2e} logits {ref_err[1]:.2e}  min top-2 gap {min_gap:.2e}")


if __name__ == "__main__":
    main()
