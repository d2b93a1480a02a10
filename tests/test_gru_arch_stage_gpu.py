"""GPU: the layer stack of the GRU denoiser alone (rgn_gru_stack.hip: k_gru_stack, one launch per anti-diagonal of (layer, step) cells) against the fp64
host statement tests/gru_arch_ref.py: gru_stack, one scan per case, driven through launch_gru_stack by the stand-alone program
tests/gru_arch_stage_check.hip (ONE process for all cases, built once per module).

The cases (tests/gru_arch_stage_cases.py): N in {1, 15, 16, 17, 33}, S in {1, 2, 3, L, L + 5} for L in {1, 2, 3, 8}, d in {16, 64, 512}, both stride
orders, 1 and 2 segments. The program itself ends with an error when an output element outside the covered rows lost its fill, when a covered one kept
it, or when NaN in the padding sequences and in the unwritten state ring changed a single output bit; with the ring full of NaN, a state slot read before
its launch wrote it (an off-by-one in the ring's parity) or a step-0 cell that multiplied the unwritten state comes back as NaN. Here every case is held
to max(8 x the fp32 error of the host statement on that case, 2^-20), the project's rule for the GRU kernels; the share of the bound each case uses is
printed (profiles/gru_arch_parity.txt).

A process that times out, dies of a signal or reports a HIP error fails every case: nothing else is started."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import gru_arch_stage_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "regennet_amd", "csrc")
KERNEL_SOURCES = ["rgn_gru_stack.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden"]   # build()'s


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    """{case: ndarray} from one run of the checker over all cases, or the text of what went wrong."""
    cand = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    hipcc = cand if os.path.exists(cand) else shutil.which("hipcc")
    if hipcc is None:
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("gru_arch_stage_check")
    objs = []
    for src in [os.path.join(ROOT, "tests", "gru_arch_stage_check.hip")] + [os.path.join(CSRC, s) for s in KERNEL_SOURCES]:
        built = os.path.join(ROOT, "build", "obj", os.path.basename(src) + ".o")
        fresh = src.startswith(CSRC) and os.path.exists(built) and os.path.getmtime(built) >= max(
            os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith(".h") or f == os.path.basename(src))
        if fresh:
            objs.append(built)
            continue
        obj = str(out / (os.path.basename(src) + ".o"))
        p = subprocess.run([hipcc] + FLAGS + ["-I", CSRC, "-c", src, "-o", obj], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-4000:]
        objs.append(obj)
    exe = str(out / "gru_arch_stage_check")
    p = subprocess.run([hipcc] + FLAGS + objs + ["-o", exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    d = out / "cases"
    d.mkdir()
    C.write_inputs(str(d))
    try:
        p = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        return "gru_arch_stage_check did not finish in 120 s"
    if p.returncode != 0:
        return f"gru_arch_stage_check ended with status {p.returncode}: {(p.stdout + p.stderr)[-2000:]}"
    ran = {line.split(":")[0]: int(line.rsplit(" ", 1)[1]) for line in p.stdout.splitlines() if ": ran, launches " in line}
    res = {c["name"]: (C.read_output(c, str(d)), ran[c["name"]]) for c in C.CASES}
    shutil.rmtree(str(d), ignore_errors=True)
    return res


@pytest.mark.parametrize("name", [c["name"] for c in C.CASES])
def test_stack_is_its_host_statement(name, outputs):
    assert isinstance(outputs, dict), outputs
    c = C.BY_NAME[name]
    got, launches = outputs[name]
    ref, bd = C.bound(c)
    assert launches == c["S"] + c["L"] - 1
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"\n[gru stage] {name:28s} err {err:.3e}  bound {bd:.3e}  share {err / bd:.3f}")
    assert err <= bd, (name, err, bd)
