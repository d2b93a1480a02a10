"""GPU: every fused kernel of the ST-GCN recogniser - k_sg_gcn, k_sg_tconv, k_sg_tconv_pre, k_sg_tconv_s2, split-bf16 and fp16 - and the row-shifted
GEMM launch_gemm_x3_sg against the fp64 host
statement of ITS OWN arithmetic (tests/sg_stage_ref.py), one launch at a time, row by row, before any pool.

The kernels are driven through their launch_* functions by the stand-alone program tests/sg_stage_check.hip (one process per kernel family, built once
per module): planes in, planes out, every element outside the rows a launch covers still holding its fill. The bounds - max and rms of
u = |got - ref| / (2^-24 S) for the split form; share, max and rms in fp16 ulps for the fp16 form - come from the host model alone
(tests/sg_stage_cases.py; tests/test_sg_stage_cpu.py shows that they tell the mutants apart). The walk cases assert that the launch had more than twice
as many tiles as the device has CUs.

Measured (profiles/sg_stage_parity.txt): all 93 cases inside their bounds. Every split-form kernel sits at 0.50 - 0.55 of its bound: its max u equals the
kernels'-text member's (x3) to the digit, because the largest deviation from the real operation is the deterministic one - the al . wl product that is never
formed and the output split. The fp16 kernels sit at 0.39 - 0.80; the closest is s2_128x256_v56_T9_f16 (max 16 ulp against 20).

A process that times out, dies of a signal or reports a HIP error fails its cases and stops the module: no later case starts another GPU process."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import sg_stage_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "regennet_amd", "csrc")
KERNEL_SOURCES = ["rgn_sg_kernels.hip", "rgn_gemm_x3.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden"]   # build()'s (-ffp-contract=off among them)
_STOP = []       # the reason the module stopped starting GPU processes
_RESULTS = {}    # kernel -> {case: (ndarray, cus, tiles)} | the text of what went wrong


def _hipcc():
    cand = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return cand if os.path.exists(cand) else shutil.which("hipcc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/sg_stage_check.hip, linked with the kernel objects build() left under build/obj where they are fresh (else those sources are compiled here)."""
    from concurrent.futures import ThreadPoolExecutor
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("sg_stage_check")

    def compile_one(src, obj):
        p = subprocess.run([hipcc] + FLAGS + ["-I", CSRC, "-c", src, "-o", obj], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-4000:]
        return obj

    todo, objs = [(os.path.join(ROOT, "tests", "sg_stage_check.hip"), str(out / "sg_stage_check.o"))], []
    for s in KERNEL_SOURCES:
        built = os.path.join(ROOT, "build", "obj", s + ".o")
        stale = not os.path.exists(built) or os.path.getmtime(built) < max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith(".h") or f == s)
        if stale:
            todo.append((os.path.join(CSRC, s), str(out / (s + ".o"))))
        else:
            objs.append(built)
    with ThreadPoolExecutor(max_workers=min(len(todo), 16)) as ex:
        objs += list(ex.map(lambda so: compile_one(*so), todo))
    exe = str(out / "sg_stage_check")
    p = subprocess.run([hipcc] + FLAGS + objs + ["-o", exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return exe, out


def _run_kernel(kernel, checker):
    """ONE process for all cases of the kernel family; its outputs, or the text of the failure."""
    if kernel in _RESULTS:
        return _RESULTS[kernel]
    if _STOP:
        return "not started: " + _STOP[0]
    exe, out = checker
    d = out / kernel
    d.mkdir()
    C.write_inputs(kernel, str(d))
    try:
        p = subprocess.run([exe, kernel, str(d)], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _STOP.append(f"sg_stage_check {kernel} did not finish in 120 s")
        _RESULTS[kernel] = _STOP[0]
        return _RESULTS[kernel]
    if p.returncode != 0:
        text = f"sg_stage_check {kernel} ended with status {p.returncode}: {(p.stdout + p.stderr)[-2000:]}"
        if p.returncode < 0 or "HIP error" in p.stderr:
            _STOP.append(text)
        _RESULTS[kernel] = text
        return text
    ran = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^(\S+): ran, cus (\d+) tiles (\d+)$", p.stdout, re.M)}
    _RESULTS[kernel] = {c["name"]: (C.read_output(c["name"], str(d)),) + ran[c["name"]] for c in C.cases_of(kernel)}
    shutil.rmtree(str(d), ignore_errors=True)
    return _RESULTS[kernel]


@pytest.mark.parametrize("name", [c["name"] for k in C.KERNELS for c in C.cases_of(k)])
def test_kernel_is_its_host_statement(name, checker):
    """every statistic of (kernel output - fp64 host evaluation) over the real rows within the case's host-derived bounds."""
    res = _run_kernel(C.BY_NAME[name]["kernel"], checker)
    assert isinstance(res, dict), res
    (got, cus, tiles), ref, bd = res[name], C.reference(name), C.bounds(name)
    assert got.shape == ref.shape and np.isfinite(got).all(), "an element the kernel must write still holds the fill pattern"
    assert tiles == C.tiles(name), (tiles, C.tiles(name))
    if C.is_walk(C.BY_NAME[name]):
        print(f"{name}: {tiles} tiles on {cus} CUs")
        assert tiles > 2 * cus, (tiles, cus)
    st = C.stats(name, got)
    print(f"{name:44s} kernel {C.fmt_stats(st)} | bound {C.fmt_stats(bd)} | x {C.violation(st, bd):.2f}")
    assert all(s <= b for s, b in zip(st, bd)), (st, bd)
