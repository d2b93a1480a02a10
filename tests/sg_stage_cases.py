"""The cases of the recogniser's stage tests (test_sg_stage_cpu.py, test_sg_stage_gpu.py): shapes, inputs, the host evaluation, the bounds and the
mutants. Everything is derived from sg_stage_ref.py; no figure here comes from a kernel.

Shapes: the smallest at which each kernel can still go wrong. Every case with taps has NM = 3 sequences (sequence boundaries inside tiles), T >= 9 (the
first and last four frames see zeros, not the neighbour), (T + 4) V no multiple of the tile height (tile and window edges mid-frame and mid-sequence).
Activations are relu-like - half of them zero - with a few large entries; the pad VERTEX rows of a small graph hold +5 on input. Weights are seeded
Gaussians of the checkpoint's scale, every 16-bit operand representable (a hi + lo pair, or fp16). The WALK cases run the narrowest channel count over
more than 512 tiles - more than twice the CUs of the device, which the GPU test asserts from the driver's print - with the reference on ALL rows.

Bounds. Split form: u = |got - ref| / (2^-24 S) elementwise, S = sum |a| |w| + |bias| + |residual| in float64; the statistics are max u
and rms u over the real rows. fp16 form: the share of elements that differ from rne16(statement), the max and the rms difference in fp16 ulps. The
bound of a case is TWICE the worst statistic among the fp32 members of its family (sg_stage_ref: p8, p8r, p16, and x3 for the split form). A mutant
counts as detected when it violates one bound by a factor >= 1.5.
"""
import functools
import os
import zlib

import numpy as np

from tests import sg_stage_ref as R

FACTOR, DETECT = 2.0, 1.5
KERNELS = ("gcn", "tconv", "tconv_pre", "tconv_s2", "x3_sg")
HERE = os.path.dirname(os.path.abspath(__file__))
NM = 3


def _gcn(name, V, ci, co, bn, graph, fmt, cap=256, pbb=0, nm=NM, T=5):
    return dict(kernel="gcn", name=f"gcn_{name}_{fmt}", V=V, ci=ci, co=co, BN=bn, graph=graph, fmt=fmt, cap=cap, pbb=pbb, NM=nm, T=T)


def _tc(shape, V, N, tail, T, fmt, small=0, nm=NM, tag=""):
    bm, bn = shape
    return dict(kernel="tconv", name=f"tconv_{bm}x{bn}_t{tail}_v{V}_T{T}{tag}_{fmt}", V=V, N=N, tail=tail, T=T, fmt=fmt, small=small, BM=bm, BN=bn, NM=nm)


def _pre(V, N, tail, T, nm=NM, tag=""):
    return dict(kernel="tconv_pre", name=f"pre_n{N}_t{tail}_v{V}_T{T}{tag}_split", V=V, N=N, tail=tail, T=T, fmt="split", small=0, BM=256,
                BN=128 if (N != 64 and tail != 3) else 64, NM=nm)


def _s2(V, ci, co, T, fmt, nm=NM, tag=""):
    return dict(kernel="tconv_s2", name=f"s2_{ci}x{co}_v{V}_T{T}{tag}_{fmt}", V=V, ci=ci, N=co, T=T, fmt=fmt, NM=nm)


def _all():
    out = []
    # ---- k_sg_gcn: C_in -> C_out, tile width (cap = widest_tile), the 64-wide kernel with one barrier per channel block (default) or per k-block (pbb);
    # V = 16, 20: the padded planes of 15- and 18-vertex graphs (bias period 32, 40). fp16 only for V >= 32 (the engine refuses it below)
    for fmt in ("split", "f16"):
        out += [_gcn("v56_64x64", 56, 64, 64, 64, "golden", fmt),
                _gcn("v56_64x64_pbb", 56, 64, 64, 64, "golden", fmt, pbb=1),
                _gcn("v56_64x128", 56, 64, 128, 128, "golden", fmt),
                _gcn("v56_128x256", 56, 128, 256, 256, "golden", fmt),
                _gcn("v56_256x256", 56, 256, 256, 256, "golden", fmt),
                _gcn("v36_64x64_tree", 36, 64, 64, 64, "tree", fmt),
                _gcn("v64_128x256_tree", 64, 128, 256, 128, "tree", fmt)]          # (V = 64: a 256-wide tile does not fit 160 KiB)
    out += [_gcn("v56_64x128_cap64", 56, 64, 128, 64, "golden", "split", cap=64),   # two 64-wide column tiles
            _gcn("v56_256x256_cap128", 56, 256, 256, 128, "golden", "split", cap=128),
            _gcn("v56_64x64_tree", 56, 64, 64, 64, "tree", "split"),
            _gcn("v15_64x64_tree", 15, 64, 64, 64, "tree", "split"),
            _gcn("v18_64x128_tree", 18, 64, 128, 128, "tree", "split"),
            _gcn("v15_256x256_tree", 15, 256, 256, 256, "tree", "split", pbb=1),
            _gcn("walk_v56_64x64", 56, 64, 64, 64, "golden", "split", nm=37, T=60)]   # 37 x 64 x 56 rows = 518 tiles
    # ---- k_sg_tconv: five tile shapes x tails 0 - 3 (tail 0 split only) x arithmetic. 512-row tiles: V % 8 == 0; 256 x 64 / 256 x 128: V = 36, or
    # small_tiles. Tail 3: both parities of T and of ceil(T / 2) (T = 9: odd, odd; 10: even, odd; 11: odd, even; 12: even, even)
    shapes = [((512, 64), 64, (56, 32, 64, 56), 0), ((512, 128), 128, (64, 56, 32, 56), 0), ((256, 256), 256, (56, 36, 64, 32), 0),
              ((256, 64), 64, (36, 56, 36, 64), None), ((256, 128), 128, (36, 64, 36, 56), None)]
    poly_T = (9, 10, 11, 12, 11)
    for si, (shape, N, Vs, small) in enumerate(shapes):
        for tail in range(4):
            V = Vs[tail]
            sm = (0 if V == 36 else 1) if small is None else small
            T = poly_T[si] if tail == 3 else (9, 13)[(si + tail) % 2]
            if tail == 3 and T == 12 and V in (32, 64):
                V = 56
            out.append(_tc(shape, V, N, tail, T, "split", sm))
            if tail:
                Tf = poly_T[(si + 2) % 5] if tail == 3 else (13, 9)[(si + tail) % 2]
                Vf = Vs[(tail + 1) % 4]
                smf = (0 if Vf == 36 else 1) if small is None else small
                if tail == 3 and Tf == 12 and Vf in (32, 64):
                    Vf = 56
                out.append(_tc(shape, Vf, N, tail, Tf, "f16", smf))
    out.append(_tc((256, 128), 56, 256, 2, 9, "split", 1, tag="_n256"))            # 256 channels as two 128-wide column tiles (small_tiles)
    out.append(_tc((256, 64), 36, 64, 2, 60, "split", 0, nm=58, tag="_walk"))     # 58 x 64 x 36 rows = 522 tiles
    # ---- k_sg_tconv_pre: V in {16, 20, 24, 28} x N in {64, 128, 256} (256: two column tiles), tails 0 - 3 (tail 3: the two-step frame walk, 64-wide tiles)
    out += [_pre(16, 64, 0, 9), _pre(20, 64, 1, 13), _pre(24, 64, 2, 9), _pre(28, 64, 3, 9), _pre(16, 64, 3, 10), _pre(20, 64, 3, 11), _pre(24, 64, 3, 12),
            _pre(20, 128, 0, 13), _pre(24, 128, 1, 9), _pre(28, 128, 2, 13), _pre(16, 128, 3, 11), _pre(28, 128, 3, 10),
            _pre(24, 256, 0, 9), _pre(28, 256, 1, 9), _pre(16, 256, 2, 13), _pre(20, 256, 3, 9),
            _pre(20, 64, 2, 60, nm=103, tag="_walk")]                              # 103 x 64 x 20 rows = 515 tiles
    # ---- k_sg_tconv_s2: 64 -> 128 (k2 = 2) and 128 -> 256 (k2 = 4), T odd and even (regions E and O differ in real frames when T is odd)
    out += [_s2(16, 64, 128, 9, "split"), _s2(36, 64, 128, 10, "split"), _s2(56, 64, 128, 9, "split"),
            _s2(16, 128, 256, 10, "split"), _s2(36, 128, 256, 9, "split"), _s2(56, 128, 256, 10, "split"),
            _s2(36, 64, 128, 9, "f16"), _s2(56, 64, 128, 10, "f16"), _s2(36, 128, 256, 10, "f16"), _s2(56, 128, 256, 9, "f16"),
            _s2(36, 64, 128, 60, "split", nm=108, tag="_walk")]                    # 108 x 34 x 36 rows = 517 tiles
    # ---- launch_gemm_x3_sg at V = 30, where the window kernels do not apply (V % 4) and it is the default: the row-shifted 9-tap GEMM in its narrow (256 x 64,
    # four waves) and wide (256 x 128) form, its stride-2 tap table, and the (row % add_mod) addend with ReLU - the GEMM of the two-launch graph convolution
    x3 = lambda tag, kind, N, T, K=0: dict(kernel="x3_sg", name=f"x3_{tag}_v30_n{N}_T{T}_split", kind=kind, V=30, N=N, K=K, T=T, fmt="split", NM=NM, BM=256, BN=64 if N <= 64 else 128)   # noqa: E731
    out += [x3("taps", 0, 64, 9), x3("taps", 0, 128, 13), x3("taps", 0, 256, 9), x3("s2taps", 1, 128, 9), x3("s2taps", 1, 64, 10), x3("addmod", 2, 64, 5, K=192), x3("addmod", 2, 128, 5, K=192)]
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return out


CASES = _all()
BY_NAME = {c["name"]: c for c in CASES}


def cases_of(kernel):
    return [c for c in CASES if c["kernel"] == kernel]


def is_walk(c):
    return "walk" in c["name"]


def _rng(name, salt=""):
    return np.random.Generator(np.random.PCG64(zlib.crc32((name + salt).encode())))


def _fmt(a, fmt):
    """the nearest values the case's operand format holds, float64."""
    return R.f16(a) if fmt == "f16" else R.splittable(a).astype(np.float64)


def _relu_like(rng, shape, fmt):
    """half zero, half |N(0, 1)|, one entry in 200 thirty times as large."""
    a = np.maximum(rng.standard_normal(shape), 0.0)
    a = a * np.where(rng.random(shape) < 0.005, 30.0, 1.0)
    return _fmt(a, fmt)


def _weights(rng, shape, fan_in, fmt, gain=1.5):
    return _fmt(rng.standard_normal(shape) * (gain / np.sqrt(fan_in)), fmt)


def _tree8(V):
    """a skeleton whose longest lists are 1 / 1 / 6 - all eight slots: vertex 0 has six children, the rest hang in a binary tree below them."""
    parent = np.zeros(V, np.int64)
    for v in range(7, V):
        parent[v] = (v - 7) // 2 + 1
    adj = np.eye(V)
    for v in range(1, V):
        adj[v, parent[v]] = adj[parent[v], v] = 1.0
    dn = adj / adj.sum(0, keepdims=True)
    A = np.zeros((3, V, V), np.float32)
    for v in range(V):
        for w in range(V):
            if adj[v, w]:
                A[0 if v == w else (1 if parent[w] == v else 2), v, w] = dn[v, w]
    return A


@functools.lru_cache(maxsize=None)
def _graph(kind, V):
    """A' = A . edge_importance (fp32 product) on the plane's Vp vertices: the golden graph (longest lists 1 / 6 / 1) or the eight-slot tree."""
    A = np.load(os.path.join(HERE, "golden", "stgcn.npz"))["A"].astype(np.float32) if kind == "golden" else _tree8(V)
    assert A.shape[1] == V
    imp = (1.0 + 0.3 * _rng(f"imp_{kind}_{V}").standard_normal(A.shape)).astype(np.float32)
    Vp = R.padded_nodes(V)
    Ap = np.zeros((A.shape[0], Vp, Vp))
    Ap[:, :V, :V] = (A * imp).astype(np.float64)
    return Ap


@functools.lru_cache(maxsize=3)
def stage(name):
    """name -> the case's Stage (sg_stage_ref) on the case's inputs."""
    c = BY_NAME[name]
    fmt, rng, k, fp16 = c["fmt"], _rng(name), c["kernel"], c["fmt"] == "f16"
    if k == "gcn":
        V, Vp, P = c["V"], R.padded_nodes(c["V"]), R.bias_period(c["V"])
        geo = R.Geo(c["NM"], c["T"], Vp)
        A = _graph(c["graph"], V)
        seq = _relu_like(rng, (c["NM"], c["T"], Vp, c["ci"]), fmt)
        seq[:, :, V:] = 5.0                                                           # pad vertex rows: nothing may read them
        W1 = _weights(rng, (c["co"], A.shape[0] * c["ci"]), c["ci"], fmt)
        b1 = np.zeros((P, c["co"]))
        bv = (0.3 * rng.standard_normal((V, c["co"]))).astype(np.float32).astype(np.float64)
        for r in range(P):
            if r % Vp < V:
                b1[r] = bv[r % Vp]
        return R.GcnStage(geo.plane(seq), geo, A, W1, b1, fp16)
    if k in ("tconv", "tconv_pre"):
        V, N = c["V"], c["N"]
        geo = R.Geo(c["NM"], c["T"], V)
        gseq = _relu_like(rng, (c["NM"], c["T"], V, N), fmt)
        xres = None
        if k == "tconv_pre":
            gseq[:, :, V - 1] = 5.0                                                   # the last vertex row as a pad vertex's
        if c["tail"] >= 2:
            xres = geo.plane(_relu_like(rng, (c["NM"], c["T"], V, N), fmt))
        W2 = _weights(rng, (N, N, 9), 9 * N, fmt)
        b2 = (0.3 * rng.standard_normal(N)).astype(np.float32).astype(np.float64)
        return R.TconvStage(geo.plane(gseq), geo, W2, b2, c["tail"], xres, fp16)
    if k == "x3_sg":
        V, N = c["V"], c["N"]
        if c["kind"] == 2:
            geo = R.Geo(c["NM"], c["T"], V)
            z = geo.plane(_relu_like(rng, (c["NM"], c["T"], V, c["K"]), fmt))
            b1 = (0.3 * rng.standard_normal((V, N))).astype(np.float32).astype(np.float64)
            return R.GemmStage(z, geo, _weights(rng, (N, c["K"]), c["K"] // 3, fmt), b1)
        geo = R.Geo(c["NM"], c["T"], V, poly=c["kind"] == 1)
        g = geo.plane(_relu_like(rng, (c["NM"], c["T"], V, N), fmt))
        W2 = _weights(rng, (N, N, 9), 9 * N, fmt)
        if c["kind"] == 1:
            return R.TconvS2Stage(g, None, geo, W2, None, None, conv_only=True)
        return R.TconvStage(g, geo, W2, np.zeros(N), 0)
    V, N, ci = c["V"], c["N"], c["ci"]
    geo = R.Geo(c["NM"], c["T"], V, poly=True)
    g = geo.plane(_relu_like(rng, (c["NM"], c["T"], V, N), fmt))
    x = geo.plane(_relu_like(rng, (c["NM"], c["T"], V, ci), fmt))
    W2 = _weights(rng, (N, N, 9), 9 * N, fmt)
    Wr = _weights(rng, (N, ci), ci, fmt, gain=1.0)
    b = (0.3 * rng.standard_normal(N)).astype(np.float32).astype(np.float64)
    return R.TconvS2Stage(g, x, geo, W2, Wr, b, fp16)


def real_rows(name):
    """the rows of evaluate()'s result that hold real frames, in (sequence, frame, vertex) order."""
    st = stage(name)
    return (st.out_geo if isinstance(st, R.TconvS2Stage) else st.geo).real_rows()


def evaluate(name, mode="f64", mut=None):
    """the case's stage in `mode` -> float64 [real rows, N]."""
    c = BY_NAME[name]
    y = stage(name).evaluate(mode, mut)[real_rows(name)]
    if mut == "poly_parity":   # the last frame of an odd T stored into the other region: its rows of region E are never written
        assert c["tail"] == 3 and c["T"] % 2 == 1
        y = y.reshape(c["NM"], c["T"], c["V"], -1).copy()
        y[:, c["T"] - 1] = np.nan
        y = y.reshape(-1, y.shape[-1])
    return y


@functools.lru_cache(maxsize=None)
def _reference(name):
    ref = evaluate(name)
    S = None if BY_NAME[name]["fmt"] == "f16" else stage(name).S()[real_rows(name)]
    ref.setflags(write=False)
    return ref, S


def reference(name):
    return _reference(name)[0]


def stats(name, got):
    """the case's statistics of `got` [real rows, N] against the statement."""
    ref, S = _reference(name)
    got = np.where(np.isnan(got), np.inf, got)
    return R.stats_f16(got, ref) if S is None else R.stats_split(got, ref, S)


def modes(name):
    return R.F16_MODES if BY_NAME[name]["fmt"] == "f16" else R.SPLIT_MODES


@functools.lru_cache(maxsize=None)
def family(name):
    return tuple(stats(name, evaluate(name, m)) for m in modes(name))


@functools.lru_cache(maxsize=None)
def bounds(name):
    fam = family(name)
    return tuple(FACTOR * max(f[i] for f in fam) for i in range(len(fam[0])))


def violation(st, bd):
    return max((s / b if b > 0 else (float("inf") if s > 0 else 0.0)) for s, b in zip(st, bd))


def fmt_stats(st):
    if len(st) == 2:
        return f"max u {st[0]:10.2f}  rms u {st[1]:9.3f}"
    return f"share {100 * st[0]:7.3f} %  max {st[1]:9.1f} ulp  rms {st[2]:9.4f} ulp"


def mutants(name):
    """the host-side variations of the statement the case's bounds must tell from it (sg_stage_ref.Stage.evaluate's `mut`)."""
    c = BY_NAME[name]
    k, split = c["kernel"], c["fmt"] == "split"
    m = ["kblock_last", "row_zero"]
    if split:
        m += ["drop_alwh", "drop_ahwl"]
    if k == "x3_sg":
        return m + (["no_relu", "out_lo_zero", "bias_neighbour"] if c["kind"] == 2 else ["tap_edge", "pads_neighbour"])
    if k == "gcn":
        m += ["no_relu", "slot_dropped"] + (["out_lo_zero"] if split else ["agg_fp32", "coef_unrounded"])
        if R.bias_period(c["V"]) % 32:          # (a period that is a multiple of 32 - P = 32, 64 - wraps only where a 32-row tile starts: nothing to get wrong)
            m += ["bias_neighbour"]
    elif k == "tconv_s2":
        m += ["no_relu", "tap_edge", "pads_neighbour", "shortcut_dropped"] + (["out_lo_zero"] if split else [])
    else:
        m += ["tap_edge", "pads_neighbour"]
        if c["tail"]:
            m += ["no_relu"] + (["out_lo_zero"] if split else [])
        if c["tail"] >= 2:
            m += ["resid_hi"] if split else []      # (an fp16 residual has one plane: there is no lo to lose)
        if c["tail"] == 3 and c["T"] % 2:
            m += ["poly_parity"]
    return m


# ---- the files tests/sg_stage_check.hip reads (the fields of a case line stand above its run_* functions) -------------------------------------------------
def _dump(path, a):
    np.ascontiguousarray(a, dtype="<f4").tofile(path)


def write_inputs(kernel, directory, names=None):
    """<directory>/<kernel>.cases + every tensor of the kernel's cases (or of `names`)."""
    lines = []
    for c in cases_of(kernel):
        name = c["name"]
        if names is not None and name not in names:
            continue
        st, f = stage(name), int(c["fmt"] == "f16")
        p = lambda t: os.path.join(directory, f"{name}.{t}.f32")   # noqa: E731
        if kernel == "gcn":
            slot_k, sv, sa = st.slot_tables()
            _dump(p("x"), st.x), _dump(p("W1"), st.W1), _dump(p("b1"), st.b1), _dump(p("slv"), sv), _dump(p("sla"), sa)
            lines.append(f"{name} {f} {st.V} {st.M} {st.C} {c['co']} {st.K} {st.b1.shape[0]} {c['cap']} {c['pbb']} {slot_k} {c['BN']}")
        elif kernel == "x3_sg":
            if c["kind"] == 2:
                _dump(p("z"), st.z), _dump(p("W"), st.W), _dump(p("b1"), st.b1)
            else:
                _dump(p("g"), st.g), _dump(p("W2"), st.W2)
            lines.append(f"{name} {c['kind']} {c['V']} {st.M} {c['N']} {c['K']}")
        elif kernel in ("tconv", "tconv_pre"):
            _dump(p("g"), st.g), _dump(p("W2"), st.W2), _dump(p("b2"), st.b2)
            if st.xres is not None:
                _dump(p("R"), st.xres)
            region = R.Geo(c["NM"], c["T"], c["V"], poly=True).region
            lines.append(f"{name} {f} {c['V']} {st.M} {c['N']} {c['tail']} {c['small']} {int(kernel == 'tconv_pre')} {c['BM']} {c['BN']} {c['T']} {region}")
        else:
            _dump(p("g"), st.g), _dump(p("x"), st.x), _dump(p("W2"), st.W2), _dump(p("Wr"), st.Wr), _dump(p("b"), st.bias)
            lines.append(f"{name} {f} {c['V']} {st.M} {c['N']} {c['ci']}")
    with open(os.path.join(directory, kernel + ".cases"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


def read_output(name, directory):
    """the driver's output of a case -> float64 [real rows, N] (hi + lo; an element still holding the fill: NaN)."""
    c, st = BY_NAME[name], stage(name)
    N = c["co"] if c["kernel"] == "gcn" else c["N"]
    parts = [np.fromfile(os.path.join(directory, f"{name}.out_hi.f32"), dtype="<f4").astype(np.float64).reshape(-1, N)]
    if st.out_fmt == "split":
        parts.append(np.fromfile(os.path.join(directory, f"{name}.out_lo.f32"), dtype="<f4").astype(np.float64).reshape(-1, N))
    body = sum(parts)
    if c["kernel"] != "gcn" and c.get("tail") == 3:   # stored polyphase: the real rows of the two-region plane
        return body[R.Geo(c["NM"], c["T"], c["V"], poly=True).real_rows()]
    return body[real_rows(name)]


def tiles(name):
    c, st = BY_NAME[name], stage(name)
    if c["kernel"] == "gcn":
        return -(-c["co"] // c["BN"]) * -(-st.M // 256)
    if c["kernel"] == "tconv_s2":
        return (c["N"] // 128) * -(-st.M // 256)
    return -(-c["N"] // c["BN"]) * -(-st.M // c["BM"])
