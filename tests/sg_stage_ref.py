"""The arithmetic of the ST-GCN recogniser's fused kernels, stated once on the host: one stage per kernel, in the kernels' ROW GEOMETRY.

Rows are (sequence, frame, vertex). A PLANE here is a float64 array [G + rows + G, C] in natural channel order: G = 4 V guard rows at both ends, and behind
every sequence four zero PAD frames (which are also the pad in front of the next one). A POLYPHASE plane holds two regions of the same geometry back to
back - E, the even frames of every sequence, then O, the odd ones, ceil(T / 2) + 4 frames per sequence in both (rgn_stgcn.hip: rgn_stgcn_forward). The
temporal taps are then plain row shifts by multiples of V, and that is how they are written below: what a tap reads beyond a sequence is whatever the
plane holds there - zeros, if the pads are what k_sg_zero leaves.

    GcnStage      k_sg_gcn        relu(sum_k sum_c (sum_v A'_k[v, w] x[(f, v), c]) W1'[o, (k, c)] + b1'[row % P, o])
    TconvStage    k_sg_tconv, k_sg_tconv_pre   sum_dt g[row + (dt - 4) V] . W2'[:, :, dt] + b2'  (tail 0: fp32) | relu(...) (1) | relu(... + x) (2) | as 2, stored polyphase (3)
    TconvS2Stage  k_sg_tconv_s2   relu(sum_j gE[row + (j - 2) V] . W2'[:, :, 2 j] + sum_j gO[row + (j - 2) V] . W2'[:, :, 2 j + 1] + xE[row] . Wr' + (b2' + br'))

The fold is rgn_stgcn_finalize's, in float64 (fold): A' = A . edge_importance (an fp32 product, as the reference forms it), W1' = s1 Wg,
b1'[w] = s1 sum_k bg_k colsum_k[w] + t1, W2' = s2 Wt, b2' = s2 bt + t2, Wr' = sr Wr, br' = sr br + tr. forward_stages composes the stages over a block plan.

SPLIT-bf16 FORM. Operands are exact hi + lo pairs, accumulation is fp32, k_sg_gcn splits its aggregated sum once and every output is split once: there
is no 16-bit rounding site to model, and the statement (mode "f64") is the real operation. The fp32 MEMBERS of the family say how far a correct fp32
implementation may lie from it (the bounds are twice the worst of them, tests/sg_stage_cases.py):

    "p8", "p8r"   exact 8-deep partial products (formed in float64, rounded once to fp32), added one after the other to an fp32 accumulator; forward and reversed
    "p16"         16-deep partials, the MFMA's own step, in the kernel's k order
    "x3"          the kernels' text: per 16-deep step al . wh, then ah . wl, then ah . wh (rgn_dma_gemm.h dg_mma; al . wl is never formed), and for
                  k_sg_gcn the aggregated operand as the kernel forms it: an fp32 FMA chain over the slots, split into hi + lo
Every member ends as the kernels do: the addends in fp32 in sg_epilogue's order, ReLU, and the OUTPUT FORMAT (hi = bf16(r), lo = bf16(r - hi); fp32 for tail 0).

fp16 FORM (SG_F16). One IEEE fp16 plane per operand, one MFMA per product, fp32 accumulation, fp16 output. The rounding sites, from k_sg_gcn's F16 branch
(rgn_sg_kernels.hip) and sg_epilogue:
    1. k_sg_gcn: the slot coefficient, c16 = rne16(sl_a[w][s])                                    `const _Float16 c16 = (_Float16)sa[s]`
    2. k_sg_gcn: the aggregated operand is a chain of PACKED fp16 FMAs over the slots of partition k in slot order (= list order, source vertex ascending),
       starting from +0: z <- rne16(c16 . x[v_s] + z), one rounding per slot                      `zf[ks] = __builtin_elementwise_fma(cv, h, zf[ks])`
       (a slot whose coefficient is zero for every row of a wave is skipped: fma(0, x, z) = z, the same value)
    3. every kernel: the output, rne16(relu(acc + addends)), the addends added in fp32             sg_epilogue / dg_store_pair<true>
Between the sites the statement is evaluated in float64 (a product of two fp16 values is exact in fp32; only the order of the fp32 sums is free).
"""
import numpy as np

U24 = 2.0 ** -24
PAD = 4                    # zero frames behind every sequence (SG_PAD)
SPLIT_MODES = ("p8", "p8r", "p16", "x3")
F16_MODES = ("p8", "p8r", "p16")


# ---- number formats -------------------------------------------------------------------------------------------------------------------------------
def bf16(x):
    """float32 array -> the nearest bf16 (ties to even), as float32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (u & 0xFFFFFFFF).astype(np.uint32).view(np.float32).reshape(x.shape)


def split(x):
    """x -> (hi, lo) float64 with hi = bf16(fp32(x)), lo = bf16(fp32(x) - hi): the pair a split plane holds."""
    x32 = np.asarray(x).astype(np.float32)
    hi = bf16(x32)
    lo = bf16(x32 - hi)
    return hi.astype(np.float64), lo.astype(np.float64)


def splittable(x):
    """x -> float32 values v that ARE hi + lo pairs: split(v) = (hi, lo) with hi + lo == v."""
    v = np.asarray(x).astype(np.float32)
    for _ in range(4):
        hi, lo = split(v)
        w = (hi + lo).astype(np.float32)
        if np.array_equal(w, v):
            return v
        v = w
    hi, lo = split(v)
    bad = (hi + lo) != v.astype(np.float64)
    v = np.where(bad, hi.astype(np.float32), v)
    hi, lo = split(v)
    assert np.array_equal(hi + lo, v.astype(np.float64))
    return v


def f16(x):
    """float64 -> the nearest IEEE fp16 (ties to even; one rounding, straight from float64), as float64."""
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------------------
class Geo:
    """NM sequences of T frames of V plane vertices; poly: the two-region layout a stride-2 block reads."""

    def __init__(self, NM, T, V, poly=False):
        self.NM, self.T, self.V, self.poly = NM, T, V, poly
        self.Treg = (T + 1) // 2 if poly else T           # real frames per sequence of region E (of the plane, if plain)
        self.Tp = self.Treg + PAD                          # frames per sequence of the rows
        self.region = NM * self.Tp * V                     # rows of one region
        self.rows = self.region * (2 if poly else 1)
        self.G = PAD * V

    def row(self, n, t, v):
        """body row (0 = the first row behind the leading guard rows) of (sequence, frame, vertex); arrays broadcast."""
        if self.poly:
            return (t & 1) * self.region + (n * self.Tp + (t >> 1)) * self.V + v
        return (n * self.Tp + t) * self.V + v

    def real_rows(self):
        """the body rows of the real frames, in (sequence, frame, vertex) order."""
        n, t, v = np.meshgrid(np.arange(self.NM), np.arange(self.T), np.arange(self.V), indexing="ij")
        return self.row(n, t, v).reshape(-1)

    def plane(self, seq):
        """seq [NM, T, V, C] -> plane [G + rows + G, C] with zero pad frames and guard rows."""
        seq = np.asarray(seq, dtype=np.float64)
        assert seq.shape[:3] == (self.NM, self.T, self.V), (seq.shape, self.NM, self.T, self.V)
        p = np.zeros((self.rows + 2 * self.G, seq.shape[3]))
        p[self.G + self.real_rows()] = seq.reshape(-1, seq.shape[3])
        return p

    def seq(self, body):
        """body rows [rows, C] -> the real frames [NM, T, V, C]."""
        return body[self.real_rows()].reshape(self.NM, self.T, self.V, -1)

    def frame_of_row(self):
        """per row of ONE region: (sequence, frame of the region's Tp, vertex)."""
        r = np.arange(self.region)
        return r // (self.Tp * self.V), (r // self.V) % self.Tp, r % self.V


def with_neighbour_pads(plane, geo):
    """The mutant 'pad frames read the neighbouring sequence': pad frame j behind sequence n holds frame j of sequence n + 1 of the same region."""
    p = plane.copy()
    V, Tp = geo.V, geo.Tp
    for reg in range(2 if geo.poly else 1):
        base = geo.G + reg * geo.region
        for n in range(geo.NM - 1):
            dst = base + (n * Tp + Tp - PAD) * V
            src = base + (n + 1) * Tp * V
            p[dst:dst + PAD * V] = plane[src:src + PAD * V]
    return p


# ---- the contraction in its modes ----------------------------------------------------------------------------------------------------------------------
def _granules(blocks, pairs):
    """k-blocks [(a [M, 32 j], w [N, 32 j])] -> the 16-deep granules in the order the MFMAs run. Split form: k half 0, 1 of every k-block. fp16 form
    (pairs): a k-step holds two channel blocks A | B and runs A.0, B.0, A.1, B.1 (dg_mma<true> per k half)."""
    out = []
    for a, w in blocks:
        if pairs and a.shape[1] == 64:
            order = (0, 2, 1, 3)
        else:
            order = range(a.shape[1] // 16)
        assert a.shape[1] % 16 == 0
        for g in order:
            out.append((a[:, 16 * g:16 * g + 16], w[:, 16 * g:16 * g + 16]))
    return out


def contract(blocks, mode, pairs=False, drop=None):
    """sum over the k-blocks of a . w^T -> float64 [M, N] (holding fp32 values in the fp32 modes). drop: 'alwh' | 'ahwl', the mutant that never forms
    that cross product (mode f64)."""
    if mode == "f64":
        acc = 0.0
        for a, w in blocks:
            acc = acc + a @ w.T
            if drop:
                ah, al = split(a)
                wh, wl = split(w)
                acc = acc - (al @ wh.T if drop == "alwh" else ah @ wl.T)
        return acc
    gr = _granules(blocks, pairs)
    acc = np.zeros((gr[0][0].shape[0], gr[0][1].shape[0]), dtype=np.float32)
    if mode == "x3":
        for a, w in gr:
            ah, al = split(a)
            wh, wl = split(w)
            acc = acc + (al @ wh.T).astype(np.float32)
            acc = acc + (ah @ wl.T).astype(np.float32)
            acc = acc + (ah @ wh.T).astype(np.float32)
    elif mode == "p16":
        for a, w in gr:
            acc = acc + (a @ w.T).astype(np.float32)
    else:
        parts = [(a[:, h:h + 8], w[:, h:h + 8]) for a, w in gr for h in (0, 8)]
        if mode == "p8r":
            parts = [(a[:, ::-1], w[:, ::-1]) for a, w in reversed(parts)]
        else:
            assert mode == "p8", mode
        for a, w in parts:
            acc = acc + (a @ w.T).astype(np.float32)
    return acc.astype(np.float64)


def abs_sum(blocks):
    s = 0.0
    for a, w in blocks:
        s = s + np.abs(a) @ np.abs(w).T
    return s


# ---- stages ---------------------------------------------------------------------------------------------------------------------------------------------
class Stage:
    """out_fmt: 'split' | 'f16' | 'f32'. evaluate(mode, mut) -> float64 [M, N] in the stage's own row order (all the rows the launch covers)."""
    relu = True
    fp16 = False
    out_fmt = "split"

    def blocks(self, mode, mut):
        raise NotImplementedError

    def addends(self, mut):
        """(bias broadcastable to [M, N], residual [M, N] or None), float64 holding fp32 values."""
        raise NotImplementedError

    BLOCK_MUTANTS = ("kblock_last", "drop_alwh", "drop_ahwl", "slot_dropped", "tap_edge", "pads_neighbour", "shortcut_dropped", "agg_fp32", "coef_unrounded")

    def evaluate(self, mode="f64", mut=None):
        if mode == "f64" and mut not in self.BLOCK_MUTANTS and getattr(self, "_acc64", None) is not None:
            acc = self._acc64                                  # (the mutants of the epilogue share the statement's contraction)
        else:
            bl = self.blocks(mode, mut)
            if mut == "kblock_last":
                a, w = bl[-1]
                bl = bl[:-1] + ([(a[:, :-32], w[:, :-32])] if a.shape[1] > 32 else [])
            acc = contract(bl, mode, self.fp16, {"drop_alwh": "alwh", "drop_ahwl": "ahwl"}.get(mut))
            if mode == "f64" and mut not in self.BLOCK_MUTANTS:
                self._acc64 = acc
        bias, res = self.addends(mut)
        if mode == "f64":
            r = acc + bias + (0.0 if res is None else res)
        else:   # sg_epilogue: (acc + bias) + residual, every addition rounded to fp32
            r = (acc.astype(np.float32) + f32(bias))
            if res is not None:
                r = r + f32(res)
            r = r.astype(np.float64)
        if self.relu and mut != "no_relu":
            r = np.maximum(r, 0.0)
        if mut == "row_zero":
            r = r.copy()
            r[self.victim_row()] = 0.0
        if self.out_fmt == "f16":
            return f16(r)
        if mode == "f64" and mut != "out_lo_zero":
            return r
        if self.out_fmt == "f32":
            return f32(r).astype(np.float64)
        hi, lo = split(r)
        return hi if mut == "out_lo_zero" else hi + lo

    def S(self):
        """sum |a| |w| over the element's products + |bias| + |residual|, float64 [M, N]."""
        bias, res = self.addends(None)
        return self.abs_products() + np.abs(bias) + (0.0 if res is None else np.abs(res))

    def abs_products(self):
        return abs_sum(self.blocks("f64", None))

    def victim_row(self):
        """'one row of a tile's last wave zero': of the last 32 rows of a 256-row tile - the second tile first, then the others - that hold a real row, the
        real row whose statement has the most nonzero elements."""
        ref, real = self.evaluate(), self.real_mask()
        M = ref.shape[0]
        starts = []
        for wave in range(7, -1, -1):                        # (where every last wave holds pad frames only: the wave in front of it, and so on)
            s = list(range(32 * wave, M, 256))
            starts += s[1:] + s[:1]
        for lo in starts:
            rows = np.arange(lo, min(lo + 32, M))
            rows = rows[real[rows]]
            if rows.size and (ref[rows] != 0).any():
                return int(rows[np.argmax((ref[rows] != 0).sum(1))])
        raise AssertionError("no tile's last wave holds a real row")

    def real_mask(self):
        raise NotImplementedError


class GcnStage(Stage):
    """k_sg_gcn on the M rows of a plane. xplane [G + M + G, C]; A [K, V, V] = A' on the PLANE's vertices (a pad vertex: zero row and column);
    W1 [N, K C] in (k, c) order; b1 [P, N] (row r: vertex r % V)."""

    def __init__(self, xplane, geo, A, W1, b1, fp16=False):
        self.x, self.geo, self.A, self.W1, self.b1, self.fp16 = np.asarray(xplane, np.float64), geo, np.asarray(A, np.float64), np.asarray(W1, np.float64), np.asarray(b1, np.float64), fp16
        self.out_fmt = "f16" if fp16 else "split"
        self.K, self.V = self.A.shape[0], geo.V
        self.M, self.C = geo.rows, self.x.shape[1]
        assert self.A.shape[1] == self.V and self.W1.shape[1] == self.K * self.C
        # the nonzero lists of A'_k[:, w], source vertex ascending (rgn_stgcn_finalize); a partition owns as many slots as its longest list
        self.lists = [[[(v, self.A[k, v, w]) for v in range(self.V) if self.A[k, v, w] != 0.0] for w in range(self.V)] for k in range(self.K)]
        self.cnt = [max(len(l) for l in self.lists[k]) for k in range(self.K)]

    def slot_tables(self):
        """(slot_k, sl_v [V][8], sl_a [V][8]) by the contract of rgn_internal.h: slot s serves partition (slot_k >> 4 s) & 15 (15: unused); a list shorter than
        its partition's slot count is padded with (w, 0)."""
        assert sum(self.cnt) <= 8 and self.K <= 8
        sv = np.tile(np.arange(self.V)[:, None], (1, 8)).astype(np.int32)
        sa = np.zeros((self.V, 8), np.float32)
        slot_k = 0xFFFFFFFF
        for w in range(self.V):
            s = 0
            for k in range(self.K):
                for i in range(self.cnt[k]):
                    if i < len(self.lists[k][w]):
                        sv[w, s], sa[w, s] = self.lists[k][w][i][0], self.lists[k][w][i][1]
                    slot_k = (slot_k & ~(15 << (4 * s))) | (k << (4 * s))
                    s += 1
        return slot_k & 0xFFFFFFFF, sv, sa

    def _z(self, mode, mut, absolute=False):
        """the aggregated operand [F, V, K, C] of the body rows."""
        xs = self.x[self.geo.G:self.geo.G + self.M].reshape(-1, self.V, self.C)
        A = self.A
        if mut == "slot_dropped":   # the first entry of the longest list of partition K - 1 ... of ONE vertex
            k = int(np.argmax(self.cnt))
            w = int(np.argmax([len(l) for l in self.lists[k]]))
            A = A.copy()
            A[k, self.lists[k][w][0][0], w] = 0.0
        if absolute:
            return np.einsum("kvw,fvc->fwkc", np.abs(A), np.abs(xs))
        chain16 = self.fp16 and mut != "agg_fp32"
        if not chain16 and mode != "x3":
            z = np.einsum("kvw,fvc->fwkc", A, xs)
            if self.fp16:                                     # mutant: the sum in fp32, rounded to fp16 once
                return f16(f32(z).astype(np.float64))
            return z if mode == "f64" else f32(z).astype(np.float64)
        # the chains: slot i of partition k, for every vertex at once (a padded slot: coefficient 0, source the vertex itself)
        rnd = f16 if chain16 else (lambda v: f32(v).astype(np.float64))
        z = np.zeros((xs.shape[0], self.V, self.K, self.C))
        for k in range(self.K):
            for i in range(self.cnt[k]):
                src = np.array([self.lists[k][w][i][0] if i < len(self.lists[k][w]) else w for w in range(self.V)])
                co = np.array([(A[k, self.lists[k][w][i][0], w] if i < len(self.lists[k][w]) else 0.0) for w in range(self.V)])
                if chain16 and mut != "coef_unrounded":
                    co = f16(co)
                z[:, :, k, :] = rnd(co[None, :, None] * xs[:, src, :] + z[:, :, k, :])
        return z

    def _blocks_of(self, z):
        M, C, K = self.M, self.C, self.K
        if C % 32:
            return [(z.reshape(M, K * C), self.W1)]
        step = 64 if self.fp16 else 32                      # fp16: a window holds two channel blocks
        out = []
        for c0 in range(0, C, step):
            for k in range(K):
                out.append((z[:, :, k, c0:c0 + step].reshape(M, step), self.W1[:, k * C + c0:k * C + c0 + step]))
        return out

    def blocks(self, mode, mut):
        return self._blocks_of(self._z(mode, mut))

    def abs_products(self):
        return abs_sum(self._blocks_of(self._z("f64", None, absolute=True)))

    def addends(self, mut):
        P = self.b1.shape[0]
        r = np.arange(self.M)
        idx = r % P
        if mut == "bias_neighbour":   # where row % P wraps inside a 32-row tile, the rows behind the wrap take the next vertex's row
            wrapped = (r % P) < ((r // 32 * 32) % P)
            idx = np.where(wrapped, (idx + 1) % P, idx)
        return self.b1[idx], None

    def real_mask(self):
        m = np.zeros(self.M, bool)
        m[self.geo.real_rows()] = True
        return m


class TconvStage(Stage):
    """k_sg_tconv / k_sg_tconv_pre on the M rows of a PLAIN plane. W2 [N, C, 9]; b2 [N]; tail 0 - 3; xres: the residual plane (tails 2, 3)."""

    def __init__(self, gplane, geo, W2, b2, tail, xres=None, fp16=False):
        assert not geo.poly
        self.g, self.geo, self.W2, self.b2, self.tail, self.fp16 = np.asarray(gplane, np.float64), geo, np.asarray(W2, np.float64), np.asarray(b2, np.float64), tail, fp16
        self.xres = None if xres is None else np.asarray(xres, np.float64)
        assert (tail >= 2) == (xres is not None) and not (fp16 and tail == 0)
        self.relu = tail != 0
        self.out_fmt = "f32" if tail == 0 else ("f16" if fp16 else "split")
        self.M, self.C = geo.rows, self.g.shape[1]

    def _edge_rows(self):
        _, t, _ = self.geo.frame_of_row()
        return np.nonzero((t < 4) | ((t >= self.geo.T - 4) & (t < self.geo.T)))[0]

    def blocks(self, mode, mut):
        g, G, V, M = self.g, self.geo.G, self.geo.V, self.M
        if mut == "pads_neighbour":
            g = with_neighbour_pads(g, self.geo)
        step = 64 if self.fp16 else 32
        out = []
        for c0 in range(0, self.C, step):
            for dt in range(9):
                a = g[G + (dt - 4) * V:G + (dt - 4) * V + M, c0:c0 + step]
                if mut == "tap_edge" and dt == 2:             # one tap one frame off, in the first / last four frames of a sequence only
                    a = a.copy()
                    e = self._edge_rows()
                    a[e] = g[G + (dt - 3) * V + e, c0:c0 + step]
                out.append((a, self.W2[:, c0:c0 + step, dt]))
        return out

    def addends(self, mut):
        if self.xres is None:
            return self.b2[None, :], None
        res = self.xres[self.geo.G:self.geo.G + self.M]
        if mut == "resid_hi":
            res = f16(res) if self.fp16 else split(res)[0]
        return self.b2[None, :], res

    def real_mask(self):
        m = np.zeros(self.M, bool)
        m[self.geo.real_rows()] = True
        return m


class TconvS2Stage(Stage):
    """k_sg_tconv_s2 on the rows of ONE region of polyphase planes (gplane, xplane: E | O). W2 [N, C, 9]; Wr [N, Cin]; bias = b2' + br'. Output rows:
    (sequence, frame of ceil(T / 2) + 4, vertex), the geometry of a plain plane of ceil(T / 2) frames."""

    def __init__(self, gplane, xplane, geo, W2, Wr, bias, fp16=False, conv_only=False):
        assert geo.poly
        self.conv_only = conv_only      # the row-shifted GEMM with the stride-2 tap table (launch_gemm_x3_sg): the fp32 convolution alone - no shortcut, bias or ReLU
        if conv_only:
            xplane, Wr, bias = np.zeros((np.asarray(gplane).shape[0], 0)), np.zeros((np.asarray(W2).shape[0], 0)), np.zeros(np.asarray(W2).shape[0])
            self.relu = False
        self.g, self.x, self.geo = np.asarray(gplane, np.float64), np.asarray(xplane, np.float64), geo
        self.W2, self.Wr, self.bias, self.fp16 = np.asarray(W2, np.float64), np.asarray(Wr, np.float64), np.asarray(bias, np.float64), fp16
        self.out_fmt = "f32" if conv_only else ("f16" if fp16 else "split")
        self.M, self.C, self.Cin = geo.region, self.g.shape[1], self.x.shape[1]
        self.out_geo = Geo(geo.NM, geo.Treg, geo.V)

    def blocks(self, mode, mut):
        g, G, V, M = self.g, self.geo.G, self.geo.V, self.M
        if mut == "pads_neighbour":
            g = with_neighbour_pads(g, self.geo)
        step = 64 if self.fp16 else 32
        out = []
        for c0 in range(0, self.C, step):
            for i9 in range(9):                                # E taps dt = 0, 2, 4, 6, 8, then O taps 1, 3, 5, 7
                j, reg, dt = (i9, 0, 2 * i9) if i9 < 5 else (i9 - 5, 1, 2 * (i9 - 5) + 1)
                lo = G + reg * M + (j - 2) * V
                a = g[lo:lo + M, c0:c0 + step]
                if mut == "tap_edge" and i9 == 1:
                    a = a.copy()
                    _, t, _ = self.geo.frame_of_row()
                    e = np.nonzero((t < 2) | ((t >= self.geo.Treg - 2) & (t < self.geo.Treg)))[0]   # the first / last four INPUT frames
                    a[e] = g[lo + V + e, c0:c0 + step]
                out.append((a, self.W2[:, c0:c0 + step, dt]))
        if mut != "shortcut_dropped":
            for c0 in range(0, self.Cin, step):
                out.append((self.x[G:G + M, c0:c0 + step], self.Wr[:, c0:c0 + step]))
        return out

    def addends(self, mut):
        return self.bias[None, :], None

    def real_mask(self):
        m = np.zeros(self.M, bool)
        m[self.out_geo.real_rows()] = True
        return m


class GemmStage(Stage):
    """launch_gemm_x3_sg with the (row % add_mod) addend and ReLU - the GEMM of the two-launch graph convolution: relu(z . W^T + b1[row % P]) on the body rows
    of the plane z [G + M + G, K] (the aggregated operand, as planes)."""

    def __init__(self, zplane, geo, W, b1):
        self.z, self.geo, self.W, self.b1 = np.asarray(zplane, np.float64), geo, np.asarray(W, np.float64), np.asarray(b1, np.float64)
        self.M = geo.rows

    def blocks(self, mode, mut):
        body = self.z[self.geo.G:self.geo.G + self.M]
        return [(body[:, k:k + 32], self.W[:, k:k + 32]) for k in range(0, body.shape[1], 32)]

    addends = GcnStage.addends
    real_mask = GcnStage.real_mask


def gcn(xplane, geo, A, W1, b1):
    """The graph convolution on every row of the plane, float64 [rows, N]."""
    return GcnStage(xplane, geo, A, W1, b1).evaluate()


def tconv(gplane, geo, W2, b2, tail, xres=None):
    return TconvStage(gplane, geo, W2, b2, tail, xres).evaluate()


def tconv_s2(gplane, xplane, geo, W2, Wr, bias):
    return TconvS2Stage(gplane, xplane, geo, W2, Wr, bias).evaluate()


# ---- statistics --------------------------------------------------------------------------------------------------------------------------------------------
def stats_split(got, ref, S):
    """(max u, rms u), u = |got - ref| / (2^-24 S) elementwise; an element with S = 0 must be met exactly."""
    d = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(S > 0, d / (U24 * S), np.where(d > 0, np.inf, 0.0))
    u = np.where(np.isfinite(d), u, np.inf)
    return float(u.max()), float(np.sqrt(np.mean(np.square(u))))


def stats_f16(got, ref):
    """(share of elements that differ from the rounded statement, max and rms difference in fp16 ulps of the statement's value)."""
    got = np.asarray(got, np.float64)
    ulp = np.spacing(np.abs(ref).astype(np.float16)).astype(np.float64)
    d = np.where(np.isfinite(got), np.abs(got - ref) / ulp, np.inf)
    return float(np.mean(d != 0)), float(d.max()), float(np.sqrt(np.mean(np.square(d))))


# ---- the fold and the composition ----------------------------------------------------------------------------------------------------------------------------
def padded_nodes(V):
    """rgn_sg_plan.h sg_padded_nodes / sg_bias_period."""
    return V if V >= 28 else (16 if V <= 16 else (V + 3) // 4 * 4)


def bias_period(V):
    Vp = padded_nodes(V)
    return V if V >= 28 else Vp * ((28 + Vp - 1) // Vp)


def fold(sd, blocks, cast=None):
    """rgn_stgcn_finalize in float64 -> (data_bn scale, shift, [per block dict(A, W1, b1, W2, b2, Wr, br, stride)]) on the plane's Vp vertices.
    cast = np.float32: every folded tensor rounded to fp32, as finalize stores them (b2r then is the fp32 sum b2' + br')."""
    d = lambda k: np.asarray(sd[k], dtype=np.float64)   # noqa: E731
    c = (lambda a: a) if cast is None else (lambda a: np.asarray(a).astype(cast).astype(np.float64))

    def bn(p):
        s = d(p + ".weight") / np.sqrt(d(p + ".running_var") + 1e-5)
        return s, d(p + ".bias") - d(p + ".running_mean") * s

    K, V = sd["A"].shape[0], sd["A"].shape[1]
    Vp, P = padded_nodes(V), bias_period(V)
    s0, t0 = bn("data_bn")
    out = []
    for i, (co, stride) in enumerate(blocks):
        p = f"st_gcn_networks.{i}."
        A = (np.asarray(sd["A"], np.float32) * np.asarray(sd[f"edge_importance.{i}"], np.float32)).astype(np.float64)   # stgcn.py:105, an fp32 product
        wg, bg = d(p + "gcn.conv.weight")[:, :, 0, 0], d(p + "gcn.conv.bias")
        ci = wg.shape[1]
        s1, t1 = bn(p + "tcn.0")
        s2, t2 = bn(p + "tcn.3")
        W1 = (s1[:, None, None] * wg.reshape(K, co, ci).transpose(1, 0, 2)).reshape(co, K * ci)
        b1v = s1[None, :] * np.einsum("ko,kw->wo", bg.reshape(K, co), A.sum(1)) + t1[None, :]
        b1 = np.zeros((P, co))
        for r in range(P):
            if r % Vp < V:
                b1[r] = b1v[r % Vp]
        Ap = np.zeros((K, Vp, Vp))
        Ap[:, :V, :V] = A
        blk = dict(A=Ap, W1=c(W1), b1=c(b1), W2=c(s2[:, None, None] * d(p + "tcn.2.weight")[:, :, :, 0]), b2=c(s2 * d(p + "tcn.2.bias") + t2), stride=stride, Wr=None, br=None)
        if (p + "residual.0.weight") in sd:
            sr, tr = bn(p + "residual.1")
            blk["Wr"], blk["br"] = c(sr[:, None] * d(p + "residual.0.weight")[:, :, 0, 0]), c(sr * d(p + "residual.0.bias") + tr)
        out.append(blk)
    return c(s0), c(t0), out


def forward_stages(sd, x, blocks, num_person=1, cast=None):
    """The stage functions composed over a block plan, through the planes rgn_stgcn_forward lays out: x [N, V, C * persons, T] -> (features [N, 256],
    logits), float64. What stands around the three stages is the forward's own: data_bn + the row permutation (k_sg_in), the pad frames back to zero
    behind every stage (k_sg_zero), the mean over persons, frames and REAL vertices (k_sg_pool)."""
    x = np.asarray(x, dtype=np.float64)
    N, V, C2, T = x.shape
    Mp = num_person
    C = C2 // Mp
    s0, t0, blks = fold(sd, blocks, cast)
    Vp = padded_nodes(V)
    # BatchNorm1d channel (m V + v) C + c; rows (n M + m, t, v)
    xs = x.reshape(N, V, Mp, C, T).transpose(0, 2, 4, 1, 3)                        # [N, M, T, V, C]
    st = lambda a: a.reshape(Mp, V, C)[None, :, None, :, :]                        # noqa: E731
    xs = xs * st(s0) + st(t0)
    seq = np.zeros((N * Mp, T, Vp, C))
    seq[:, :, :V] = xs.reshape(N * Mp, T, V, C)                                      # pad vertices are written as zeros
    for i, b in enumerate(blks):
        ipoly = b["stride"] == 2
        geo = Geo(N * Mp, T, Vp, ipoly)
        xp = geo.plane(seq)
        g = gcn(xp, geo, b["A"], b["W1"], b["b1"])
        gp = geo.plane(geo.seq(g))                                                   # k_sg_zero: pad frames and guard rows back to zero
        if ipoly:
            y = tconv_s2(gp, xp, geo, b["W2"], b["Wr"], b["b2"] + b["br"] if cast is None else (f32(b["b2"]) + f32(b["br"])).astype(np.float64))
            T = geo.Treg
            seq = Geo(N * Mp, T, Vp).seq(y)
        else:
            assert b["Wr"] is None, "a stride-1 block with a convolved shortcut runs through k_sg_post: outside the fused kernels"
            y = tconv(gp, geo, b["W2"], b["b2"], 2 if i > 0 else 1, xp if i > 0 else None)
            seq = geo.seq(y)
        # (the polyphase store of a block in front of a stride-2 block changes WHERE a row lands, not its value: Geo.plane of the next block is that store)
    feats = seq[:, :, :V].reshape(N, Mp, T, V, -1).mean(axis=(1, 2, 3))
    wf, bf = np.asarray(sd["fcn.weight"], np.float64)[:, :, 0, 0], np.asarray(sd["fcn.bias"], np.float64)
    return feats, feats @ wf.T + bf
