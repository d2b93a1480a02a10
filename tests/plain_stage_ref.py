"""The arithmetic of the plain 16-bit phase, stated once on the host: one function per kernel, on natural-layout arrays.

"Plain phase" = the kernels whose MFMA operands are single 16-bit values (bf16, or IEEE fp16 through OpFmt<true>) with fp32 accumulation. What
such a kernel computes is fixed by (a) WHERE a value becomes 16-bit, (b) which form of each non-linear function runs and (c) the order of the
fp32 sums. (a) and (b) are stated here, per kernel, from the kernel's text; (c) is the one freedom an implementation has, and the `acc`
modes other than "f64" are members of that family:

    acc = "f64"           every sum, product and elementwise operation in float64: the statement proper (what the GPU tests compare with)
    acc = "f32"           the same text in float32. A contraction takes exact 8-deep partial products (a product of two 16-bit operands is exact in
                          fp32; the partial is formed in float64 and rounded once), one after the other, into an fp32 accumulator; a row sum is a halving tree
    acc = "f32_reversed"  ... with every contraction and every row sum fed in reversed order
    acc = "f32_chain"     ... with 16-deep partials, as the kernels' k-loops run: v_mfma_f32_32x32x16 adds one 16-deep product per instruction to the
                          accumulator (32 dependent additions at K = 512, 64 at K = 1024), and the LayerNorm sums as eight 64-column partials (one per
                          wave, rgn_tail.h) added pairwise
    acc = "f32_ulp"       "f32_chain" with every result of the not correctly rounded operations below moved by -1, 0 or +1 fp32 ulp (seeded)
Every fp32 member is built from IEEE-exact elementwise fp32 operations, float64 partials rounded once and float64 transcendentals rounded once - no fp32
BLAS call and no fp32 library sum - so that the family, and with it every bound, is designed to be the same on every host (what is left: a float64
exp2, sqrt or partial that differs in its last ulp between two libraries can, rarely, round to another fp32 value and move a flip count with it).

The difference between "f64" and the fp32 members, at the 16-bit OUTPUT of a stage, is how far two correct implementations of the same
arithmetic may lie apart; tests/plain_stage_cases.py turns it into the bounds (twice the worst of them).

A rounding is round-to-nearest-even through the torch dtype (`Ctx.rnd(x, site)`), every rounding SITE has a name and can be switched off
(`off=`), and every other way of being subtly wrong the tests know of is a named mutation (`mut=`). Inputs are natural layout: activations
[rows, 512], nn.Linear weights [out, in], vectors [n].

Operations of the kernels whose fp32 result is NOT correctly rounded, and which this file therefore states as "+-1 fp32 ulp" operations
(evaluated exactly here; 2^-24 relative is 2^-15 of a bf16 and 2^-12 of an fp16 rounding step, far inside the summation freedom above):

    v_exp_f32   __builtin_amdgcn_exp2f   softmax numerators, flash rescale factors  rgn_qkv_attn.hip qa_attention, rgn_attn.h attn_exp2_sum,
                                                                                   rgn_qkv_attn_long.hip, rgn_layers.hip
    v_rsq_f32   __builtin_amdgcn_rsqf    LayerNorm 1 / sqrt(var + eps)             rgn_tail.h tail_layernorm, rgn_rowgemm.hip norm
    (the softmax's 1.0f / sum is an IEEE division: hipcc rounds fp32 division correctly by default)

The sources are built with -ffp-contract=off: a * b + c written as such is a multiply and an add; the FMAs the kernels DO run are written as
__builtin_elementwise_fma (LayerNorm's two output FMAs, the GELU polynomial, the sum of squares) - one rounding where this file's fp32 modes
have two, which is again inside the family.
"""
import math

import numpy as np
import torch

FMT = {"bf16": torch.bfloat16, "fp16": torch.float16}
ACCS = ("f64", "f32", "f32_reversed", "f32_chain", "f32_ulp")
D, FF, H, DH = 512, 1024, 4, 128

# gelu2_p13 (rgn_device.h): x (0.5 + t Q(t^2)), t = clamp(x, +-3.9); t Q(t^2) ~ Phi(t) - 0.5 is an odd degree-13 polynomial. The coefficients of Q,
# highest power of t^2 first, as the fp32 literals of the kernel (data, not code)
GELU_P13_CLAMP = 3.9
GELU_P13_Q = (3.214928057e-08, -2.075321845e-06, 5.740237248e-05, -9.056383278e-04, 9.218782187e-03, -6.556465477e-02, 3.986084461e-01)
LN_EPS = 1e-5
LOG2E_F32 = np.float32(1.44269504088896340736)


def qscale_f32(dh=DH):
    """1 / sqrt(dh) as the engine forms it (rgn_plan.cpp qscale): fp32 division of 1 by fp32 sqrt. 1 / sqrt(128) = 0.0884 is no power of two, so
    WHERE it multiplies decides what q rounds to."""
    return np.float32(1.0) / np.sqrt(np.float32(dh))


class Ctx:
    """fmt, acc, the rounding sites switched off and the mutations switched on."""

    def __init__(self, fmt, acc="f64", off=(), mut=()):
        assert fmt in FMT and acc in ACCS
        self.fmt, self.acc, self.off, self.mut = fmt, acc, frozenset(off), frozenset(mut)
        self.dt = torch.float64 if acc == "f64" else torch.float32
        self.rev, self.chain = acc == "f32_reversed", acc in ("f32_chain", "f32_ulp")
        self.depth = None if acc == "f64" else (16 if self.chain else 8)
        self.gen = torch.Generator().manual_seed(1) if acc == "f32_ulp" else None

    def t(self, x):
        return torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).to(self.dt)

    def rnd(self, x, site):
        """x -> the nearest value of the 16-bit format (ties to even), unless `site` is switched off."""
        if site in self.off or "*" in self.off:
            return x
        return x.to(torch.float32).to(FMT[self.fmt]).to(self.dt)

    def mm(self, a, w, name):
        """a [.., K] . w [.., N, K]^T in the accumulation mode; mutation "kblock:<name>": the last 32 columns of K never contracted."""
        if "kblock:" + name in self.mut:
            a, w = a[..., :-32], w[..., :-32]
        a, w = a.double(), w.double()
        if self.depth is None:
            return a @ w.transpose(-1, -2)
        if self.rev:
            a, w = a.flip(-1), w.flip(-1)
        out = torch.zeros(a.shape[:-1] + (w.shape[-2],), dtype=torch.float32)
        for k0 in range(0, a.shape[-1], self.depth):
            out = out + (a[..., k0:k0 + self.depth] @ w[..., k0:k0 + self.depth].transpose(-1, -2)).float()
        return out

    @staticmethod
    def _tree(x):
        n = 1
        while n < x.shape[-1]:
            n *= 2
        if n != x.shape[-1]:
            x = torch.cat((x, torch.zeros(x.shape[:-1] + (n - x.shape[-1],), dtype=x.dtype)), -1)
        while x.shape[-1] > 1:
            x = x[..., :x.shape[-1] // 2] + x[..., x.shape[-1] // 2:]
        return x

    def rowsum(self, x):
        if self.depth is None:
            return x.sum(-1, keepdim=True)
        if self.rev:
            x = x.flip(-1)
        if self.chain and x.shape[-1] % 64 == 0:
            x = self._tree(x.reshape(x.shape[:-1] + (x.shape[-1] // 64, 64)))[..., 0]
        return self._tree(x)

    def rsqrt(self, x):
        """1 / sqrt(x) [v_rsq_f32, +-1 ulp]: the float64 value rounded once (a host library's fp32 reciprocal or sqrt need not be IEEE's)."""
        return self.hw((1.0 / torch.sqrt(x.double())).to(self.dt))

    def recip(self, x):
        """1.0f / x as IEEE rounds it."""
        return (1.0 / x.double()).to(self.dt)

    def exp2(self, x):
        """exp2 [+-1 ulp in the kernels]: in the fp32 modes the float64 value rounded once."""
        return self.hw(torch.exp2(x.double()).to(self.dt))

    def hw(self, x):
        """The result of a hardware transcendental (v_exp_f32, v_rsq_f32): exact here, +-1 ulp in the "f32_ulp" mode."""
        if self.gen is None:
            return x
        r = torch.randint(0, 3, x.shape, generator=self.gen)
        up, dn = torch.nextafter(x, torch.full_like(x, float("inf"))), torch.nextafter(x, torch.full_like(x, float("-inf")))
        return torch.where(r == 0, dn, torch.where(r == 2, up, x))

    def bias(self, b, name):
        b = self.t(b)
        return torch.zeros_like(b) if "drop:" + name in self.mut else b


def rounded(x, fmt):
    """A float32 ndarray of values representable in fmt: what the kernels are fed."""
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(FMT[fmt]).to(torch.float32).numpy()


def gelu_p13(x):
    t = x.clamp(-GELU_P13_CLAMP, GELU_P13_CLAMP)
    z = t * t
    p = torch.full_like(x, GELU_P13_Q[0])
    for c in GELU_P13_Q[1:]:
        p = p * z + c
    return x * (t * p + 0.5)


def gelu_erf(x):
    return x * 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)))


def _gelu(c, x):
    if "gelu:erf" in c.mut:
        return gelu_erf(x)
    if "gelu:tanh" in c.mut:
        return gelu_tanh(x)
    return gelu_p13(x)


def _layernorm(c, x, gamma, shift):
    """tail_layernorm (rgn_tail.h): ONE pass - sum and sum of squares together, mean = s / 512, var = max(q / 512 - mean^2, 0),
    r = rsq(var + 1e-5) [+-1 ulp], out = (x r - mean r) gamma + shift. `shift` is beta plus whatever the kernel folded into it."""
    eps = 1e-6 if "eps" in c.mut else LN_EPS
    n = x.shape[-1]
    mean = c.rowsum(x) / n
    var = (c.rowsum(x * x) / n - mean * mean).clamp_min(0.0)
    r = c.rsqrt(var + eps)
    return (x * r + (-mean * r)) * gamma + shift


def _pervec_rows(c, M, Tq, nsamp):
    """The sample whose per-sample vector row m takes: m // Tq. Mutation "pervec_row": (m + 1) // Tq - the last token of a sample takes its successor's."""
    m = torch.arange(M)
    s = (m + 1) // Tq if "pervec_row" in c.mut else m // Tq
    return s.clamp_max(nsamp - 1)


def attn_stage(c, x, Wqkv, bqkv, Tq, qscale=None):
    """k_qkv_attn_rs<false> (rgn_qkv_attn.hip): packed in_proj + causal softmax attention of Bm samples of Tq <= 64 tokens, 4 heads of 128.
    x [Bm Tq, 512] (the residual-stream plane), Wqkv [1536, 512], bqkv [1536] -> the attention image [Bm Tq, 512] (head hd = columns 128 hd ..).

    Sites, in the kernel's order (qa_attention, "xq / xk / xv"):
      "w", "in"   the weight plane and the input plane hold 16-bit values (the packer's / the previous kernel's rounding)
      "q"         q = 16bit( (x . Wq^T + b_q) * qs2 ),  qs2 = fp32(qscale * log2 e): q is PRE-SCALED, and by log2 e as well - the scores are in
                  log2 units and the softmax is exp2(s - max). The bias goes in before the scale, in fp32
      "k"         k = 16bit( x . Wk^T + b_k )   - this kernel ADDS b_k (it is softmax-invariant up to this rounding; k_layers drops it)
      "v"         v = 16bit( x . Wv^T + b_v )
                  s[key, query] = k . q summed in fp32 (four 32-wide dh partials, one per wave, added in wave order); key visible iff
                  key <= min(query, Tq - 1); max and sum over the visible keys in fp32; e = exp2(s - max) [+-1 ulp]
      "p"         p = 16bit(e): the UNNORMALISED numerator (<= 1) is the MFMA operand; the sum that normalises is of the unrounded e
      "out"       att = 16bit( (p . v) * (1.0f / sum) )
    Rows >= Tq of the 64-row tile replicate token Tq - 1 and are never stored. For a stored query q < Tq every key <= q is < Tq, so in the causal
    form "the padded keys left unmasked" changes nothing that is written: that mutant does not apply here (it does to the full-attention form)."""
    x, W = c.rnd(c.t(x), "in"), c.rnd(c.t(Wqkv), "w")
    B = x.shape[0] // Tq
    qs = np.float32(qscale_f32() if qscale is None else qscale)
    qs2 = float(np.float32(qs * LOG2E_F32))
    if "scale_in_exponent" in c.mut:   # where k_layers puts it
        qs2 = 1.0
    qkv = c.mm(x, W, "qkv")
    b = c.t(bqkv)
    q = c.rnd((qkv[:, :D] + c.bias(b[:D], "b_q")) * qs2, "q")
    k = c.rnd(qkv[:, D:2 * D] + c.bias(b[D:2 * D], "b_k"), "k")
    v = c.rnd(qkv[:, 2 * D:] + c.bias(b[2 * D:], "b_v"), "v")
    q, k, v = _heads(q, B, Tq), _heads(k, B, Tq), _heads(v, B, Tq)
    s = c.mm(q, k, "s")                                              # [B, H, query, key]
    if "scale_in_exponent" in c.mut:
        s = s * float(np.float32(qs * LOG2E_F32))
    return _softmax_pv(c, s, v, Tq).permute(0, 2, 1, 3).reshape(B * Tq, D)


def _softmax_pv(c, s, v, Tq):
    qi, ki = torch.arange(Tq)[:, None], torch.arange(Tq)[None, :]
    lim = (qi + 1).clamp_max(Tq - 1) if "causal+1" in c.mut else qi
    s = s.masked_fill(ki > lim, float("-inf"))
    e = c.exp2((s - s.max(-1, keepdim=True).values))
    tot = c.rowsum(e)
    p = c.rnd(e, "p")
    o = c.mm(p, v.transpose(-1, -2), "pv")
    return c.rnd(o * c.recip(tot), "out")


def tail_stage(c, att, h, w, Tq, pervec=None, stepvec=None, step=0):
    """k_mlp2 (rgn_mlp2.hip + rgn_tail.h): the decoder-layer tail of M token rows.
    att, h [M, 512]; w: Wo [512, 512], W1 [1024, 512], W2 [512, 1024], bo, bf1, bf2, g1, b1, g2, b2, g3, b3; pervec [samples, 512] and
    stepvec [steps, 512] (either may be None) -> the next residual-stream plane [M, 512].

      "w", "in"   weight planes, att and h planes hold 16-bit values
                  x  = att . Wo^T (fp32, from zero)  +  (h + b_o)                               out_proj, residual: the bias rides with the residual
                  y1 = LN(x; g1) + ((stepvec[step] + b1) + pervec[row // Tq])                   norm1; its beta and both vectors pre-summed in that order
                  y2 = LN(y1; g2) + b2                                                          norm2
      "hprime"    h' = 16bit(y2): ONE image, read as linear1's operand AND as norm3's residual
                  a  = b_1 + h' . W1^T                                                          (the accumulator starts from the bias)
      "hidden"    g  = 16bit( gelu2_p13(a) ): the polynomial GELU (rgn_device.h), NOT erf
                  z  = b_2 + g . W2^T  + h'                                                     hidden columns 0-511 first, then 512-1023
      "out"       out = 16bit( LN(z; g3) + b3 )
    Every LN is one-pass (sum and sum of squares in one exchange), eps 1e-5, rsq +-1 ulp; see _layernorm."""
    att, h = c.rnd(c.t(att), "in"), c.rnd(c.t(h), "in")
    Wo, W1, W2 = (c.rnd(c.t(w[n]), "w") for n in ("Wo", "W1", "W2"))
    M = att.shape[0]
    x = c.mm(att, Wo, "o") + (h + c.bias(w["bo"], "b_o"))
    shift = c.t(w["b1"]).expand(M, D)
    if stepvec is not None:
        shift = c.t(stepvec)[step] + shift
    if pervec is not None:
        pv = c.t(pervec)
        shift = shift + pv[_pervec_rows(c, M, Tq, pv.shape[0])]
    y = _layernorm(c, x, c.t(w["g1"]), shift)
    y = _layernorm(c, y, c.t(w["g2"]), c.t(w["b2"]))
    return _ffn_norm3(c, y, h, W1, W2, w)


def _ffn_norm3(c, y, h, W1, W2, w):
    hp = c.rnd(y, "hprime")
    a = c.bias(w["bf1"], "b_1") + c.mm(hp, W1, "1")
    g = c.rnd(_gelu(c, a), "hidden")
    z = c.bias(w["bf2"], "b_2") + c.mm(g, W2, "2")
    z = z + (h if "resid_h" in c.mut else hp)                        # mutation: norm3's residual from the layer input instead of h'
    return c.rnd(_layernorm(c, z, c.t(w["g3"]), c.t(w["b3"])), "out")


def _kept_bk(c, b):
    """Mutation "keep:b_k": the k bias a kernel drops, put back (the reference adds it; exact arithmetic cannot tell)."""
    return b[D:2 * D] if "keep:b_k" in c.mut else 0.0


def _heads(t, B, Tq):
    return t.reshape(B, Tq, H, DH).permute(0, 2, 1, 3)


# k_qkv_attn_long's work units (rgn_qkv_attn_long.hip): (query tile, first key tile, last key tile) of waves 0 .. 8; a tile's units are merged in this order
LONG_UNITS = ((0, 0, 0), (1, 0, 1), (2, 1, 2), (3, 2, 3), (4, 4, 4), (2, 0, 0), (3, 0, 1), (4, 0, 1), (4, 2, 3))


def attn_stage_long(c, x, Wqkv, bqkv, Tq, qscale=None):
    """k_qkv_attn_long (rgn_qkv_attn_long.hip + rgn_attn.h): the same stage for 65 .. 160 tokens, one workgroup per (sample, head). What differs
    from attn_stage, site by site:
      "q"    q = 16bit( x . Wq^T + b_q ): UNSCALED. 1 / sqrt(dh) rides in the exponent, e = exp2( fma(s, qs2, -m qs2) ) [+-1 ulp], qs2 = fp32(qscale log2 e)
      "k"    k = 16bit( x . Wk^T ): WITHOUT b_k (q . b_k is the same for every key of a query: the softmax removes it, in real arithmetic)
      "v"    v = 16bit( x . Wv^T + b_v )
             s = k . q in fp32 over the whole head dim (eight 16-wide MFMA steps); key visible iff key <= query and key < Tq
      "p"    flash-style: the causal key tiles of a 32-query tile are split into UNITS of <= 2 key tiles (LONG_UNITS). A unit walks its key tiles with
             a running maximum m and sum l: m' = max(m, tile max); O, l *= exp2((m - m') qs2); p = 16bit( exp2(qs2 s - qs2 m') ) - rounded RELATIVE TO THE
             RUNNING maximum of its unit, not to the row's; O += p . v; l += sum of the unrounded e
             merge, in fp32: O = sum_u exp2((m_u - m) qs2) O_u, l likewise, m = max_u m_u
      "out"  att = 16bit( O * (1.0f / l) )
    Keys >= Tq: as in attn_stage, a stored query never sees one in the causal form - that mutant does not apply."""
    x, W = c.rnd(c.t(x), "in"), c.rnd(c.t(Wqkv), "w")
    B = x.shape[0] // Tq
    qs2 = float(np.float32(np.float32(qscale_f32() if qscale is None else qscale) * LOG2E_F32))
    qkv = c.mm(x, W, "qkv")
    b = c.t(bqkv)
    q = _heads(c.rnd(qkv[:, :D] + c.bias(b[:D], "b_q"), "q"), B, Tq)
    k = _heads(c.rnd(qkv[:, D:2 * D] + _kept_bk(c, b), "k"), B, Tq)
    v = _heads(c.rnd(qkv[:, 2 * D:] + c.bias(b[2 * D:], "b_v"), "v"), B, Tq)
    s = c.mm(q, k, "s")                                              # [B, H, query, key], unscaled
    qi, ki = torch.arange(Tq)[:, None], torch.arange(Tq)[None, :]
    lim = (qi + 1).clamp_max(Tq - 1) if "causal+1" in c.mut else qi
    s = s.masked_fill(ki > lim, float("-inf"))
    out = torch.zeros(B, H, Tq, DH, dtype=c.dt)
    for qt in range((Tq + 31) // 32):
        q0, q1 = 32 * qt, min(32 * qt + 32, Tq)
        parts = []
        for (uq, k0, k1) in LONG_UNITS:
            if uq != qt:
                continue
            m = torch.full((B, H, q1 - q0, 1), float("-inf"), dtype=c.dt)
            l = torch.zeros_like(m)
            O = torch.zeros(B, H, q1 - q0, DH, dtype=c.dt)
            for kj in range(k0, k1 + 1):
                a0, a1 = 32 * kj, min(32 * kj + 32, Tq)
                if a0 >= Tq:
                    continue
                st = s[:, :, q0:q1, a0:a1]
                m_new = torch.maximum(torch.maximum(m, st.max(-1, keepdim=True).values), torch.full_like(m, -1e30))
                alpha = c.exp2(((m - m_new) * qs2))
                e = c.exp2((st * qs2 + (-m_new * qs2)))
                l = l * alpha + c.rowsum(e)
                vt = v[:, :, a0:a1, :]
                if "kblock:pv" in c.mut and kj == k1:
                    e, vt = e[..., :0], vt[:, :, :0, :]
                O = O * alpha + c.mm(c.rnd(e, "p"), vt.transpose(-1, -2), "pv_tile")
                m = m_new
            parts.append((m, l, O))
        m = parts[0][0]
        for (mu, _, _) in parts[1:]:
            m = torch.maximum(m, mu)
        f = [c.exp2(((mu - m) * qs2)) for (mu, _, _) in parts]
        l = sum(lu * fu for (_, lu, _), fu in zip(parts, f))
        O = sum(Ou * fu for (_, _, Ou), fu in zip(parts, f))
        out[:, :, q0:q1] = c.rnd(O * c.recip(l), "out")
    return out.permute(0, 2, 1, 3).reshape(B * Tq, D)


# gelu2_p15 (rgn_device.h): 0.5 x (1 + erf(u)), erf an odd degree-15 polynomial in u = clamp(x / sqrt 2, +-3.2); coefficients of the polynomial in u^2
# that multiplies u, highest power first
GELU_P15_CLAMP = 3.2
GELU_P15_Q = (-2.6911866e-07, 1.2661994e-05, -2.5566161e-04, 2.9286479e-03, -2.1317327e-02, 1.0528564e-01, -3.7135834e-01, 1.1274883e+00)


def gelu_p15(x):
    u = (x * 0.70710678118654752440).clamp(-GELU_P15_CLAMP, GELU_P15_CLAMP)
    z = u * u
    p = torch.full_like(x, GELU_P15_Q[0])
    for cf in GELU_P15_Q[1:]:
        p = p * z + cf
    hx = x * 0.5
    return hx * (p * u) + hx


def _layernorm2(c, x, gamma, beta):
    """k_rowgemm's LayerNorm: TWO passes (mean, then the centred sum of squares), r = rsq(var + 1e-5) [+-1 ulp], out = (x - mean) (r gamma) + beta."""
    eps = 1e-6 if "eps" in c.mut else LN_EPS
    n = x.shape[-1]
    xc = x - c.rowsum(x) / n
    r = c.rsqrt(c.rowsum(xc * xc) / n + eps)
    return xc * (r * gamma) + beta


def rowgemm_stage(c, a, W, bias, epi, Tq=1, qscale=None, resid=None, ga=None, ba=None, gb=None, bb=None, pervec=None, stepvec=None, step=0):
    """k_rowgemm (rgn_rowgemm.hip; bf16 operands only - it has no fp16 form), the kernel-per-stage chain's GEMM with its three epilogues.
    a [M, K], W [N, K], bias [N]; t = a . W^T (fp32 from zero) + bias, then
      epi = "act1"  "out": 16bit( gelu2_p15(t) ) - the degree-15 erf polynomial here, NOT gelu2_p13 and not erf              -> [M, N]
      epi = "act2"  packed in_proj for the slab-staged attention, N = 3 x 512: "q": 16bit( t_q * qscale ) - pre-scaled by 1 / sqrt(dh) alone (no
                    log2 e: k_attn_x3 runs __expf); "k": 16bit( t_k ) WITH b_k; "v": 16bit( t_v )                              -> [M, 1536] = q | k | v
      epi = "ln"    u = t + resid; y = LN_a(u) (two-pass, see _layernorm2); with gb: y = LN_b( y + (stepvec[step] + pervec[row // Tq]) );
                    "out": 16bit(y). The residual plane is 16-bit ("in").                                                      -> [M, 512]"""
    a, W = c.rnd(c.t(a), "in"), c.rnd(c.t(W), "w")
    t = c.mm(a, W, "rg") + c.bias(bias, "b_rg")
    M = a.shape[0]
    if epi == "act1":
        g = gelu_erf(t) if "gelu:erf" in c.mut else (gelu_tanh(t) if "gelu:tanh" in c.mut else (gelu_p13(t) if "gelu:p13" in c.mut else gelu_p15(t)))
        return c.rnd(g, "out")
    if epi == "act2":
        qs = float(np.float32(qscale_f32() if qscale is None else qscale))
        if "qscale_log2e" in c.mut:   # where k_qkv_attn_rs puts it
            qs = float(np.float32(np.float32(qs) * LOG2E_F32))
        return torch.cat((c.rnd(t[:, :D] * qs, "q"), c.rnd(t[:, D:2 * D], "k"), c.rnd(t[:, 2 * D:], "v")), dim=1)
    assert epi == "ln"
    y = _layernorm2(c, t + c.rnd(c.t(resid), "in"), c.t(ga), c.t(ba))
    if gb is not None:
        add = torch.zeros(M, D, dtype=c.dt)
        if stepvec is not None:
            add = add + c.t(stepvec)[step]
        if pervec is not None:
            pv = c.t(pervec)
            add = add + pv[_pervec_rows(c, M, Tq, pv.shape[0])]
        y = _layernorm2(c, y + add, c.t(gb), c.t(bb))
    return c.rnd(y, "out")


def layer_stage(c, h, w, Tq, pervec=None, stepvec=None, step=0, qscale=None):
    """One decoder layer as k_layers<false> composes it (rgn_layers.hip; steps = 0, one workgroup per sample of Tq <= 64 tokens on resident images).
    h [Bm Tq, 512] -> the next residual-stream plane. The tail is tail_stage's text (rgn_tail.h is shared) with x = (b_o + att . Wo^T) + h - the
    accumulator starts from the bias - and pervec [Bm, 512] one row per sample. The attention is NOT attn_stage's:
      "q"    q = 16bit( b_q + x . Wq^T ): UNSCALED, the accumulator starts from the bias; 1 / sqrt(dh) in the exponent, exp2( fma(s, qs2, -max qs2) )
      "k"    k = 16bit( x . Wk^T ): b_k dropped
      "v"    v = 16bit( b_v + x . Wv^T )
             s = k . q, four 32-wide dh partials summed in wave order; key visible iff key <= min(query, Tq - 1)
      "p"    p = 16bit( e * (1.0f / sum) ): the NORMALISED probability is rounded (k_qkv_attn_rs rounds e and normalises the output)
      "att"  att = 16bit( p . v ): the attention image; no multiplication behind the MFMA
      "hprime", "hidden", "out": as tail_stage (the output image of the layer is "out")."""
    x, W = c.rnd(c.t(h), "in"), c.rnd(c.t(w["Wqkv"]), "w")
    B = x.shape[0] // Tq
    qs2 = float(np.float32(np.float32(qscale_f32() if qscale is None else qscale) * LOG2E_F32))
    qkv = c.mm(x, W, "qkv")
    b = c.t(w["bqkv"])
    q = _heads(c.rnd(c.bias(b[:D], "b_q") + qkv[:, :D], "q"), B, Tq)
    k = _heads(c.rnd(qkv[:, D:2 * D] + _kept_bk(c, b), "k"), B, Tq)
    v = _heads(c.rnd(c.bias(b[2 * D:], "b_v") + qkv[:, 2 * D:], "v"), B, Tq)
    s = c.mm(q, k, "s")
    qi, ki = torch.arange(Tq)[:, None], torch.arange(Tq)[None, :]
    lim = (qi + 1).clamp_max(Tq - 1) if "causal+1" in c.mut else qi
    s = s.masked_fill(ki > lim, float("-inf"))
    e = c.exp2((s * qs2 + (-s.max(-1, keepdim=True).values * qs2)))
    p = c.rnd(e * c.recip(c.rowsum(e)), "p")
    att = c.rnd(c.mm(p, v.transpose(-1, -2), "pv"), "att").permute(0, 2, 1, 3).reshape(B * Tq, D)
    Wo, W1, W2 = (c.rnd(c.t(w[n]), "w") for n in ("Wo", "W1", "W2"))
    M = x.shape[0]
    y = (c.bias(w["bo"], "b_o") + c.mm(att, Wo, "o")) + x
    shift = c.t(w["b1"]).expand(M, D)
    if stepvec is not None:
        shift = shift + c.t(stepvec)[step]
    if pervec is not None:
        pv = c.t(pervec)
        shift = shift + pv[_pervec_rows(c, M, Tq, pv.shape[0])]
    y = _layernorm(c, y, c.t(w["g1"]), shift)
    y = _layernorm(c, y, c.t(w["g2"]), c.t(w["b2"]))
    return _ffn_norm3(c, y, x, W1, W2, w)


# ---- what a stage is called with, from a reference-named state dict (synth.make_state_dict / a checkpoint)
def layer_weights(sd, l=0):
    p = f"seqTransDecoder.layers.{l}."
    g = lambda k: np.asarray(sd[p + k], dtype=np.float32)   # noqa: E731
    return {"Wqkv": g("self_attn.in_proj_weight"), "bqkv": g("self_attn.in_proj_bias"), "Wo": g("self_attn.out_proj.weight"),
            "bo": g("self_attn.out_proj.bias"), "W1": g("linear1.weight"), "bf1": g("linear1.bias"), "W2": g("linear2.weight"),
            "bf2": g("linear2.bias"), "g1": g("norm1.weight"), "b1": g("norm1.bias"), "g2": g("norm2.weight"), "b2": g("norm2.bias"),
            "g3": g("norm3.weight"), "b3": g("norm3.bias")}


def stats(a, b):
    """(share of differing elements, rms difference, max abs difference) of two arrays."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    dlt = a - b
    return float((dlt != 0).mean()), float(np.sqrt((dlt * dlt).mean())), float(np.abs(dlt).max())
