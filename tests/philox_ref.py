"""The engine's noise stream, stated on the host (numpy only): what include/regennet_hip.h promises to callers of rgn_randn / rgn_randn_step and
what rgn_sample_range adds at a loop index when it draws its own noise.

    value(motion b, feature f, frame t) of loop index i  =  Philox(seed; sample_offset + b, i, f * 4096 + t)

  element   e = f * 4096 + t                  (not the flat index: a draw does not depend on the sequence length)
  counter   (e >> 2, stream, sample lo, sample hi), sample = sample_offset + b as a 64-bit integer, stream = i mod 2^32 (x_T: i = -1)
  key       (seed lo, seed hi)
  block     Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 library): four words r0..r3
  pair      p = (e >> 1) & 1 takes the words (r[2p], r[2p+1]); member m = e & 1
  uniforms  u1 = ((r[2p] >> 8) + 1) * 2^-24 in (0, 1],  u2 = (r[2p+1] >> 8) * 2^-24 in [0, 1)
  normal    sqrt(-2 ln u1) * cos(2 pi u2) for m = 0, ... * sin(2 pi u2) for m = 1       (Box-Muller)

normals_f64 evaluates the last line in float64 and is the reference of the GPU tests; normals_f32 evaluates it in float32 the way a float32
implementation writes it (log2 and the -2 ln 2 factor) and serves only to size their tolerance: max |normals_f32 - normals_f64| is what rounding
alone costs such an implementation."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57          # the multipliers of the two 32 x 32 -> 64 products
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85          # the Weyl increments of the key: golden ratio, sqrt(3) - 1
FRAME_STRIDE = 4096                                    # element = feature * FRAME_STRIDE + frame
XT_STREAM = 0xFFFFFFFF                                 # loop index -1: the x_T draw
NEG_2LN2_F32 = np.float32(-1.3862943611198906)


def _u64(a):
    return np.asarray(a, dtype=np.uint64) & M32


def philox4x32_10(c0, c1, c2, c3, k0, k1, rounds=10, m0=PHILOX_M0, m1=PHILOX_M1):
    """Philox4x32 over arrays (broadcast together) of 32-bit words held in uint64. Returns the four output words, uint64 < 2^32.
    One round: (hi0, lo0) = m0 * c0, (hi1, lo1) = m1 * c2; c <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key is bumped between rounds."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[_u64(v) for v in (c0, c1, c2, c3, k0, k1)])
    m0, m1 = np.uint64(m0), np.uint64(m1)
    for r in range(rounds):
        if r:
            k0, k1 = (k0 + np.uint64(PHILOX_W0)) & M32, (k1 + np.uint64(PHILOX_W1)) & M32
        p0, p1 = m0 * c0, m1 * c2                       # < 2^64: no wrap
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
    return c0, c1, c2, c3


def flat_elem(f, t, T):
    """The WRONG element rule a flat [F, T] index would give: kept for the tests that show the suite tells it from the documented one."""
    return f * T + t


def counters(sample, stream, F, T, elem=None):
    """(c0, c1, c2, c3, e) for the [F, T] elements of one motion's draw; `sample` = sample_offset + b, any Python int (taken mod 2^64)."""
    f, t = np.meshgrid(np.arange(F, dtype=np.uint64), np.arange(T, dtype=np.uint64), indexing="ij")
    e = (f * np.uint64(FRAME_STRIDE) + t) if elem is None else np.asarray(elem(f, t, np.uint64(T)), dtype=np.uint64)
    sample = int(sample) % (1 << 64)
    full = np.ones_like(e)
    return e >> np.uint64(2), full * np.uint64(int(stream) % (1 << 32)), full * np.uint64(sample & 0xFFFFFFFF), full * np.uint64(sample >> 32), e


def words(seed, sample, stream, F, T, **kw):
    """The two 32-bit words (u1's, u2's) behind each of the [F, T] elements, and the member index (0: cos, 1: sin)."""
    elem = kw.pop("elem", None)
    c0, c1, c2, c3, e = counters(sample, stream, F, T, elem)
    seed = int(seed) % (1 << 64)
    r = philox4x32_10(c0, c1, c2, c3, seed & 0xFFFFFFFF, seed >> 32, **kw)
    pair = (e >> np.uint64(1)) & np.uint64(1)
    ra = np.where(pair == 0, r[0], r[2])
    rb = np.where(pair == 0, r[1], r[3])
    return ra, rb, (e & np.uint64(1)).astype(np.int64)


def uniforms(seed, sample, stream, F, T, **kw):
    """(u1 in (0, 1], u2 in [0, 1), member) as float64 [F, T]; both uniforms are exact multiples of 2^-24."""
    ra, rb, member = words(seed, sample, stream, F, T, **kw)
    u1 = ((ra >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (rb >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return u1, u2, member


def normals_f64(seed, sample, stream, F, T, **kw):
    """float64 [F, T]: the stream's value at every element."""
    u1, u2, member = uniforms(seed, sample, stream, F, T, **kw)
    rad = np.sqrt(-2.0 * np.log(u1))
    # cos / sin of 2 pi u2 with the quadrant taken off exactly first (u2 is a multiple of 2^-24), so that the zeros of the pair are zeros
    q = np.floor(u2 * 4.0)
    a = 2.0 * np.pi * (u2 - q * 0.25)
    ca, sa = np.cos(a), np.sin(a)
    q = q.astype(np.int64)
    c = np.choose(q, [ca, -sa, -ca, sa])
    s = np.choose(q, [sa, ca, -sa, -ca])
    return rad * np.where(member == 0, c, s)


def normals_f32(seed, sample, stream, F, T, **kw):
    """float32 [F, T]: the same formula carried out in float32 - u * 2^-24, -2 ln 2 * log2(u1), sqrt, cos / sin of 2 pi u2."""
    ra, rb, member = words(seed, sample, stream, F, T, **kw)
    u1 = ((ra >> np.uint64(8)) + np.uint64(1)).astype(np.float32) * np.float32(2.0 ** -24)
    u2 = (rb >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    rad = np.sqrt(NEG_2LN2_F32 * np.log2(u1))
    a = np.float32(2.0 * np.pi) * u2
    out = rad * np.where(member == 0, np.cos(a), np.sin(a))
    assert out.dtype == np.float32
    return out


def batch_normals_f64(seed, sample_offset, stream, B, F, T, **kw):
    """float64 [B, F, T]: rgn_randn_step's output for B motions (reshape to [B, njoints, nfeats, T]: F = njoints * nfeats)."""
    return np.stack([normals_f64(seed, int(sample_offset) + b, stream, F, T, **kw) for b in range(B)])


def batch_normals_f32(seed, sample_offset, stream, B, F, T, **kw):
    return np.stack([normals_f32(seed, int(sample_offset) + b, stream, F, T, **kw) for b in range(B)])
