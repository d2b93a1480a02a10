"""Inputs of the loss-term tests: the property grid of tests/test_losses_gpu.py and the generator that the fixture recorder
(tests/golden/make_golden_losses.py) shares with it. NumPy (PCG64) and the torch restatements only.

A motion is a random base pose plus a cumulative drift per frame: nominally 0.01 per entry with vel_threshold 0.03, or 0.004 with 0.01, each row
at 0.5 to 2.5 times that rate. On the 55-joint skeleton that leaves 60 - 90 % of the foot frames in contact and the rest out of it, so both sides
of the foot-contact threshold are exercised. Two conditions on the
inputs are ENFORCED by a seed search (find_inputs) and checked on the CPU, in fp64:

  * the relative root orientation between the actor and either reactor (target, output) stays <= 3.0 rad. Near pi the quaternion's real part goes
    through the square root of a difference that cancels to nothing (`_sqrt_positive_part`), and fp32 has no digits left to compare. The actor's root
    is drawn as the reactor's times a rotation of at most 2 rad;
  * a motion whose ground-truth foot speed comes within 16 d of the threshold, d = the deviation of the fp32 joint restatement from the fp64 one on
    that very input, is "undecided": fp32 arithmetic may legitimately put the frame on either side. Fixtures hold none; a property case may hold
    one, whose fc comparison is skipped (and reported)."""
import numpy as np
import torch

from regennet_amd import synth
from tests.losses_ref import joints_of, matrix_to_angle
from tests.rot2xyz_ref import rotation_6d_to_matrix

MAX_ANGLE = 3.0
GAP_FACTOR = 16.0

SKELETONS = {
    # kind: (joints, foot joints of the fc term, row of the transl term)
    "tree55": (55, (7, 10, 8, 11), 55),
    "tree9": (9, (5, 8, 6, 7), 4),
}


def skeleton(kind):
    J = SKELETONS[kind][0]
    return synth.make_skeleton(J) if J == 55 else synth.make_skeleton(J, depth=8, seed=J)        # tree9: one chain of 8 edges


def _rotmat(q):
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = (q[..., i] for i in range(4))
    m = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                  2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)
    return m.reshape(q.shape[:-1] + (3, 3))


def make_motions(B, T, J, drift, seed):
    """target, output, cmotion fp32 [B, J + 1, 6, T]: rot6d rows of proper rotations (+ drift), last row [tx, ty, tz, 0, 0, 0] (+ drift on tx..tz).
    The output is the target's base pose moved by 0.05 per entry with a drift of its own; the actor is independent but for its root."""
    rng = np.random.Generator(np.random.PCG64(seed))

    def rows(base_rot, base_tr):
        x = np.zeros((B, J + 1, 6, T))
        rate = drift * rng.uniform(0.5, 2.5, (B, J, 1, 1))               # rows drift at 0.5 .. 2.5 times the nominal rate: feet on both sides of the threshold
        x[:, :J] = base_rot[..., None] + np.cumsum(rate * rng.standard_normal((B, J, 6, T)), axis=-1)
        x[:, J, :3] = base_tr[..., None] + np.cumsum(drift * rng.standard_normal((B, 3, T)), axis=-1)
        return x

    rt = _rotmat(rng.standard_normal((B, J, 4)))                                  # the reactor's base pose
    tr_t = rng.uniform(-1, 1, (B, 3))
    target = rows(rt[:, :, :2].reshape(B, J, 6), tr_t)
    output = rows(rt[:, :, :2].reshape(B, J, 6) + 0.05 * rng.standard_normal((B, J, 6)), tr_t + 0.05 * rng.standard_normal((B, 3)))
    rc = _rotmat(rng.standard_normal((B, J, 4)))
    axis = rng.standard_normal((B, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    half = 0.5 * rng.uniform(0.2, 2.0, B)
    rc[:, 0] = rt[:, 0] @ _rotmat(np.concatenate([np.cos(half)[:, None], np.sin(half)[:, None] * axis], -1))
    cmotion = rows(rc[:, :, :2].reshape(B, J, 6), rng.uniform(-1, 1, (B, 3)))
    return {k: np.ascontiguousarray(v).astype(np.float32) for k, v in (("target", target), ("output", output), ("cmotion", cmotion))}


def make_mask(kind, B, T, seed=0):
    """bool [B, T]. 'full'; 'ragged': motion 0 with holes (frame 0 among them: a pair's mask is that of its LATER frame), the others cut to a
    random length of at least 2 frames."""
    m = np.ones((B, T), bool)
    if kind == "ragged":
        rng = np.random.Generator(np.random.PCG64(1000 + seed))
        m[0, 0] = False
        if T > 4:
            m[0, 2:] = rng.uniform(size=T - 2) < 0.6
            m[0, T - 1] = True
        for b in range(1, B):
            m[b, int(rng.integers(2, T + 1)):] = False
    else:
        assert kind == "full"
    return m


def conditions(inp, sk, foot, vel_threshold):
    """What the two conditions look at, per motion: max_angle [B], gap [B] (smallest distance of a ground-truth foot speed to the threshold),
    d [B] (fp32 joint restatement against fp64, target), undecided [B], contact (share of foot frames at or below the threshold)."""
    t, o, c = (torch.from_numpy(inp[k]).double() for k in ("target", "output", "cmotion"))
    rc, rt, ro = (rotation_6d_to_matrix(a[:, 0:1].permute(0, 1, 3, 2)) for a in (c, t, o))
    ang = torch.maximum(matrix_to_angle(rc.transpose(-1, -2) @ rt), matrix_to_angle(rc.transpose(-1, -2) @ ro)).flatten(1).max(1).values.numpy()
    x64 = joints_of(inp["target"], sk, torch.float64)
    x32 = joints_of(inp["target"], sk, torch.float32).double()
    d = (x32 - x64).abs().flatten(1).max(1).values.numpy()
    B, T = inp["target"].shape[0], inp["target"].shape[-1]
    if T < 2:
        return {"max_angle": ang, "gap": np.full(B, np.inf), "d": d, "undecided": np.zeros(B, bool), "contact": float("nan")}
    fj = list(foot)
    speed = torch.linalg.norm(x64[:, fj, :, 1:] - x64[:, fj, :, :-1], dim=2)
    gap = (speed - vel_threshold).abs().flatten(1).min(1).values.numpy()
    return {"max_angle": ang, "gap": gap, "d": d, "undecided": gap < GAP_FACTOR * d, "contact": float((speed <= vel_threshold).double().mean())}


def find_inputs(B, T, skel, drift, vel_threshold, seed, max_undecided=1, tries=200):
    """The first seed at or after `seed` whose motions meet both conditions -> (inputs, conditions, seed used)."""
    J, foot, _ = SKELETONS[skel]
    sk = skeleton(skel)
    for s in range(seed, seed + tries):
        inp = make_motions(B, T, J, drift, s)
        cond = conditions(inp, sk, foot, vel_threshold)
        if float(cond["max_angle"].max()) <= MAX_ANGLE and int(cond["undecided"].sum()) <= max_undecided:
            return inp, cond, s
    raise RuntimeError(f"no seed in [{seed}, {seed + tries}) meets the input conditions for B={B} T={T} {skel}")


SHAPES = [(1, 2), (3, 7), (2, 32), (2, 33), (3, 65), (2, 150)]     # T = 2: the shortest motion with a velocity; 33 / 65: a pair across a tile boundary; 150: Chi3D
DRIFTS = [(0.01, 0.03), (0.004, 0.01)]
# (B, T, skeleton, mask, drift, vel_threshold, first seed): every shape with both masks on the 55-joint skeleton, and once on the 9-joint one
GRID = [(B, T, "tree55", mk, *DRIFTS[(i + j) % 2], 100 * i + 10 * j) for i, (B, T) in enumerate(SHAPES) for j, mk in enumerate(("full", "ragged"))]
GRID += [(B, T, "tree9", ("ragged", "full")[i % 2], *DRIFTS[i % 2], 100 * i + 50) for i, (B, T) in enumerate(SHAPES)]
