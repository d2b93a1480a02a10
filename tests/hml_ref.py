"""fp64 numpy restatement of the reference's hml_vec post-processing, its error model, and structural mutants.

Restated, as the reference writes them:
  inv_transform           data * std + mean                           data_loaders/humanml/data/dataset.py:132 (fp32, on fp32 statistics)
  qinv, qrot              v + 2 (w uv + uuv), uv = qvec x v, uuv = qvec x uv      data_loaders/humanml/common/quaternion.py:14-20, :54-73
  recover_root_rot_pos    the cumsum of the SHIFTED rotation velocities, q = (cos a, 0, sin a, 0) with a NOT halved, the shifted root velocities
                          rotated by qinv(q) and summed, the height row put in     data_loaders/humanml/scripts/motion_process.py:362-381
  recover_from_ric        local positions rotated by qinv(q), root x / z added, root in front      motion_process.py:415-430
  the closing layout      view / permute to [B, J, 3, T]              sample/cgenerate.py:150-152

Input everywhere: x fp32 [B, D, 1, T] in the model's layout, D = 12 J - 1, mean / std fp32 [D] or None (features taken as they are).

THE ERROR MODEL. Every output element is a sum of at most T + 1 rotated vectors: the root velocities u[s], s <= t, and the joint's own local
position. Its absolute-sum companion - the same recurrences with every term replaced by its magnitude - is
    A[t] = (sum_{s <= t} (|f_1[s-1]| + |f_2[s-1]|) + |f_x| + |f_y| + |f_z| of the joint (|f_3| for the root)) * (1 + 2 sum_{s < t} |f_0[s]|).
The first factor bounds what a relative perturbation of every summand does to the sum. The second is the sensitivity to the angle: the frame turns
by 2 a, so a perturbation da of a moves a rotated vector v by at most 2 |da| |v|, and a sum a[t] of up to T terms carried with unit roundoff eps
is off by at most gamma_T sum |f_0| with gamma_T = T eps / (1 - T eps) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Lemma 3.1
and section 4.2: recursive summation of n terms has backward error gamma_{n-1} per term). Hence
    the reference's own fp32 run      |fp32 - exact| <= gamma_T(2^-24) A        gamma32(T) below, FP32_MODEL
    an fp64 evaluation in ANY order   |fp64 - exact| <= (T + 16) 2^-52 A        sums of at most T terms (2 T eps covers any order), sincos and the
                                                                                ten or so operations of a rotation in the + 16
    the kernel                        one more rounding to fp32: 2^-23 |ref| + (T + 16) 2^-52 A      gpu_bound below
Both bounds come from this host model and the number formats, never from a kernel's output.
"""
import numpy as np

EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53


def joints_of(D):
    """22 for the 263 rows of HumanML3D, 21 for the 251 of KIT (cgenerate.py:149: `22 if shape[1] == 263 else 21`); for the other skeletons the
    synthetic shapes use, the J of D = 12 J - 1."""
    assert (D + 1) % 12 == 0 and D >= 23, D
    return (D + 1) // 12


def rows_of(J):
    return 12 * J - 1


def gamma32(T):
    return T * EPS32 / (1.0 - T * EPS32)


def gpu_bound(ref, A, T):
    return 2.0 ** -23 * np.abs(ref) + (T + 16) * 2.0 ** -52 * A


# ---------------------------------------------------------------- the reference's functions, fp64
def qinv(q):
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def qrot(q, v):
    qvec = q[..., 1:]
    uv = np.cross(qvec, v)
    uuv = np.cross(qvec, uv)
    return v + 2 * (q[..., :1] * uv + uuv)


def inv_transform(x, mean, std, skip=False):
    """x [B, D, 1, T] -> data [B, 1, T, D] (the permute of cgenerate.py:150), de-normalised in fp32 (two roundings), then widened."""
    data = np.ascontiguousarray(np.transpose(np.asarray(x, dtype=np.float32), (0, 2, 3, 1)))
    if mean is not None and not skip:
        data = data * np.asarray(std, dtype=np.float32) + np.asarray(mean, dtype=np.float32)
        assert data.dtype == np.float32
    return data.astype(np.float64)


def recover_root_rot_pos(data, mutant=None):
    rot_vel = data[..., 0]
    r_rot_ang = np.zeros_like(rot_vel)
    if mutant == "inclusive_angle_sum":
        r_rot_ang[...] = rot_vel
    else:
        r_rot_ang[..., 1:] = rot_vel[..., :-1]
    r_rot_ang = np.cumsum(r_rot_ang, axis=-1)
    if mutant == "angle_halved":
        r_rot_ang = r_rot_ang / 2
    r_rot_quat = np.zeros(data.shape[:-1] + (4,))
    r_rot_quat[..., 0] = np.cos(r_rot_ang)
    r_rot_quat[..., 2] = np.sin(r_rot_ang)
    r_pos = np.zeros(data.shape[:-1] + (3,))
    r_pos[..., 1:, 0] = data[..., :-1, 1]
    r_pos[..., 1:, 2] = data[..., :-1, 2]
    turn = r_rot_quat if mutant == "q_instead_of_qinv" else qinv(r_rot_quat)
    if mutant == "velocity_under_its_own_angle":          # velocity t-1 turned by the angle of t-1
        turn = np.concatenate((turn[..., :1, :], turn[..., :-1, :]), axis=-2)
    r_pos = qrot(turn, r_pos)
    r_pos = np.cumsum(r_pos, axis=-2)
    if mutant != "root_height_dropped":
        r_pos[..., 1] = data[..., 3]
    return r_rot_quat, r_pos


def recover_from_ric(data, joints_num, mutant=None):
    """data [..., T, D] fp64 -> positions [..., T, J, 3]."""
    r_rot_quat, r_pos = recover_root_rot_pos(data, mutant)
    positions = data[..., 4:(joints_num - 1) * 3 + 4]
    positions = positions.reshape(positions.shape[:-1] + (-1, 3))
    q = r_rot_quat[..., None, :]
    q = np.broadcast_to(q if mutant == "q_instead_of_qinv" else qinv(q), positions.shape[:-1] + (4,))
    positions = qrot(q, positions)
    if mutant != "offsets_not_added":
        positions[..., 0] += r_pos[..., 0:1]
        positions[..., 2] += r_pos[..., 2:3]
    return np.concatenate([r_pos[..., None, :], positions], axis=-2)


def hml_joints_ref(x, mean=None, std=None, mutant=None):
    """cgenerate.py:149-152 in fp64 from the fp32 de-normalised features: x [B, D, 1, T] -> [B, J, 3, T]."""
    J = 22 if mutant == "layout_of_22_joints" else joints_of(x.shape[1])
    data = inv_transform(x, mean, std, skip=mutant == "statistics_skipped")
    pos = recover_from_ric(data, J, mutant)                      # [B, 1, T, J, 3]
    pos = pos.reshape((-1,) + pos.shape[2:])                     # [B, T, J, 3]
    return np.ascontiguousarray(np.transpose(pos, (0, 2, 3, 1)))


def error_model(x, mean=None, std=None):
    """A [B, J, 3, T] (module text): the absolute-sum companion of every output element."""
    J = joints_of(x.shape[1])
    f = np.abs(inv_transform(x, mean, std))[:, 0]                # [B, T, D]
    B, T = f.shape[:2]
    shifted = np.zeros((B, T, 3))
    shifted[:, 1:] = f[:, :-1, 0:3]
    s0 = np.cumsum(shifted[..., 0], axis=1)                      # sum_{s < t} |f_0[s]|
    U = np.cumsum(shifted[..., 1] + shifted[..., 2], axis=1)     # sum_{s <= t} |u[s]|, |u| <= |f_1| + |f_2|
    own = np.concatenate((f[..., 3:4], f[..., 4:4 + 3 * (J - 1)].reshape(B, T, J - 1, 3).sum(-1)), axis=-1)      # [B, T, J]
    A = (U[..., None] + own) * (1.0 + 2.0 * s0)[..., None]       # [B, T, J]
    return np.ascontiguousarray(np.broadcast_to(np.transpose(A, (0, 2, 1))[:, :, None, :], (B, J, 3, T)))


# ---------------------------------------------------------------- structural mutants: name -> the fixtures it can apply to
# (T = 1 has a = 0 and u = 0: no angle, nothing to turn, no offset; raw features have no statistics to skip; only a 251-row vector can be misread
# as 22 joints)
MUTANTS = {
    "angle_halved": lambda B, D, T, stats: T >= 2,
    "inclusive_angle_sum": lambda B, D, T, stats: True,
    "q_instead_of_qinv": lambda B, D, T, stats: T >= 2,
    "velocity_under_its_own_angle": lambda B, D, T, stats: T >= 2,
    "root_height_dropped": lambda B, D, T, stats: True,
    "offsets_not_added": lambda B, D, T, stats: T >= 2,
    "statistics_skipped": lambda B, D, T, stats: stats,
    "layout_of_22_joints": lambda B, D, T, stats: D == 251,
}


def miss_ratio(got, expected, bound):
    """max |got - expected| / bound; a result of another shape misses outright."""
    if got.shape != expected.shape:
        return float("inf")
    return float((np.abs(got - expected) / bound).max())


# ---------------------------------------------------------------- inputs
def make_stats(D, seed):
    """Statistics with the magnitudes of the dataset's: rotation velocity 0.03 +- 0.02 rad per frame (so that |a| passes pi within 196 frames), root
    velocity a few cm per frame, height about 0.9 m, local positions within half a metre; the rows recover_from_ric never reads get values too."""
    rng = np.random.Generator(np.random.PCG64(seed))
    J = joints_of(D)
    mean, std = rng.uniform(-0.5, 0.5, D), rng.uniform(0.1, 1.0, D)
    mean[0], std[0] = 0.03, 0.02
    mean[1:3], std[1:3] = (0.01, 0.02), 0.03
    mean[3], std[3] = 0.9, 0.05
    std[4:4 + 3 * (J - 1)] = rng.uniform(0.05, 0.15, 3 * (J - 1))
    return mean.astype(np.float32), std.astype(np.float32)


def make_inputs(B, D, T, seed, raw=False):
    """(x fp32 [B, D, 1, T], mean, std): seeded N(0, 1) samples of a normalised model; raw: the de-normalised features themselves with mean / std
    None."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal((B, D, 1, T)).astype(np.float32)
    mean, std = make_stats(D, seed + 1)
    if raw:
        return (x * std[None, :, None, None] + mean[None, :, None, None]).astype(np.float32), None, None
    return x, mean, std
