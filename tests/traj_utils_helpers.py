"""References, inputs and case lists shared by test_gpu_traj_utils.py, test_gpu_frame_ops.py and test_traj_utils_refs_cpu.py.

The references are exact restatements (numpy fp32, same roundings as the torch expressions of the reference) or the fp64 build of
oracle/; test_traj_utils_refs_cpu.py checks them against the recorded goldens and checks that the oracle's own fp32 build stays inside
every tolerance the GPU tests take over, ON THE INPUTS BUILT HERE -- so the GPU tests and the CPU check see the same numbers."""
import numpy as np
import torch

FD_METHODS = ("forward", "backward", "central")


# ---------------------------------------------------------------------------------------------------------------------------------
# exact references
# ---------------------------------------------------------------------------------------------------------------------------------
def interp_ref(x, n):
    """interpolate_traj_via_points (trajectory/utils.py:37-50) in numpy fp32: two rounded products and one rounded sum per element,
    alpha from torch.linspace like the reference, beta = 1 - alpha.  (..., H, D) -> (..., (H-1) n, D)."""
    x = np.asarray(x, np.float32)
    lead, (H, D) = x.shape[:-2], x.shape[-2:]
    x3 = x.reshape(-1, H, D)
    alpha = torch.linspace(0, 1, n + 2, dtype=torch.float32)[1:n + 1].numpy()
    beta = (np.float32(1.0) - alpha).astype(np.float32)
    out = x3[:, :-1, None, :] * alpha[None, None, :, None] + x3[:, 1:, None, :] * beta[None, None, :, None]
    assert out.dtype == np.float32
    return out.reshape(lead + ((H - 1) * n, D))


def fd_ref(x, dt, method):
    """finite_difference_vector (trajectory/utils.py:53-64) in numpy fp32: zero padded, one rounded difference and one correctly
    rounded division by float32(dt) (central: float32(2 dt), an exact doubling) per element."""
    x = np.asarray(x, np.float32)
    out = np.zeros_like(x)
    d1, d2 = np.float32(dt), np.float32(2.0) * np.float32(dt)
    if method == "forward":
        out[..., :-1, :] = (x[..., 1:, :] - x[..., :-1, :]) / d1
    elif method == "backward":
        out[..., 1:, :] = (x[..., 1:, :] - x[..., :-1, :]) / d1
    elif method == "central":
        out[..., 1:-1, :] = (x[..., 2:, :] - x[..., :-2, :]) / d2
    else:
        raise NotImplementedError(method)
    assert out.dtype == np.float32
    return out


def partition_ref(coll_any, outside, inner=0):
    """What get_trajs_collision_and_free's bookkeeping (tasks.py:253-284) yields for given per-trajectory facts, stated directly:
    free = collision free and inside the limits; the other list = colliding ones, then the collision-free limit violators --
    except that it is ONLY the violators when nothing is free but something was collision free."""
    t = np.arange(len(coll_any))
    free = t[~coll_any & ~outside]
    viol = t[~coll_any & outside]
    coll = t[coll_any]
    if len(free) + len(viol) == 0:
        other = coll
    elif len(free) == 0:
        other = viol
    else:
        other = np.concatenate([coll, viol])
    rows = (lambda a: np.stack([a // inner, a % inner], 1)) if inner else (lambda a: a.reshape(-1, 1))
    return rows(free), rows(other)


def partial_rows(flags, hi, rng, poison):
    """The per-wavefront partial flags that a via-point launch over trajectories of `hi` interpolated samples leaves for the
    partition kernel, built by hand (layout: ops._via_flags_offset, trk_via_partial_flags_bytes, the comment above k_traj_partition):
    uint8 (T, K), K = hi // 64 + 2.  Trajectory t is covered by the wavefronts floor(t hi / 64) .. floor(((t + 1) hi - 1) / 64); their
    nj bytes are the first entries of row t -- random subsets of flags[t]'s bits whose OR is flags[t], the full value sitting at a
    random one of them (every third trajectory: at the last one, the others zero) -- and the entries k >= nj, which the kernel must
    never read, hold `poison`."""
    flags = np.asarray(flags, np.uint8)
    T, K = len(flags), hi // 64 + 2
    t = np.arange(T, dtype=np.int64)
    nj = ((t + 1) * hi - 1) // 64 - (t * hi) // 64 + 1
    assert nj.min() >= 1 and nj.max() <= K
    rows = rng.integers(0, 4, (T, K)).astype(np.uint8) & flags[:, None]
    at = rng.integers(0, nj)
    last_only = t % 3 == 0                                       # every third trajectory: its LAST wavefront alone saw anything
    rows[last_only] = 0
    at[last_only] = nj[last_only] - 1
    rows[t, at] = flags
    rows[np.arange(K)[None, :] >= nj[:, None]] = poison
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def walk(rng, shape, step=0.05):
    """positions like a recorded trajectory: cumulative sums of N(0, step) increments along the horizon (axis -2), float32"""
    return np.cumsum(rng.standard_normal(shape) * step, axis=-2).astype(np.float32)


def quat_to_rot64(q):
    """rotation matrices (n,3,3) of wxyz quaternions (n,4), any norm, in fp64 (quaternion.py:102-120)"""
    q = np.asarray(q, np.float64)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    dc = 2.0 / (q ** 2).sum(-1)
    return np.stack([1 - dc * (y * y + z * z), dc * (x * y - z * w), dc * (x * z + y * w),
                     dc * (x * y + z * w), 1 - dc * (x * x + z * z), dc * (y * z - x * w),
                     dc * (x * z - y * w), dc * (y * z + x * w), 1 - dc * (x * x + y * y)], -1).reshape(-1, 3, 3)


def random_frames(rng, n):
    """n proper rotations (from normalised random quaternions, rounded to float32) and translations uniform in [-2, 2]"""
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return quat_to_rot64(q).astype(np.float32), rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)


# path metric -------------------------------------------------------------------------------------------------------------------
METRIC_H = (1, 2, 257, 258, 600)
METRIC_COLS = ((14, 7, 7), (7, 0, 7), (5, 2, 1), (3, 0, 3))          # (S, c0, D)
METRIC_B = (1, 70)
METRIC_TOL = 2e-6                                                    # test_trajectory_metrics_like_the_reference


def metric_input(B, H, S):
    return walk(np.random.default_rng(1000 * H + 10 * S + B), (B, H, S))


# GP prior ----------------------------------------------------------------------------------------------------------------------
GP_CONFIG5 = (5.0 / 128, 0.1, 1.0)                                   # (dt, sigma, weight) of BASELINE config 5
GP_MILD = (0.05, 0.3, 1.0)
# (B, H, D), parameters, what the shape is there for
GP_LONG = (((2, 700, 22), GP_CONFIG5, "123 KB of LDS, 16-byte path"),
           ((2, 701, 13), GP_MILD, "73 KB of LDS, H D odd: element path"),
           ((1, 5119, 4), GP_CONFIG5, "163 824 B of LDS: the largest trajectory that fits"))
GP_SMALL = (((4, 2, 1), GP_MILD), ((4, 2, 1), GP_CONFIG5), ((1, 2, 7), GP_MILD), ((1, 2, 7), GP_CONFIG5))
GP_TOO_LONG = (1, 5120, 4)                                           # 163 856 B
GP_MISALIGNED = ((3, 16, 7), (3, 64, 4))                             # H D a multiple of 4, pointers one element off 16-byte alignment
GP_TOL_COST, GP_TOL_GRAD = 2e-5, 1e-4                                # test_gp_prior_vs_fp64_oracle


def gp_input(shape):
    """positions / velocities with the statistics of test_gp_prior_vs_fp64_oracle: cumulative N(0, 0.05) steps, N(0, 0.3) velocities"""
    rng = np.random.default_rng(sum(k * v for k, v in zip((1, 10, 100000), shape)))
    return walk(rng, shape), (rng.standard_normal(shape) * 0.3).astype(np.float32)


# partition -----------------------------------------------------------------------------------------------------------------------
PARTIAL_HI = (1, 63, 64, 447, 448, 630)                              # K = 2, 2, 3, 8, 9, 11
PARTIAL_T = ((70, 0), (5003, 0), (33000, 0), (5004, 4))              # (T, inner)
PARTIAL_MIX = {"mixed": (0.4, 0.3), "none_free": (1.0, 0.2), "only_violators": (0.5, 1.0)}      # test_device_side_trajectory_partition
VIA_CASES = ((37, 64, 10), (40, 100, 7), (33000, 3, 2), (9, 65, 7))  # (T, H, n): hi = 630, 693, 4, 448


def partial_case(T, hi, mix):
    """(coll_any, outside, flags, rng) of one hand-built case"""
    rng = np.random.default_rng(T * 1000 + hi + 7 * len(mix))
    p_c, p_o = PARTIAL_MIX[mix]
    coll_any, outside = rng.random(T) < p_c, rng.random(T) < p_o
    return coll_any, outside, coll_any.astype(np.uint8) | (outside.astype(np.uint8) << 1), rng


def via_case(T, H, lo, hi, rng):
    """The trajectories of test_trajectory_flags_folded_into_the_via_launch (same construction): states of 7 positions + 7
    velocities, smooth walks inside the limits [lo, hi], a fifth of them with one way point outside (or NaN), also the last one.
    -> (x (T, H, 14) float32, viol (T,) bool)"""
    x = np.zeros((T, H, 14), np.float32)
    base = rng.uniform(lo * 0.5, hi * 0.5, size=(T, 1, 7))
    x[..., :7] = np.clip(base + np.cumsum(rng.standard_normal((T, H, 7)) * 0.01, axis=1), lo + 1e-3, hi - 1e-3)
    x[..., 7:] = rng.standard_normal((T, H, 7)) * 100.0          # velocities are not positions: never tested against the limits
    viol = rng.random(T) < 0.2
    for t in np.nonzero(viol)[0]:
        hh, d = (H - 1 if t % 3 == 0 else rng.integers(0, H)), rng.integers(0, 7)
        x[t, hh, d] = hi[d] + 0.01 if t % 2 else (np.nan if t % 5 == 0 else lo[d] - 0.01)
    return x, viol


# frame algebra -------------------------------------------------------------------------------------------------------------------
FRAME_N = (1, 63, 257, 1000)
POINTS_N, POINTS_P = (1, 257, 1000), (1, 14, 65)
ROT_N = (257, 1000)
TOL_ROT, TOL_TRANS, TOL_ADJ, TOL_TP_ADJ, TOL_BCAST = 1e-6, 2e-6, 5e-6, 1e-5, 2e-5       # test_frame_algebra_vs_reference_golden
TOL_AXIS, TOL_AXIS_ADJ = 3e-7, 2e-6                                                     # test_rotation_builders_and_frame_constructor
TOL_QUAT, TOL_EULER = 1e-6, 5e-6
QUAT_NORMS = (1e-3, 1.0, 1e3)


def frame_case(n, seed=0):
    """two batches of n frames and unit-normal adjoint weights of a result: dict of float32 arrays"""
    rng = np.random.default_rng(4000 + n + seed)
    Ra, ta = random_frames(rng, n)
    Rb, tb = random_frames(rng, n)
    return dict(Ra=Ra, ta=ta, Rb=Rb, tb=tb, wR=rng.standard_normal((n, 3, 3)).astype(np.float32),
                wt=rng.standard_normal((n, 3)).astype(np.float32))


def points_case(n, P):
    rng = np.random.default_rng(5000 + 100 * n + P)
    R, t = random_frames(rng, n)
    return dict(R=R, t=t, pts=rng.uniform(-2.0, 2.0, (P, 3)).astype(np.float32), w=rng.standard_normal((n, P, 3)).astype(np.float32))


def angle_case(n):
    """angles uniform in [-20, 20] rad, the first five exactly 0, +-pi/2, +-pi (as float32 holds them), and adjoint weights"""
    rng = np.random.default_rng(6000 + n)
    a = rng.uniform(-20.0, 20.0, n).astype(np.float32)
    a[:5] = np.asarray([0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi], np.float32)
    return a, rng.standard_normal((n, 3, 3)).astype(np.float32)


def axis_rotation_adjoint64(R_shifted, kind, w):
    """d <w, R(a)> / d a from R(a + pi/2): the derivative of an axis rotation is the rotation a quarter turn on, without the 1 on
    its axis.  R_shifted (n,3,3) fp64."""
    dR = np.array(R_shifted, np.float64)
    dR[:, kind, kind] = 0.0
    return (dR * np.asarray(w, np.float64)).sum((1, 2))


def quat_case(n=1000):
    """wxyz quaternions in three groups of norm 1e-3, 1 and 1e3 (group = index % 3), and adjoint weights"""
    rng = np.random.default_rng(7000 + n)
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q *= np.asarray(QUAT_NORMS)[np.arange(n) % 3, None]
    return q.astype(np.float32), rng.standard_normal((n, 3, 3)).astype(np.float32)


def quat_rotation_torch(q):
    """quaternion.py:102-120 as the reference writes it, in q's dtype (differentiable)"""
    qw, qx, qy, qz = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    dc = 2.0 / (q ** 2).sum(-1)
    return torch.stack([1 - dc * (qy * qy + qz * qz), dc * (qx * qy - qz * qw), dc * (qx * qz + qy * qw),
                        dc * (qx * qy + qz * qw), 1 - dc * (qx * qx + qz * qz), dc * (qy * qz - qx * qw),
                        dc * (qx * qz - qy * qw), dc * (qy * qz + qx * qw), 1 - dc * (qx * qx + qy * qy)], -1).reshape(q.shape[:-1] + (3, 3))


def quat_grad_ref(q, w, dtype=torch.float64):
    """(R, d <w, R(q)> / d q) by torch autograd on the CPU in `dtype`"""
    qt = torch.as_tensor(np.asarray(q), dtype=dtype).requires_grad_(True)
    R = quat_rotation_torch(qt)
    (R * torch.as_tensor(np.asarray(w), dtype=dtype)).sum().backward()
    return R.detach().numpy(), qt.grad.numpy()


def quat_grad_expression(got, ref):
    """the expression of test_quaternion_and_euler_gradients_flow_like_the_reference (< 1e-4 passes there)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (np.abs(ref) + 1e-3 * np.abs(ref).max())).max())


def rel_to(a, ref):
    """max |a - ref| / max(1, max |ref|)"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a.reshape(ref.shape) - ref).max() / max(1.0, np.abs(ref).max()))


def quat_euler_case(n=257):
    return random_frames(np.random.default_rng(8000 + n), n)[0]
