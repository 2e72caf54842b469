"""Trajectory post-processing on the GPU (csrc/trk_traj_post.hip).  trk_traj_spline_resample against the reference's recorded results
(tests/golden/traj_post.npz) and the fp64 restatement spline64 of traj_post_helpers (validated on the CPU: test_traj_post_cpu.py)
within C_P 2^-24 mag (positions) and C_V 2^-24 mag (N - 1) (the derivative), its bit properties, the independence of a trajectory's
bits from its place in the batch, the isolation of a NaN to its column, the buffers' edges, one captured replay, and the Python
route.  trk_traj_waypoint_variance against the goldens and variance64 within 4 (dim + 4) 2^-24 relative, its reproducibility, and
one captured replay.  Every element of every case is compared."""
from pathlib import Path

import numpy as np
import pytest
import torch

import torch_robotics_amd as tra
import traj_post_helpers as tp
from torch_robotics_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TA = dict(device=DEV, dtype=torch.float32)
ROOT = Path(__file__).resolve().parent.parent
MODE_NAMES = {0: "zero", 1: "average", 2: "spline"}
NS, SS, DS = (2, 3, 4, 5, 64, 65, 256), (2, 3, 30, 64, 257, 1024), (1, 3, 7, 8, 9, 32)


@pytest.fixture(scope="module")
def golden():
    with np.load(ROOT / "tests" / "golden" / "traj_post.npz") as z:
        return {k: z[k] for k in z.files}


def dev(a):
    return torch.as_tensor(np.array(a, order="C"), device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return (host(t) if isinstance(t, torch.Tensor) else np.asarray(t, np.float32)).view(np.uint32)


def paths(seed, n, N, D):
    """n paths: random walks, every second one with an O(3) offset"""
    rng = np.random.default_rng(seed)
    y = np.cumsum(0.3 * rng.standard_normal((n, N, D)), 1)
    y[1::2] += 3.0
    return y.astype(np.float32)


def check_spline(y, S, pos, vel, what, ref=None):
    """positions and the derivative of the spline mode against spline64 (or `ref`), every element; -> the worst ratios"""
    N = y.shape[-2]
    p64, v64 = tp.spline64(y, S, "spline") if ref is None else ref
    mag = tp.column_mag(y)
    ep = np.abs(host(pos).astype(np.float64) - p64)
    worst = [float((ep / (tp.EPS * np.maximum(mag, 1e-300))).max()), 0.0]
    assert (ep <= tp.C_P * tp.EPS * mag).all(), what
    if vel is not None:
        ev = np.abs(host(vel).astype(np.float64) - v64)
        worst[1] = float((ev / (tp.EPS * np.maximum(mag, 1e-300) * (N - 1))).max())
        assert (ev <= tp.C_V * tp.EPS * mag * (N - 1)).all(), what
    return worst


# spline 1 ---------------------------------------------------------------------------------------------------------------------
def test_spline_goldens_from_the_reference(golden):
    """the reference's own smoothen_trajectory (fp64): positions within C_P 2^-24 mag; vel_mode 0 exactly zero, vel_mode 1 bit for bit
    its formula and within 2 x 2^-24 relative of the reference (S dt and the quotient are each rounded once), vel_mode 2 within
    C_V 2^-24 mag (N - 1); and the same cases against the fp64 restatement"""
    worst = [0.0, 0.0]
    for k in range(int(golden["spline/n"])):
        y = golden[f"spline/{k}/y"]
        S, mode, _ = (int(v) for v in golden[f"spline/{k}/meta"])
        dt = float(golden[f"spline/{k}/dt"])
        pos, vel = ops.traj_spline_resample(dev(y), S, MODE_NAMES[mode], dt)
        assert pos.shape == vel.shape == (S, y.shape[1])
        gp, gv = golden[f"spline/{k}/pos"], golden[f"spline/{k}/vel"]
        w = check_spline(y, S, pos, vel if mode == 2 else None, f"golden {k}", ref=(gp, gv))
        worst = [max(a, b) for a, b in zip(worst, w)]
        check_spline(y, S, pos, vel if mode == 2 else None, f"golden {k} against spline64")
        if mode == 0:
            assert (bits(vel) == 0).all()
        if mode == 1:
            assert np.array_equal(bits(vel), bits(tp.spline32(y, S, "average", dt)[1])), k
            assert (np.abs(host(vel) - gv) <= 2 * tp.EPS * np.abs(gv)).all(), k
    print(f"  goldens: worst position ratio {worst[0]:.3f}, worst velocity ratio {worst[1]:.3f}")


# spline 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
def test_spline_against_the_fp64_restatement(N):
    """every (S, D) of the grid at this N, batches of 1 and 3 trajectories: positions, the derivative, and the bit properties --
    endpoints, a constant column, the end rows of the derivative, the average rows against their formula"""
    worst = [0.0, 0.0]
    for S in SS:
        for D in DS:
            for n in (1, 3):
                y = paths(N * 1000 + S * 10 + D + n, n, N, D)
                const = (slice(None), D // 2) if D > 1 else (slice(0, n - 1), 0)      # a constant column (D = 1: a constant trajectory)
                y[const[0], :, const[1]] = y[const[0], :1, const[1]]
                pos, vel = ops.traj_spline_resample(dev(y), S, "spline")
                assert pos.shape == vel.shape == (n, S, D)
                w = check_spline(y, S, pos, vel, f"N={N} S={S} D={D} n={n}")
                worst = [max(a, b) for a, b in zip(worst, w)]
                assert np.array_equal(bits(pos[:, 0]), bits(y[:, 0])) and np.array_equal(bits(pos[:, -1]), bits(y[:, -1]))
                assert np.array_equal(bits(pos[const[0], :, const[1]]), np.broadcast_to(bits(y[const[0], :1, const[1]]), (len(y[const[0]]), S)))
                assert (bits(vel[:, 0]) == 0).all() and (bits(vel[:, -1]) == 0).all()
                if (S - 1) % (N - 1) == 0:
                    assert np.array_equal(bits(pos[:, ::(S - 1) // (N - 1)]), bits(y))
            pa, va = ops.traj_spline_resample(dev(y), S, "average", 0.1)
            assert torch.equal(pa, pos) and np.array_equal(bits(va), bits(tp.spline32(y, S, "average", 0.1)[1]))
            pz, vz = ops.traj_spline_resample(dev(y), S, "zero")
            assert torch.equal(pz, pos) and (bits(vz) == 0).all()
    print(f"  N={N}: worst position ratio {worst[0]:.3f}, worst velocity ratio {worst[1]:.3f}")


# spline 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S", [(5, 9), (64, 127), (4, 10), (256, 256)])
def test_spline_knots_are_the_inputs_bits(N, S):
    y = paths(N + S, 4, N, 7)
    pos, _ = ops.traj_spline_resample(dev(y), S, "spline")
    assert (S - 1) % (N - 1) == 0
    assert np.array_equal(bits(pos[:, ::(S - 1) // (N - 1)]), bits(y))


# spline 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,D,n", [(4, 5, 1, 513), (4, 5, 3, 2049), (64, 64, 7, 515), (256, 30, 32, 3), (65, 257, 9, 7), (17, 30, 7, 1030), (4, 5, 7, 18500)])
def test_a_trajectorys_bits_depend_only_on_its_own_inputs(N, S, D, n):
    """batches one more (and a few more) than whole workgroup tiles -- the tile grows with the batch from 512 trajectories on, so the
    last workgroup is ragged; at 18500 x 7 a workgroup has more columns than lanes -- against: some trajectories alone, the batch in two calls, and the batch behind other trajectories;
    and against the fp64 restatement"""
    y = paths(n + N, n, N, D)
    pos, vel = ops.traj_spline_resample(dev(y), S, "spline")
    check_spline(y, S, pos, vel, f"N={N} S={S} D={D} n={n}")
    for j in (0, 1, n // 2, n - 1):
        p1, v1 = ops.traj_spline_resample(dev(y[j:j + 1]), S, "spline")
        assert torch.equal(p1[0], pos[j]) and torch.equal(v1[0], vel[j]), j
    cut = n // 3 + 1
    for a, b in ((0, cut), (cut, n)):
        p2, v2 = ops.traj_spline_resample(dev(y[a:b]), S, "spline")
        assert torch.equal(p2, pos[a:b]) and torch.equal(v2, vel[a:b])
    p3, v3 = ops.traj_spline_resample(dev(np.concatenate([paths(9, 5, N, D), y], 0)), S, "spline")
    assert torch.equal(p3[5:], pos) and torch.equal(v3[5:], vel)


# spline 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", (np.nan, np.inf))
def test_a_non_finite_value_poisons_its_own_column_and_nothing_else(bad):
    for N, S, D, n in ((64, 127, 7, 5), (3, 30, 3, 3), (256, 64, 32, 2), (17, 30, 1, 600)):
        y = paths(N + D, n, N, D)
        pos, vel = ops.traj_spline_resample(dev(y), S, "spline")
        j, i, d = n // 2, N // 2, D // 2
        y2 = y.copy()
        y2[j, i, d] = bad
        pos2, vel2 = ops.traj_spline_resample(dev(y2), S, "spline")
        keep = np.ones((n, S, D), bool)
        keep[j, :, d] = False
        assert np.array_equal(bits(pos2)[keep], bits(pos)[keep]) and np.array_equal(bits(vel2)[keep], bits(vel)[keep])
        assert not np.isfinite(host(pos2)[j, :, d]).all()


# spline 6 ---------------------------------------------------------------------------------------------------------------------
def off_boundary(a, pad=64, fill=-777.25):
    """a copy of `a` inside a larger sentinel-filled buffer, starting 4 bytes past a 16-byte boundary -> (view, whole buffer)"""
    n = int(np.prod(a.shape))
    whole = torch.full((pad + 1 + n + pad,), fill, **TA)
    assert whole.data_ptr() % 16 == 0
    view = whole[pad + 1:pad + 1 + n].view(a.shape)
    view.copy_(dev(a))
    assert view.data_ptr() % 16 == 4
    return view, whole


def raw_spline(y, n, N, D, S, mode, dt, pos, vel):
    with torch.cuda.device(DEV):
        rc = _lib.lib().trk_traj_spline_resample(y.data_ptr(), n, N, D, S, mode, dt, pos.data_ptr(), None if vel is None else vel.data_ptr(),
                                                 ops._stream_of(DEV))
    assert rc == 0, _lib.lib().trk_last_error().decode()


@pytest.mark.parametrize("N,S,D,n", [(3, 2, 1, 1), (64, 127, 7, 3), (256, 1024, 32, 2), (5, 30, 9, 700)])
def test_sentinels_around_pos_and_vel_off_a_sixteen_byte_boundary(N, S, D, n):
    y = paths(N * S, n, N, D)
    for mode in (0, 1, 2):
        ref_p, ref_v = ops.traj_spline_resample(dev(y), S, MODE_NAMES[mode], 0.05)
        yv, _ = off_boundary(y)
        (pos, p_all), (vel, v_all) = (off_boundary(np.zeros((n, S, D), np.float32)) for _ in range(2))
        raw_spline(yv, n, N, D, S, mode, 0.05, pos, vel)
        torch.cuda.synchronize()
        assert torch.equal(pos, ref_p) and torch.equal(vel, ref_v)
        m = n * S * D
        for whole in (p_all, v_all):
            edge = torch.cat([whole[:65], whole[65 + m:]])
            assert edge.numel() == 129 and (edge == -777.25).all()
    # vel = NULL with vel_mode 0: positions only
    pos, p_all = off_boundary(np.zeros((n, S, D), np.float32))
    raw_spline(dev(y), n, N, D, S, 0, 0.05, pos, None)
    torch.cuda.synchronize()
    assert torch.equal(pos, ops.traj_spline_resample(dev(y), S, "zero")[0])
    assert (torch.cat([p_all[:65], p_all[65 + n * S * D:]]) == -777.25).all()


# spline 7 ---------------------------------------------------------------------------------------------------------------------
def test_one_replay_of_a_captured_resampling_equals_the_eager_result():
    y = dev(paths(3, 40, 64, 7))
    work = lambda: ops.traj_spline_resample(y, 256, "spline")
    eager = work()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = work()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, eager):
        assert torch.equal(a, b)


# spline 8 ---------------------------------------------------------------------------------------------------------------------
def test_smoothen_trajectory_batched_equals_per_trajectory_and_follows_the_reference(golden):
    y = paths(11, 6, 17, 7).reshape(2, 3, 17, 7)
    for kw in (dict(), dict(set_average_velocity=False, zero_velocity=True), dict(set_average_velocity=False)):
        pos, vel = tra.smoothen_trajectory(dev(y), n_support_points=30, dt=0.1, **kw)
        assert pos.shape == vel.shape == (2, 3, 30, 7) and pos.device == DEV
        for a in range(2):
            for b in range(3):
                p1, v1 = tra.smoothen_trajectory(dev(y[a, b]), n_support_points=30, dt=0.1, **kw)
                assert p1.shape == (30, 7) and torch.equal(p1, pos[a, b]) and torch.equal(v1, vel[a, b])
    # a host path comes back on the host; tensor_args moves and casts; one support point is answered without a launch
    p, v = tra.smoothen_trajectory(torch.from_numpy(y[0, 0]), n_support_points=30, dt=0.1)
    assert p.device.type == "cpu" and torch.equal(p, tra.smoothen_trajectory(dev(y[0, 0]), 30, 0.1)[0].cpu())
    p, v = tra.smoothen_trajectory(y[0, 0], n_support_points=30, tensor_args=dict(device=DEV, dtype=torch.float64))
    assert p.dtype == torch.float64 and p.device == DEV
    p, v = tra.smoothen_trajectory(dev(y), n_support_points=1)
    assert torch.equal(p, dev(y)[..., :1, :]) and v.shape == p.shape and (v == 0).all()
    # a golden case through the reference's signature
    k = 13
    gy, (S, mode, _) = golden[f"spline/{k}/y"], (int(v) for v in golden[f"spline/{k}/meta"])
    assert mode == 1
    p, v = tra.smoothen_trajectory(dev(gy), n_support_points=S, dt=float(golden[f"spline/{k}/dt"]))
    check_spline(gy, S, p, None, "golden through smoothen_trajectory", ref=(golden[f"spline/{k}/pos"], None))
    assert (np.abs(host(v) - golden[f"spline/{k}/vel"]) <= 2 * tp.EPS * np.abs(golden[f"spline/{k}/vel"])).all()


# variance 1 -------------------------------------------------------------------------------------------------------------------
def check_variance(x, c0, dim, got, what):
    want = tp.variance64(x, c0, dim)
    got = host(got).astype(np.float64)
    K = x.shape[1]
    if K == 1:
        assert np.isnan(got).all() and np.isnan(want).all(), what
        return 0.0
    err = np.abs(got - want)
    assert (err <= tp.var_rtol(dim) * np.abs(want)).all(), (what, got, want)
    return float((err / (tp.var_rtol(dim) * np.abs(want))).max())


def test_variance_goldens_from_the_reference(golden):
    """the reference's value on fp64 inputs, the clustered set included: the |a|^2 + |b|^2 - 2 a.b route misses that one by 6e-3"""
    for k in range(int(golden["var/n"])):
        x, want = golden[f"var/{k}/x"], float(golden[f"var/{k}/value"])
        K, H, D = x.shape
        got = ops.traj_waypoint_variance(dev(x[None]), 0, D)
        assert got.shape == (1,)
        if K == 1:
            assert np.isnan(want) and torch.isnan(got).all()
        else:
            rel = abs(float(got[0]) - want) / abs(want)
            print(f"  golden {k} {x.shape}: relative error {rel:.2e} of {tp.var_rtol(D):.2e}")
            assert rel <= tp.var_rtol(D), k
        check_variance(x[None], 0, D, got, f"golden {k}")
    k = int(golden["var/clustered"])
    x = golden[f"var/{k}/x"]
    robot = type("R", (), {"q_dim": 3})()
    v = tra.compute_variance_waypoints(dev(x), robot)
    assert v.dim() == 0 and abs(float(v) - float(golden[f"var/{k}/value"])) <= tp.var_rtol(3) * float(golden[f"var/{k}/value"])


@pytest.mark.parametrize("K", (1, 2, 3, 64, 65, 257))
def test_variance_against_the_fp64_restatement(K):
    """H in {1, 3, 64}, D in {1, 3, 7, 32}, the positions at c0 = 0 of state_dim = D and at c0 = D of state_dim = 2 D, P in {1, 5}"""
    rng = np.random.default_rng(K)
    worst = 0.0
    for H in (1, 3, 64):
        for D in (1, 3, 7, 32):
            if K == 257 and H == 64 and D != 7:
                continue                                                    # the host's fp64 pair loop: K = 257 has H = 64 at D = 7
            for P, c0 in ((1, 0), (5, D)):
                x = (rng.standard_normal((P, 1, H, c0 + D)) + 0.5 * rng.standard_normal((P, K, H, c0 + D))).astype(np.float32)
                got = ops.traj_waypoint_variance(dev(x), c0, D)
                assert got.shape == (P,)
                worst = max(worst, check_variance(x, c0, D, got, f"K={K} H={H} D={D} P={P} c0={c0}"))
    print(f"  K={K}: worst relative error / (4 (dim + 4) 2^-24) = {worst:.3f}")


@pytest.mark.parametrize("D", (2, 4, 5, 8, 9, 16, 17))
def test_variance_at_the_widths_where_the_launch_takes_another_instantiation(D):
    """the pair kernel keeps a position in 2, 4, 8, 16 or 32 registers: both sides of every step, two tiles with a ragged second"""
    x = np.random.default_rng(D).standard_normal((2, 70, 2, D + 1)).astype(np.float32)
    check_variance(x, 1, D, ops.traj_waypoint_variance(dev(x), 1, D), f"D={D}")


def test_variance_is_reproducible_and_a_problem_stays_on_its_own():
    rng = np.random.default_rng(5)
    for K, H, D in ((65, 3, 7), (8, 64, 7), (257, 2, 3)):
        x = rng.standard_normal((5, K, H, 2 * D)).astype(np.float32)
        x[1, 3] = x[1, 0]                                                   # duplicate particles: some d_ij = 0
        x[1, K - 1] = x[1, 0]
        a = ops.traj_waypoint_variance(dev(x), D, D)
        b = ops.traj_waypoint_variance(dev(x), D, D)
        assert torch.equal(a, b)
        check_variance(x, D, D, a, f"duplicates K={K}")
        for p in range(5):
            assert torch.equal(ops.traj_waypoint_variance(dev(x[p:p + 1]), D, D)[0], a[p]), p
        assert torch.equal(ops.traj_waypoint_variance(dev(x[2:]), D, D), a[2:])
        x2 = x.copy()
        x2[3, K // 2, H // 2, D + 1] = np.inf
        c = ops.traj_waypoint_variance(dev(x2), D, D)
        keep = np.arange(5) != 3
        assert np.array_equal(bits(c)[keep], bits(a)[keep]) and not np.isfinite(host(c)[3])
    # all particles equal: every distance is 0, the variance exactly 0
    x = np.broadcast_to(rng.standard_normal((2, 1, 4, 3)).astype(np.float32), (2, 9, 4, 3))
    assert (bits(ops.traj_waypoint_variance(dev(x), 0, 3)) == 0).all()


def test_one_replay_of_a_captured_variance_equals_the_eager_result():
    x = dev(np.random.default_rng(2).standard_normal((3, 70, 16, 14)).astype(np.float32))
    work = lambda: ops.traj_waypoint_variance(x, 0, 7)
    eager = work()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = work()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)
