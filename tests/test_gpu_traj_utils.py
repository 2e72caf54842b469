"""The streaming trajectory kernels of csrc/trk_kernels.hip off their recorded shapes: k_interpolate_via_points(_flat),
k_finite_difference, k_traj_diff_norm_sum, k_gp_prior, k_traj_flags and k_traj_partition against exact numpy restatements or the fp64
oracle (tests/traj_utils_helpers.py; test_traj_utils_refs_cpu.py checks those references and every borrowed tolerance on the CPU).
Reference code: trajectory/utils.py:37-64, trajectory/metrics.py:7-35, tasks.py:244-299."""
import numpy as np
import pytest
import torch

import traj_utils_helpers as th
from helpers import gold, model, panda_cost_spec, rel_err
from torch_robotics_amd._abi import FIELD_OBJECTS, FIELD_SELF, FIELD_WS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def dev(a):
    return torch.as_tensor(a, device=DEV)


@pytest.fixture(scope="module")
def ops():
    from torch_robotics_amd import ops as o
    return o


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. interpolation: bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
def _interp_equal(ops, x, n):
    out = ops.interpolate_traj_via_points(dev(x), n)
    ref = th.interp_ref(x, n)
    assert out.shape == ref.shape
    np.testing.assert_array_equal(out.cpu().numpy(), ref, err_msg=f"x {x.shape}, n = {n}")


@pytest.mark.parametrize("D", [1, 2, 3, 7, 9, 14])
def test_interpolation_grid_is_exact(ops, D):
    """the reciprocal divisions of the LDS kernel (trk_div_small by D and by n) at other divisors than 7 and 3 / 5, the shortest
    horizons, one and several trajectories, a 4-D batch"""
    rng = np.random.default_rng(100 + D)
    for n in (1, 2, 3, 7, 10):
        for H in (2, 3, 17, 64):
            for T in (1, 5):
                _interp_equal(ops, rng.standard_normal((T, H, D)).astype(np.float32), n)
            _interp_equal(ops, rng.standard_normal((2, 3, H, D)).astype(np.float32), n)


def test_interpolation_at_the_end_of_the_reciprocal_division_range(ops):
    """One x, two n: 4 187 190 output elements per trajectory (< 2^22: reciprocal + fix-up at its largest operands) and 4 198 180
    (>= 2^22: the integer divisions, a branch nothing else reaches).  LDS 47 036 / 47 044 B: still the LDS kernel."""
    x = np.random.default_rng(1571).standard_normal((2, 1571, 7)).astype(np.float32)
    for n in (381, 382):
        assert (1570 * n * 7 < 2 ** 22) == (n == 381) and 4 * (1571 * 7 + 2 * n) <= 48 * 1024
        _interp_equal(ops, x, n)


def test_interpolation_on_both_sides_of_the_lds_switch(ops):
    """H D + 2 n = 12288 floats = 48 KB exactly: the LDS kernel; 12290: the element-per-thread kernel"""
    rng = np.random.default_rng(6139)
    for H in (6139, 6140):
        _interp_equal(ops, rng.standard_normal((2, H, 2)).astype(np.float32), 5)


def test_flat_interpolation_kernel_against_the_reference(ops):
    """the element-per-thread kernel (a trajectory too large for LDS) against numpy, not against the other kernel"""
    assert 4 * (2100 * 7 + 6) > 48 * 1024
    _interp_equal(ops, np.random.default_rng(2100).standard_normal((3, 2100, 7)).astype(np.float32), 3)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. finite differences: bit for bit, also where the division rounds
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0.25, 0.1, 5.0 / 128])
@pytest.mark.parametrize("method", th.FD_METHODS)
def test_finite_differences_are_exact(ops, method, dt):
    """dt = 0.1 is no power of two: the quotient is rounded, and a reciprocal multiply instead of the division would show.  Horizons
    without an interior (1, 2, 3), ragged last workgroups (B H D no multiple of 256), a 4-D batch."""
    rng = np.random.default_rng(int(dt * 1e4) + len(method))
    for H in (1, 2, 3, 64, 257):
        for D in (1, 3, 14):
            for lead in ((1,), (37,), (2, 3)):
                x = rng.standard_normal(lead + (H, D)).astype(np.float32)
                out = ops.finite_difference(dev(x), dt=dt, method=method).cpu().numpy()
                np.testing.assert_array_equal(out, th.fd_ref(x, dt, method), err_msg=f"{lead} {H} {D}")
                if H == 1 or (H == 2 and method == "central"):
                    assert not out.any()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. path metric
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", th.METRIC_H)
def test_path_metric_vs_fp64_oracle(ops, oracle_lib, H):
    """H > 257: the 256-thread loop over the steps makes a second trip; column windows with and without an offset"""
    for S, c0, D in th.METRIC_COLS:
        for B in th.METRIC_B:
            x = th.metric_input(B, H, S)
            got = ops.traj_diff_norm_sum(dev(x), c0, D).cpu().numpy()
            ref = oracle_lib.traj_diff_norm_sum(x.astype(np.float64), c0, D, "f64")
            assert got.shape == (B,)
            if H == 1:
                assert not got.any() and not ref.any()
            else:
                assert ref.min() > 0 and rel_err(got, ref) < th.METRIC_TOL, (S, c0, D, B)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. GP prior
# ---------------------------------------------------------------------------------------------------------------------------------
def _gp_check(ops, oracle_lib, shape, dt, sigma, w):
    q, qd = th.gp_input(shape)
    rc, rgq, rgqd = oracle_lib.gp_prior(q.astype(np.float64), qd.astype(np.float64), dt, sigma, w, "f64")
    c, gq, gqd = ops.gp_prior_cost_grad(dev(q), dev(qd), dt, sigma, w)
    assert c.shape == shape[:1] and gq.dtype == torch.float32
    assert rel_err(c.cpu().numpy(), rc) < th.GP_TOL_COST
    assert rel_err(gq.cpu().numpy(), rgq) < th.GP_TOL_GRAD and rel_err(gqd.cpu().numpy(), rgqd) < th.GP_TOL_GRAD
    # accumulate mode: added to what the buffers hold
    rng = np.random.default_rng(shape[1])
    g0, g1 = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    a0, a1 = dev(g0), dev(g1)
    ca, _, _ = ops.gp_prior_cost_grad(dev(q), dev(qd), dt, sigma, w, accumulate_into=(a0, a1))
    assert torch.equal(ca, c)
    assert rel_err(a0.cpu().numpy(), g0.astype(np.float64) + rgq) < th.GP_TOL_GRAD
    assert rel_err(a1.cpu().numpy(), g1.astype(np.float64) + rgqd) < th.GP_TOL_GRAD
    # fp16 I/O with the loss scale of gp_grad_scale: the oracle sees the fp16-rounded inputs; the bound is the fp16 expression of
    # test_gp_prior_vs_fp64_oracle (one fp16 rounding of the scaled value + fp32 arithmetic)
    qh, qdh = dev(q).half(), dev(qd).half()
    rc, rgq, rgqd = oracle_lib.gp_prior(qh.cpu().numpy().astype(np.float64), qdh.cpu().numpy().astype(np.float64), dt, sigma, w, "f64")
    gs = ops.gp_grad_scale(dt, sigma, w, float(qh.abs().max()), float(qdh.abs().max()))
    c, gq, gqd = ops.gp_prior_cost_grad(qh, qdh, dt, sigma, w, grad_scale=gs)
    assert gq.dtype == torch.float16 and gqd.dtype == torch.float16 and c.dtype == torch.float32
    assert rel_err(c.cpu().numpy(), rc) < th.GP_TOL_COST
    assert torch.isfinite(gq.float()).all() and torch.isfinite(gqd.float()).all()
    assert np.abs(rgq).max() * gs < 65504 and np.abs(rgqd).max() * gs < 65504
    for got, ref in ((gq, rgq), (gqd, rgqd)):
        err = np.abs(got.float().cpu().numpy().astype(np.float64) / gs - ref)
        assert (err <= 2.0 ** -10 * np.abs(ref) + 2.0 ** -24 / gs + 2e-5 * np.abs(ref).max()).all()
    # ... and accumulated into a scaled fp16 gradient: one more fp16 rounding
    base16 = (torch.as_tensor(g0, device=DEV) * 3.0 * gs).half()
    a0, a1 = base16.clone(), torch.zeros_like(base16)
    ops.gp_prior_cost_grad(qh, qdh, dt, sigma, w, accumulate_into=(a0, a1), grad_scale=gs)
    ref = base16.double().cpu().numpy() / gs + rgq
    err = np.abs(a0.double().cpu().numpy() / gs - ref)
    assert torch.isfinite(a0.float()).all() and (err <= 2.0 ** -9 * (np.abs(ref) + np.abs(rgq)) + 2.0 ** -23 / gs + 4e-5 * np.abs(rgq).max()).all()
    assert torch.equal(a1, gqd)                                   # added to zeros: the plain result


@pytest.mark.parametrize("shape,params,why", th.GP_LONG, ids=[str(s) for s, _, _ in th.GP_LONG])
def test_gp_prior_long_trajectories(ops, oracle_lib, shape, params, why):
    """more than 64 KB of LDS per workgroup, up to the last trajectory that fits the 160 KiB the launcher accepts"""
    B, H, D = shape
    assert 64 * 1024 < 4 * (2 * ((H * D + 3) & ~3) + 4) <= 160 * 1024
    _gp_check(ops, oracle_lib, shape, *params)


@pytest.mark.parametrize("shape,params", th.GP_SMALL, ids=[f"{s}-{p[1]}" for s, p in th.GP_SMALL])
def test_gp_prior_smallest_shapes(ops, oracle_lib, shape, params):
    """D = 1 and H = 2: one factor per trajectory, every element has one neighbour only"""
    _gp_check(ops, oracle_lib, shape, *params)


def test_gp_prior_refuses_a_trajectory_beyond_the_lds(ops):
    """163 856 B: a host refusal -- no kernel runs, nothing is written"""
    B, H, D = th.GP_TOO_LONG
    assert 4 * (2 * H * D + 4) > 160 * 1024
    q, qd = torch.zeros(B, H, D, device=DEV), torch.zeros(B, H, D, device=DEV)
    a0, a1 = torch.full((B, H, D), 7.0, device=DEV), torch.full((B, H, D), -3.0, device=DEV)
    with pytest.raises(NotImplementedError, match="must fit the 160 KiB LDS"):
        ops.gp_prior_cost_grad(q, qd, 0.05, 0.3, accumulate_into=(a0, a1))
    with pytest.raises(NotImplementedError, match="must fit the 160 KiB LDS"):
        ops.gp_prior_cost_grad(q.half(), qd.half(), 0.05, 0.3)
    torch.cuda.synchronize()
    assert bool((a0 == 7.0).all()) and bool((a1 == -3.0).all())


@pytest.mark.parametrize("shape", th.GP_MISALIGNED, ids=str)
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_gp_prior_misaligned_views_equal_the_aligned_copy(ops, oracle_lib, shape, half):
    """H D is a multiple of 4 but q, qd and the accumulate buffers start one element into their allocations: the launcher must take
    the element path (a 16-byte access there would be misaligned), and cost and gradients must be those of the aligned copies, bit
    for bit -- the cost too: both paths give a thread the same elements in the same order (the element path once took them one per
    thread, and the cost of (3, 16, 7) differed from the aligned launch in its last bit)."""
    dt, sigma, w = th.GP_MILD
    q, qd = th.gp_input(shape)
    n = q.size
    dtype = torch.float16 if half else torch.float32
    rng = np.random.default_rng(n)
    g0, g1 = (rng.standard_normal(shape).astype(np.float32) for _ in range(2))

    def off_by_one(a):
        flat = torch.zeros(n + 1, device=DEV, dtype=dtype)
        view = flat[1:].view(shape)
        view.copy_(dev(a))
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        return view
    gs = ops.gp_grad_scale(dt, sigma, w) if half else 1.0
    aligned = [dev(a).to(dtype) for a in (q, qd, g0 * gs, g1 * gs)]
    assert all(a.data_ptr() % 16 == 0 for a in aligned)
    shifted = [off_by_one(a.float()) for a in aligned]
    res = []
    for qq, qqd, b0, b1 in (aligned, shifted):
        c, gq, gqd = ops.gp_prior_cost_grad(qq, qqd, dt, sigma, w, grad_scale=gs)
        ca, _, _ = ops.gp_prior_cost_grad(qq, qqd, dt, sigma, w, accumulate_into=(b0, b1), grad_scale=gs)
        assert torch.equal(c, ca)
        res.append((c, gq, gqd, b0, b1))
    for k in range(5):
        assert torch.equal(res[0][k], res[1][k]), k
    rc, _, _ = oracle_lib.gp_prior(aligned[0].double().cpu().numpy(), aligned[1].double().cpu().numpy(), dt, sigma, w, "f64")
    assert rel_err(res[1][0].cpu().numpy(), rc) < th.GP_TOL_COST


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. flags and partition
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_partition(part, x, coll_any, outside, inner):
    nf, nc, no = part.counts()
    assert (nf, nc, no) == (int((~coll_any & ~outside).sum()), int(coll_any.sum()), int((~coll_any & outside).sum()))
    np.testing.assert_array_equal(part.flags.cpu().numpy(), coll_any.astype(np.uint8) | (outside.astype(np.uint8) << 1))
    free_e, _ = th.partition_ref(coll_any, outside, inner)
    np.testing.assert_array_equal(part.idx[:nf].cpu().numpy(), free_e)
    # the kernel's second group is always [colliding | collision-free violators]; partition_ref's `other` list is that group cut the
    # way the task hands it out (test_device_side_trajectory_partition checks that cut through PlanningTask)
    rest = np.concatenate([np.flatnonzero(coll_any), np.flatnonzero(~coll_any & outside)])
    got = part.idx[nf:].cpu().numpy()
    np.testing.assert_array_equal(got[:, 0] * inner + got[:, 1] if inner else got[:, 0], rest)
    _, other_e = th.partition_ref(coll_any, outside, inner)
    np.testing.assert_array_equal(got if nf else (got[nc:] if no else got[:nc]), other_e)
    gathered = part.gathered.cpu().numpy()
    np.testing.assert_array_equal(gathered[:nf], x[~coll_any & ~outside])
    np.testing.assert_array_equal(gathered[nf:], x[rest])
    assert nf + nc + no == len(coll_any)


@pytest.mark.parametrize("T,H,n_interp", th.VIA_CASES)
def test_trajectory_flags_through_the_via_launch_at_long_trajectories(ops, T, H, n_interp):
    """test_trajectory_flags_folded_into_the_via_launch at more samples per trajectory (630, 693, 448: beyond the 8-entry rows of the
    partition's phase 0 and beyond one 512-way-point trip of k_traj_flags) and at more than 32768 trajectories (the assembled flags no
    longer stay in LDS)."""
    g, robot = gold("cost_spheres3d"), gold("panda_robot")
    m = model("panda_arm_no_gripper")
    h, cm = ops.ModelHandle(m), ops.CostHandle(panda_cost_spec(g, robot), DEV)
    lo, hi = np.asarray(m.lower[m.dof_idx >= 0], np.float32), np.asarray(m.upper[m.dof_idx >= 0], np.float32)
    lo, hi = lo[np.argsort(m.dof_idx[m.dof_idx >= 0])], hi[np.argsort(m.dof_idx[m.dof_idx >= 0])]
    x, viol = th.via_case(T, H, lo, hi, np.random.default_rng(T + H))
    xt, qmin, qmax = dev(x), dev(lo), dev(hi)
    fields = FIELD_SELF | FIELD_OBJECTS | FIELD_WS
    wp0 = ops.rollout_collision_via(h, cm, fields, xt, n_interp, margin=0.0)
    wp1, buf = ops.rollout_collision_via(h, cm, fields, xt, n_interp, margin=0.0, limits=(qmin, qmax))
    assert wp0.shape == (T, (H - 1) * n_interp) and torch.equal(wp0, wp1)
    ref = ops.traj_validate(wp0, xt, 7, qmin, qmax)
    got = ops.traj_validate(None, xt, 7, qmin, qmax, flags=buf)
    assert torch.equal(ref.flags, got.flags)
    expect = wp0.any(1).to(torch.uint8) | (dev(viol).to(torch.uint8) << 1)
    assert torch.equal(got.flags, expect)
    assert ref.counts() == got.counts() and sum(got.counts()) == T
    assert torch.equal(ref.idx, got.idx) and torch.equal(ref.gathered.nan_to_num(7.0), got.gathered.nan_to_num(7.0))
    coll = wp0.any(1).cpu().numpy()
    assert 0 < coll.sum() < T or T < 10
    free_e, _ = th.partition_ref(coll, viol)
    np.testing.assert_array_equal(got.idx[:got.counts()[0]].cpu().numpy(), free_e)


@pytest.mark.parametrize("mix", sorted(th.PARTIAL_MIX))
@pytest.mark.parametrize("T,inner", th.PARTIAL_T)
def test_partition_from_hand_built_partial_flags(ops, T, inner, mix):
    """k_traj_partition's phase 0 on its own, no generated kernel involved: rows of 2 .. 11 per-wavefront bytes (both sides of the
    8-entry row form), trajectory counts on both sides of the 32768 flags kept in LDS, and the entries past a trajectory's last
    wavefront poisoned -- they are never read, so zeros and threes there give the same result."""
    lo, hi_q = dev(np.full(7, -1.0, np.float32)), dev(np.full(7, 1.0, np.float32))
    x = np.random.default_rng(T).uniform(-0.99, 0.99, (T, 4, 7)).astype(np.float32)
    xt = dev(x)
    for hi in th.PARTIAL_HI:
        coll_any, outside, flags, rng = th.partial_case(T, hi, mix)
        for poison in (0, 3):
            rows = th.partial_rows(flags, hi, rng, poison)
            off = ops._via_flags_offset(T)
            buf = np.full(off + rows.size, 0xFF, np.uint8)                # counters and flags are outputs: whatever they held
            buf[off:] = rows.reshape(-1)
            part = ops.traj_validate(None, xt, 7, lo, hi_q, inner=inner, flags=(dev(buf), hi))
            _check_partition(part, x, coll_any, outside, inner)
