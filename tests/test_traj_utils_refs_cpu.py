"""The references of test_gpu_traj_utils.py / test_gpu_frame_ops.py, checked without a GPU: the numpy restatements reproduce the
recorded goldens bit for bit, the hand-built partial-flags buffer has the size the library asks for, and the oracle's own fp32 build
stays inside every tolerance those tests take over from the suite -- on the very inputs they use.  The last point is the condition that
a correct fp32 implementation can meet the bounds at the new shapes at all."""
import numpy as np
import pytest
import torch

import traj_utils_helpers as th
from helpers import gold, grad_excess, rel_err
from oracle.oracle import Oracle


def test_interp_and_fd_refs_reproduce_the_goldens_bit_for_bit():
    g = gold("traj")
    np.testing.assert_array_equal(th.interp_ref(g["x"], 5), g["interp5"])
    for m in th.FD_METHODS:
        np.testing.assert_array_equal(th.fd_ref(g["x"], 0.25, m), g["fd_" + m])
    # zero padding at the horizons too short for a difference
    one = np.ones((2, 1, 3), np.float32)
    assert all(not th.fd_ref(one, 0.1, m).any() for m in th.FD_METHODS)
    assert not th.fd_ref(np.ones((2, 2, 3), np.float32), 0.1, "central").any()
    assert th.interp_ref(np.zeros((2, 3, 4, 5), np.float32), 3).shape == (2, 3, 9, 5)


def test_partial_rows_layout_and_size():
    from torch_robotics_amd._lib import lib
    rng = np.random.default_rng(3)
    for T, _ in th.PARTIAL_T:
        for hi in th.PARTIAL_HI:
            flags = rng.integers(0, 4, T).astype(np.uint8)
            for poison in (0, 3):
                rows = th.partial_rows(flags, hi, rng, poison)
                assert rows.dtype == np.uint8 and rows.size == int(lib().trk_via_partial_flags_bytes(T, 2, hi))      # H = 2, n = hi
                t = np.arange(T)
                nj = ((t + 1) * hi - 1) // 64 - (t * hi) // 64 + 1
                live = np.arange(rows.shape[1])[None, :] < nj[:, None]
                np.testing.assert_array_equal(np.bitwise_or.reduce(np.where(live, rows, 0), axis=1), flags)
                assert (rows[~live] == poison).all() and (~live).any()
    # the last live entry alone carries a bit somewhere: a reader that stops one entry early is caught
    flags = np.full(5003, 3, np.uint8)
    rows = th.partial_rows(flags, 630, rng, 0)
    t = np.arange(5003)
    nj = ((t + 1) * 630 - 1) // 64 - (t * 630) // 64 + 1
    head = np.bitwise_or.reduce(np.where(np.arange(rows.shape[1])[None, :] < nj[:, None] - 1, rows, 0), axis=1)
    assert (head != flags).any()
    for T, H, n in th.VIA_CASES:
        assert int(lib().trk_via_partial_flags_bytes(T, H, n)) == T * ((H - 1) * n // 64 + 2)


def test_partition_ref_orders_like_the_reference():
    coll = np.array([0, 1, 0, 1, 0], bool)
    out = np.array([0, 0, 1, 1, 0], bool)
    free, other = th.partition_ref(coll, out)
    np.testing.assert_array_equal(free[:, 0], [0, 4])
    np.testing.assert_array_equal(other[:, 0], [1, 3, 2])
    free, other = th.partition_ref(coll | ~out, out)                  # nothing free, one collision-free violator: only the violator
    assert len(free) == 0 and other.tolist() == [[2]]
    free, other = th.partition_ref(coll, out, inner=2)
    assert free.tolist() == [[0, 0], [2, 0]] and other.tolist() == [[0, 1], [1, 1], [1, 0]]


def test_oracle_fp32_path_metric_inside_the_bound(oracle_lib):
    worst = 0.0
    for H in th.METRIC_H:
        for S, c0, D in th.METRIC_COLS:
            for B in th.METRIC_B:
                x = th.metric_input(B, H, S)
                r64 = oracle_lib.traj_diff_norm_sum(x.astype(np.float64), c0, D, "f64")
                r32 = oracle_lib.traj_diff_norm_sum(x, c0, D, "f32")
                if H == 1:
                    assert not r64.any() and not r32.any()
                else:
                    worst = max(worst, rel_err(r32, r64))
    print(f"path metric, oracle fp32 vs fp64: {worst:.2e}")
    assert worst < th.METRIC_TOL


def test_oracle_fp32_gp_prior_inside_the_bounds(oracle_lib):
    for shape, (dt, sigma, w) in [(s, p) for s, p, _ in th.GP_LONG] + list(th.GP_SMALL) + [(s, th.GP_MILD) for s in th.GP_MISALIGNED]:
        q, qd = th.gp_input(shape)
        c64, g64, gd64 = oracle_lib.gp_prior(q.astype(np.float64), qd.astype(np.float64), dt, sigma, w, "f64")
        c32, g32, gd32 = oracle_lib.gp_prior(q, qd, dt, sigma, w, "f32")
        errs = rel_err(c32, c64), rel_err(g32, g64), rel_err(gd32, gd64)
        print(f"gp prior {shape} dt={dt:.4f} sigma={sigma}: oracle fp32 vs fp64 cost {errs[0]:.2e}, gq {errs[1]:.2e}, gqd {errs[2]:.2e}")
        assert errs[0] < th.GP_TOL_COST and errs[1] < th.GP_TOL_GRAD and errs[2] < th.GP_TOL_GRAD, shape


def test_oracle_fp32_frame_algebra_inside_the_bounds(oracle_lib):
    worst = dict(R=0.0, t=0.0, adj=0.0, bcast=0.0)
    for n in th.FRAME_N:
        c = th.frame_case(n)
        c64 = {k: v.astype(np.float64) for k, v in c.items()}
        for op in (0, 1, 2):
            R64, t64 = Oracle.frame_compose(op, c64["Ra"], c64["ta"], c64["Rb"], c64["tb"], "f64")
            R32, t32 = Oracle.frame_compose(op, c["Ra"], c["ta"], c["Rb"], c["tb"], "f32")
            worst["R"], worst["t"] = max(worst["R"], th.rel_to(R32, R64)), max(worst["t"], th.rel_to(t32, t64))
            a64 = Oracle.frame_compose_backward(op, c64["Ra"], c64["ta"], c64["Rb"], c64["tb"], c64["wR"], c64["wt"], "f64")
            a32 = Oracle.frame_compose_backward(op, c["Ra"], c["ta"], c["Rb"], c["tb"], c["wR"], c["wt"], "f32")
            for g32, g64 in zip(a32, a64):
                worst["adj"] = max(worst["adj"], th.rel_to(g32, g64))
            if op == 1:
                continue
            # a broadcast frame: values, and its gradient = the batch sum of the per-sample adjoints (fp32 sums here, fp64 there)
            for side in ("a", "b"):
                one = {k: (v[:1] if k in ("R" + side, "t" + side) else v) for k, v in c.items()}
                full = {k: (np.repeat(v[:1], n, 0) if k in ("R" + side, "t" + side) else v) for k, v in c.items()}
                R64, t64 = Oracle.frame_compose(op, *[one[k].astype(np.float64) for k in ("Ra", "ta", "Rb", "tb")], "f64")
                R32, t32 = Oracle.frame_compose(op, *[one[k] for k in ("Ra", "ta", "Rb", "tb")], "f32")
                assert R64.shape == (n, 3, 3)
                worst["R"], worst["t"] = max(worst["R"], th.rel_to(R32, R64)), max(worst["t"], th.rel_to(t32, t64))
                keys = ("Ra", "ta", "Rb", "tb", "wR", "wt")
                a64 = Oracle.frame_compose_backward(op, *[full[k].astype(np.float64) for k in keys], "f64")
                a32 = Oracle.frame_compose_backward(op, *[full[k] for k in keys], "f32")
                for j in ((0, 1) if side == "a" else (2, 3)):
                    s64, s32 = a64[j].sum(0), a32[j].sum(0, dtype=np.float32)
                    worst["bcast"] = max(worst["bcast"], th.rel_to(s32, s64))
    print("frame algebra, oracle fp32 vs fp64: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["R"] < th.TOL_ROT and worst["t"] < th.TOL_TRANS and worst["adj"] < th.TOL_ADJ and worst["bcast"] < th.TOL_BCAST


def test_oracle_fp32_transform_points_inside_the_bounds(oracle_lib):
    worst = dict(val=0.0, adj=0.0)
    for n in th.POINTS_N:
        for P in th.POINTS_P:
            c = th.points_case(n, P)
            o64, gR64, gt64 = Oracle.frame_transform_points(*[c[k].astype(np.float64) for k in ("R", "t", "pts")], c["w"].astype(np.float64), "f64")
            o32, gR32, gt32 = Oracle.frame_transform_points(c["R"], c["t"], c["pts"], c["w"], "f32")
            worst["val"] = max(worst["val"], th.rel_to(o32, o64))
            worst["adj"] = max(worst["adj"], th.rel_to(gR32, gR64), th.rel_to(gt32, gt64))
    print("transform_point, oracle fp32 vs fp64: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["val"] < th.TOL_TRANS and worst["adj"] < th.TOL_TP_ADJ


def test_fp32_rotation_builders_inside_the_bounds(oracle_lib):
    """x_rot / y_rot / z_rot at angles up to 20 rad: the oracle's fp32 build, and numpy's fp32 cos / sin, against fp64 at the SAME
    float32 angles; the angle adjoint formed from them in fp32."""
    worst = dict(val=0.0, np=0.0, adj=0.0)
    for n in th.ROT_N:
        a, w = th.angle_case(n)
        a64 = a.astype(np.float64)
        worst["np"] = max(worst["np"], np.abs(np.cos(a).astype(np.float64) - np.cos(a64)).max(), np.abs(np.sin(a).astype(np.float64) - np.sin(a64)).max())
        for kind in (0, 1, 2):
            R64 = Oracle.rotation_from(kind, a64, "f64")
            worst["val"] = max(worst["val"], np.abs(Oracle.rotation_from(kind, a, "f32") - R64).max())
            g64 = th.axis_rotation_adjoint64(Oracle.rotation_from(kind, a64 + np.pi / 2, "f64"), kind, w)
            # the same adjoint from fp32 cos / sin and fp32 products: dR/da has -sin on the two diagonal entries and -+cos off it
            i, j = (1 if kind == 0 else 0), (1 if kind == 2 else 2)
            sg = np.float32(-1.0 if kind == 1 else 1.0)
            c32, s32 = np.cos(a), np.sin(a)
            g32 = -s32 * (w[:, i, i] + w[:, j, j]) + c32 * sg * (w[:, j, i] - w[:, i, j])
            assert g32.dtype == np.float32
            worst["adj"] = max(worst["adj"], th.rel_to(g32, g64))
    print("axis rotations, fp32 vs fp64: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["val"] < th.TOL_AXIS and worst["np"] < th.TOL_AXIS and worst["adj"] < th.TOL_AXIS_ADJ


def test_fp32_quaternion_rotation_inside_the_bounds(oracle_lib):
    q, w = th.quat_case()
    R64, g64 = th.quat_grad_ref(q, w)
    np.testing.assert_allclose(Oracle.rotation_from(3, q.astype(np.float64), "f64"), R64, rtol=0, atol=1e-14)
    np.testing.assert_allclose(R64, th.quat_to_rot64(q), rtol=0, atol=1e-14)
    R32 = Oracle.rotation_from(3, q, "f32")
    assert np.abs(R32 - R64).max() < 1e-6 * np.abs(R64).max() + 1e-6
    # The gradient has no fp32 oracle.  torch's own fp32 autograd through the reference's expression is the nearest thing: it meets the
    # element-wise gradient criterion of helpers.grad_excess inside every norm group, and is reported against the expression of
    # test_quaternion_and_euler_gradients_flow_like_the_reference (< 1e-4 there; its floor of 1e-3 max|g| is one fp32 ulp of the largest
    # entry, which fp32 autograd itself misses at some of these 1000 samples: 1.24e-4).
    _, g32 = th.quat_grad_ref(q, w, dtype=torch.float32)
    print(f"q_to_rotation_matrix, fp32 vs fp64: values {np.abs(R32 - R64).max():.2e}, gradient expression {th.quat_grad_expression(g32, g64):.2e}")
    for k in range(3):
        assert grad_excess(g32[k::3], g64[k::3]) <= 1.0, th.QUAT_NORMS[k]


def test_oracle_fp32_quat_euler_inside_the_bounds(oracle_lib):
    R = th.quat_euler_case()
    q64, e64 = Oracle.frame_quat_euler(R.astype(np.float64), "f64")
    q32, e32 = Oracle.frame_quat_euler(R, "f32")
    print(f"get_quaternion / get_euler, oracle fp32 vs fp64: {np.abs(q32 - q64).max():.2e}, {np.abs(e32 - e64).max():.2e}")
    assert np.abs(q32 - q64).max() < th.TOL_QUAT and np.abs(e32 - e64).max() < th.TOL_EULER
