"""The frame-algebra kernels (k_frame_compose(_bwd), k_frame_transform_points(_bwd), k_rotation_from, k_frame_quat_euler) beyond the
one wavefront of tests/golden/frame_algebra.npz: ragged and multi-block batches, a broadcast operand on either side, one point, angles
far outside one turn, quaternions far from unit length -- against the fp64 oracle (oracle/oracle.py; reference code frame.py:55-121,
spatial_vector.py:8-47, quaternion.py:102-120).  The bounds are those of test_frame_algebra_vs_reference_golden and
test_rotation_builders_and_frame_constructor, relative to max(1, max |ref|); test_traj_utils_refs_cpu.py shows that the oracle's fp32
build is inside them on these inputs."""
import numpy as np
import pytest
import torch

import traj_utils_helpers as th
from helpers import grad_excess
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
COMPOSE, INVERSE, INV_COMPOSE = 0, 1, 2


def dev(a):
    return torch.as_tensor(a, device=DEV)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    from torch_robotics_amd import ops as o
    assert (o.FRAME_COMPOSE, o.FRAME_INVERSE, o.FRAME_INV_COMPOSE) == (COMPOSE, INVERSE, INV_COMPOSE)
    return o


def _f64(c, keys):
    return [c[k].astype(np.float64) for k in keys]


@pytest.mark.parametrize("op", [COMPOSE, INVERSE, INV_COMPOSE], ids=["compose", "inverse", "inv_compose"])
@pytest.mark.parametrize("n", th.FRAME_N)
def test_frame_compose_values_and_adjoints(ops, oracle_lib, n, op):
    c = th.frame_case(n)
    leaf = {k: dev(c[k]).requires_grad_(True) for k in ("Ra", "ta", "Rb", "tb")}
    args = [leaf[k] for k in (("Ra", "ta") if op == INVERSE else ("Ra", "ta", "Rb", "tb"))]
    Ro, to = ops.frame_compose(op, *args)
    R64, t64 = Oracle.frame_compose(op, *_f64(c, ("Ra", "ta", "Rb", "tb")), "f64")
    assert Ro.shape == (n, 3, 3) and to.shape == (n, 3)
    assert th.rel_to(host(Ro), R64) < th.TOL_ROT and th.rel_to(host(to), t64) < th.TOL_TRANS
    grads = torch.autograd.grad((Ro * dev(c["wR"])).sum() + (to * dev(c["wt"])).sum(), args)
    ref = Oracle.frame_compose_backward(op, *_f64(c, ("Ra", "ta", "Rb", "tb", "wR", "wt")), "f64")
    for got, want in zip(grads, ref):
        assert th.rel_to(host(got), want) < th.TOL_ADJ
    # without autograd: the same values from the plain launch
    with torch.no_grad():
        Rp, tp = ops.frame_compose(op, *[a.detach() for a in args])
    assert torch.equal(Rp, Ro.detach()) and torch.equal(tp, to.detach())


@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("op", [COMPOSE, INV_COMPOSE], ids=["compose", "inv_compose"])
@pytest.mark.parametrize("n", th.FRAME_N)
def test_frame_compose_with_a_broadcast_frame(ops, oracle_lib, n, op, side):
    """a batch of 1 on either side: the broadcast launch (no gradient wanted) and the expanded one (the broadcast frame's gradient is
    the batch sum of the per-sample adjoints, here summed in fp64 from the oracle's)"""
    c = th.frame_case(n)
    own = ("R" + side, "t" + side)
    one = {k: (v[:1] if k in own else v) for k, v in c.items()}
    full = {k: (np.repeat(v[:1], n, 0) if k in own else v) for k, v in c.items()}
    keys = ("Ra", "ta", "Rb", "tb")
    R64, t64 = Oracle.frame_compose(op, *_f64(one, keys), "f64")
    Ro, to = ops.frame_compose(op, *[dev(one[k]) for k in keys])                    # a_bcast / b_bcast inside the kernel
    assert Ro.shape == (n, 3, 3)
    assert th.rel_to(host(Ro), R64) < th.TOL_ROT and th.rel_to(host(to), t64) < th.TOL_TRANS
    leaf = {k: dev(one[k]).requires_grad_(True) for k in keys}
    Rg, tg = ops.frame_compose(op, *[leaf[k] for k in keys])
    assert torch.equal(Rg.detach(), Ro) and torch.equal(tg.detach(), to)
    grads = torch.autograd.grad((Rg * dev(c["wR"])).sum() + (tg * dev(c["wt"])).sum(), [leaf[k] for k in keys])
    ref = Oracle.frame_compose_backward(op, *_f64(full, keys + ("wR", "wt")), "f64")
    for k, got, want in zip(keys, grads, ref):
        if k in own:
            assert got.shape[0] == 1
            assert th.rel_to(host(got)[0], want.sum(0)) < th.TOL_BCAST, k
        else:
            assert th.rel_to(host(got), want) < th.TOL_ADJ, k
    # a gradient wanted for the full-batch frame only: the broadcast one is expanded all the same, the same launch
    others = [k for k in keys if k not in own]
    part = {k: (dev(one[k]).requires_grad_(True) if k in others else dev(one[k])) for k in keys}
    Rh, th_ = ops.frame_compose(op, *[part[k] for k in keys])
    gh = torch.autograd.grad((Rh * dev(c["wR"])).sum() + (th_ * dev(c["wt"])).sum(), [part[k] for k in others])
    assert torch.equal(Rh.detach(), Ro) and all(torch.equal(x, grads[keys.index(k)]) for k, x in zip(others, gh))


@pytest.mark.parametrize("P", th.POINTS_P)
@pytest.mark.parametrize("n", th.POINTS_N)
def test_frame_transform_points_values_and_adjoints(ops, oracle_lib, n, P):
    c = th.points_case(n, P)
    R, t = dev(c["R"]).requires_grad_(True), dev(c["t"]).requires_grad_(True)
    out = ops.frame_transform_points(R, t, dev(c["pts"]))
    o64, gR64, gt64 = Oracle.frame_transform_points(*_f64(c, ("R", "t", "pts", "w")), "f64")
    assert out.shape == (n, P, 3) and th.rel_to(host(out), o64) < th.TOL_TRANS
    gR, gt = torch.autograd.grad((out * dev(c["w"])).sum(), [R, t])
    assert th.rel_to(host(gR), gR64) < th.TOL_TP_ADJ and th.rel_to(host(gt), gt64) < th.TOL_TP_ADJ


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["x_rot", "y_rot", "z_rot"])
@pytest.mark.parametrize("n", th.ROT_N)
def test_axis_rotations_at_large_angles(ops, oracle_lib, n, kind):
    """angles up to +-20 rad (three turns) and exactly 0, +-pi/2, +-pi: cosf / sinf with their argument reduction"""
    a, w = th.angle_case(n)
    at = dev(a).requires_grad_(True)
    R = ops.axis_rotation(kind, at)
    R64 = Oracle.rotation_from(kind, a.astype(np.float64), "f64")
    err = np.abs(host(R) - R64).max()
    (ga,) = torch.autograd.grad((R * dev(w)).sum(), [at])
    g64 = th.axis_rotation_adjoint64(Oracle.rotation_from(kind, a.astype(np.float64) + np.pi / 2, "f64"), kind, w)
    gerr = th.rel_to(host(ga), g64)
    print(f"axis {kind}, n = {n}: values {err:.2e}, angle adjoint {gerr:.2e}")
    assert R.shape == (n, 3, 3) and err < th.TOL_AXIS
    assert gerr < th.TOL_AXIS_ADJ
    np.testing.assert_array_equal(host(R)[0], np.eye(3, dtype=np.float32))        # angle 0 exactly


def test_quaternion_rotation_far_from_unit_norm(ops, oracle_lib):
    """q_to_rotation_matrix divides by |q|^2: norms 1e-3, 1 and 1e3, values and the gradient w.r.t. q (which scales with 1 / |q|)"""
    q, w = th.quat_case()
    R64, g64 = th.quat_grad_ref(q, w)
    qt = dev(q).requires_grad_(True)
    R = ops.quat_to_rotmat(qt)
    (R * dev(w)).sum().backward()
    assert np.abs(host(R) - R64).max() < 1e-6 * np.abs(R64).max() + 1e-6
    with torch.no_grad():
        assert torch.equal(ops.quat_to_rotmat(dev(q)), R.detach())
    g = host(qt.grad)
    per_group = [grad_excess(g[k::3], g64[k::3]) for k in range(3)]
    print(f"quaternion gradient: expression {th.quat_grad_expression(g, g64):.2e}, element-wise excess per norm group {per_group}")
    assert th.quat_grad_expression(g, g64) < 1e-4
    # that expression's floor is set by the largest gradients (the |q| = 1e-3 group); the element-wise gradient criterion of the suite
    # (helpers.grad_excess: 1e-4 relative + 5e-6 of the largest entry) inside each group checks the other two as well
    assert max(per_group) <= 1.0


def test_quat_euler_of_transforms_equals_rotations(ops, oracle_lib):
    """Frame.get_quaternion / get_euler read out of (n,4,4) transforms (stride 16, pitch 4) and out of their contiguous (n,3,3)
    rotation blocks (stride 9, pitch 3): the same bits, and both inside the bounds against the oracle.  n = 257: a ragged second block."""
    R = th.quat_euler_case()
    n = R.shape[0]
    Hm = np.zeros((n, 4, 4), np.float32)
    Hm[:, :3, :3], Hm[:, 3, 3] = R, 1.0
    Hm[:, :3, 3] = np.random.default_rng(n).uniform(-2.0, 2.0, (n, 3))
    q3, e3 = ops.frame_quat_euler(dev(R), want_quat=True, want_euler=True)
    q4, e4 = ops.frame_quat_euler(dev(Hm), want_quat=True, want_euler=True)
    assert q3.shape == (n, 4) and e3.shape == (n, 3)
    assert torch.equal(q3, q4) and torch.equal(e3, e4)
    q64, e64 = Oracle.frame_quat_euler(R.astype(np.float64), "f64")
    assert np.abs(host(q3) - q64).max() < th.TOL_QUAT and np.abs(host(e3) - e64).max() < th.TOL_EULER
