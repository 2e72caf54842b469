"""The plan-specialised rollout family (k_rollout_fx) against the generic generated kernel and the fp64 oracle.

Same inputs through both families (`ops.set_plan_specialized(False)` keeps a launch generic): every output `np.array_equal`.
Which family ran is read from `ops.last_plan_specialized()`; both answer 'generated' to `ops.last_dispatch()`.
Against the fp64 oracle: DESIGN section 2's fp32 tolerances (|dH| <= 2e-6, cost rel 1e-5, gradient rel 1e-4 and per element).
The Panda's first collision point (link 2's origin, (0, 0, 0.333) at the identity base) is a constant of the model: the family reads
its signed distance and gradient from a record evaluated once per cost model.  It lies on joint 1's axis and at joint 2's origin, so
its force has no lever arm on any joint -- its share of d cost / d q is zero in exact arithmetic, and what is asserted non-zero
is its cost share and its position gradient (trk_sdf_points).
"""
import itertools

import numpy as np
import pytest
import torch

from helpers import gold, grad_close_kinks, model, panda_cost_spec, rel_err
from torch_robotics_amd._abi import FIELD_OBJECTS, FIELD_SELF, FIELD_WS
from torch_robotics_amd.costmodel import make_object, sphere_prims

pytestmark = pytest.mark.gpu

TOL_H, TOL_C = 2e-6, 1e-5
W_C2, W_C3 = (0.0, 1.0, 0.0, 1.0), (1.0, 1.0, 1.0, 1.0)
COMPILED_PAIRS = 5          # codegen.FX_AOT["panda"]
P0 = np.array([0.0, 0.0, 0.333], np.float32)      # the constant collision point


def _centres(n, seed=7):
    """n sphere centres in the arm's reach, none within 0.5 m of the constant point (so that it stays outside the cutoff)"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        c = rng.uniform([-0.7, -0.7, 0.0], [0.7, 0.7, 1.0]).astype(np.float32)
        if np.linalg.norm(c - P0) > 0.5:
            out.append(c)
    return np.stack(out)


@pytest.fixture(scope="module")
def env():
    from torch_robotics_amd import ops
    g, robot, gs = gold("rollout_panda"), gold("panda_robot"), gold("cost_spheres3d")
    kin = model("panda_arm_no_gripper")
    handle = ops.ModelHandle(kin)
    cache = {}

    def scene(centres, r=0.15, clamp=False):
        """clamp: the hinge form relu(margin - sdf) of all three fields (clamp_sdf=True), in which a cutoff exists"""
        key = (np.asarray(centres, np.float32).tobytes(), float(r), clamp)
        if key not in cache:
            spec = panda_cost_spec(gs, robot, ee_target=g["target"])
            spec.clamp_fields = (FIELD_SELF | FIELD_OBJECTS | FIELD_WS) if clamp else 0
            spec.objects = [make_object(sphere_prims(centres, np.full(len(centres), r, np.float32)))]
            spec.validate()
            cache[key] = (spec, ops.CostHandle(spec, "cuda:0"))
        return cache[key]

    rng = np.random.default_rng(3)
    q = rng.uniform(-2.8, 2.8, (257 * 48, 7)).astype(np.float32)
    return dict(ops=ops, kin=kin, h=handle, scene=scene, q=q)


def _run(env, cm, w, q, h=None, want_pos=True, want_sum=True, specialised=True):
    """(pos, cost, gq, cost_sum, ran the plan-specialised family?) as numpy"""
    ops = env["ops"]
    qd = torch.as_tensor(q, device="cuda:0")
    n = qd.shape[0] * (qd.shape[1] if qd.dim() == 3 else 1)
    sums = torch.full(((n + 63) // 64,), np.nan, device="cuda:0") if want_sum else None
    prev = ops.set_plan_specialized(specialised)
    try:
        pos, cost, gq = ops.rollout_cost_grad(h or env["h"], cm, w, qd, want_pos=want_pos, cost_sum=sums)
        fx = ops.last_plan_specialized()
        assert ops.last_dispatch() == "generated"
    finally:
        ops.set_plan_specialized(prev)
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return host(pos), host(cost), host(gq), host(sums), fx


def _same(a, b):
    for x, y in zip(a[:4], b[:4]):
        assert (x is None) == (y is None)
        if x is not None:
            assert np.array_equal(x, y)


@pytest.mark.parametrize("n,horizon", [(1, 1), (63, 1), (64, 1), (65, 1), (257, 1), (5, 48)])
@pytest.mark.parametrize("w", [W_C2, W_C3])
def test_both_families_agree_on_ragged_batches_and_match_the_oracle(env, n, horizon, w):
    from oracle.oracle import Oracle
    spec, cm = env["scene"](_centres(2 * COMPILED_PAIRS))
    q = env["q"][:n * horizon].reshape(n, horizon, 7) if horizon > 1 else env["q"][:n]
    fx, gen = _run(env, cm, w, q), _run(env, cm, w, q, specialised=False)
    assert fx[4] and not gen[4]
    _same(fx, gen)
    assert not np.isnan(fx[3]).any()
    q2 = q.reshape(-1, 7)
    o = Oracle(env["kin"], spec)
    p64, c64, g64 = o.rollout(q2.astype(np.float64), w, "f64")
    assert np.abs(fx[0].reshape(-1, 11, 3) - p64).max() < TOL_H
    assert rel_err(fx[1].reshape(-1), c64) < TOL_C
    assert grad_close_kinks(fx[2].reshape(-1, 7), g64, q2, lambda qq: o.rollout(qq, w, "f64")[2])


@pytest.mark.parametrize("n_spheres", [1, 2, 9, 10, 16, 17])
def test_only_a_compiled_pair_count_is_served_and_every_scene_agrees(env, n_spheres):
    spec, cm = env["scene"](_centres(n_spheres, seed=11))
    q = env["q"][:257]
    for w in (W_C2, W_C3):
        fx, gen = _run(env, cm, w, q), _run(env, cm, w, q, specialised=False)
        assert fx[4] == ((n_spheres + 1) // 2 == COMPILED_PAIRS) and not gen[4]      # 9 (odd: the pad copy) and 10 spheres are 5 pairs
        _same(fx, gen)


@pytest.mark.parametrize("mask", list(itertools.product((0.0, 1.0), repeat=4)))
def test_every_zero_pattern_of_the_weights(env, mask):
    spec, cm = env["scene"](_centres(2 * COMPILED_PAIRS))
    w = tuple(m * v for m, v in zip(mask, (0.7, 1.3, 0.4, 2.0)))       # (self, obj, ws, ee)
    q = env["q"][:193]
    fx, gen = _run(env, cm, w, q), _run(env, cm, w, q, specialised=False)
    assert fx[4] == (mask in (W_C2, W_C3)) and not gen[4]
    _same(fx, gen)


@pytest.mark.parametrize("want_pos,want_sum", [(False, True), (True, False), (False, False)])
def test_an_absent_output_goes_to_the_generic_kernel(env, want_pos, want_sum):
    spec, cm = env["scene"](_centres(2 * COMPILED_PAIRS))
    q = env["q"][:130]
    fx, gen = _run(env, cm, W_C2, q, want_pos=want_pos, want_sum=want_sum), _run(env, cm, W_C2, q, want_pos=want_pos, want_sum=want_sum, specialised=False)
    assert not fx[4] and not gen[4]
    _same(fx, gen)
    full = _run(env, cm, W_C2, q)
    assert full[4] and np.array_equal(full[1], fx[1]) and np.array_equal(full[2], fx[2])


def test_constant_point_inside_and_outside_the_cutoff(env):
    ops = env["ops"]
    far = _centres(2 * COMPILED_PAIRS, seed=5)
    near = far.copy()
    near[3] = P0 + np.array([0.12, -0.05, 0.08], np.float32)          # 0.153 m from the point: 3 mm outside the sphere, inside the cutoff
    q = env["q"][:257]
    w_obj = (0.0, 1.0, 0.0, 0.0)
    shares = {}
    for name, c in (("near", near), ("far", far)):
        for clamp in (False, True):
            spec, cm = env["scene"](c, clamp=clamp)
            for w in (W_C2, W_C3):
                fx, gen = _run(env, cm, w, q), _run(env, cm, w, q, specialised=False)
                assert fx[4] and not gen[4]
                _same(fx, gen)
        # (hinge form) the point's own cost share: hinge(margin_0 - sdf(P0)), from the scene's distance at the point
        sdf, grad = ops.sdf_points(cm, torch.as_tensor(P0[None], device="cuda:0"), want_grad=True)
        d = float(sdf.min().cpu())
        shares[name] = (max(0.0, float(spec.obj_link_margin[0]) - d), float(grad.abs().max().cpu()))
    assert shares["near"][0] > 1e-3 and shares["near"][1] > 0.5          # a cost share, and a unit gradient at the point
    assert shares["far"][0] == 0.0
    # the share reaches the cost: every sample of the near scene pays at least it (object term alone, other links add >= 0)
    spec, cm = env["scene"](near, clamp=True)
    fx = _run(env, cm, w_obj, q, specialised=False)
    assert fx[1].min() >= shares["near"][0] * (1 - 1e-5)
    c2 = _run(env, cm, W_C2, q)
    from oracle.oracle import Oracle
    o = Oracle(env["kin"], spec)
    p64, c64, g64 = o.rollout(q.astype(np.float64), W_C2, "f64")
    assert rel_err(c2[1], c64) < TOL_C
    assert grad_close_kinks(c2[2], g64, q, lambda qq: o.rollout(qq, W_C2, "f64")[2])


def test_a_moved_base_and_a_changed_scene_under_the_same_model(env):
    """The family runs at the identity base only; a moved base goes to the generic kernel, and moving it back is served again.  A scene
    cannot change under a cost handle (there is no such call): a second handle has its own record."""
    from oracle.oracle import Oracle
    ops = env["ops"]
    spec, cm = env["scene"](_centres(2 * COMPILED_PAIRS))
    q = env["q"][:130]
    h2 = ops.ModelHandle(env["kin"])
    first = _run(env, cm, W_C2, q, h=h2)
    assert first[4]
    a = 0.3
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32)
    t = np.array([0.1, -0.2, 0.05], np.float32)
    h2.set_base_pose(R, t)
    moved, moved_gen = _run(env, cm, W_C2, q, h=h2), _run(env, cm, W_C2, q, h=h2, specialised=False)
    assert not moved[4]
    _same(moved, moved_gen)
    assert not np.array_equal(moved[1], first[1])
    h2.set_base_pose(np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
    back = _run(env, cm, W_C2, q, h=h2)
    assert back[4]
    _same(back, first)
    near = _centres(2 * COMPILED_PAIRS)
    near[0] = P0 + np.array([-0.1, 0.1, -0.06], np.float32)
    spec2, cm2 = env["scene"](near)
    other, other_gen = _run(env, cm2, W_C2, q, h=h2), _run(env, cm2, W_C2, q, h=h2, specialised=False)
    assert other[4]
    _same(other, other_gen)
    assert not np.array_equal(other[1], first[1])
    again = _run(env, cm, W_C2, q, h=h2)
    _same(again, first)
