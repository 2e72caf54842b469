"""The fused via-point cost (trk_rollout_via_cost_grad, generated kernels k_via_cost; ops.rollout_via_cost_grad, ops.RolloutViaPlan,
ops.rollout_via_cost, PlanningTask.compute_collision_cost_via) on the Panda in EnvSpheres3D and EnvTableShelf: costs and way-point
gradient against the fp64 oracle on the via points interpolated in fp32 (each product and the sum rounded once) with the gradient
folded in fp64, and against the two-step route on the GPU (ops.interpolate_traj_via_points + ops.rollout_cost_grad + the fold);
seeds; autograd; determinism, sharding, sentinels and unaligned views; the weights; the iiwa7 and UR10 units and a run-time unit;
the dispatch; graph capture.
Bounds: cost rel 1e-5 of the batch maximum, no exclusions; gradient DESIGN section 2's bound per element, 1e-4 |ref| + 5e-6 max|ref|.
At most 3 way-point rows per case may miss it, and each must touch a via point at which the KERNEL's own gradient (read out with
one-hot seeds) misses the bound too and which helpers.kink_rows_ok confirms to sit on a kink of the fp64 objective."""
import ctypes as C

import numpy as np
import pytest
import torch

import torch_robotics_amd as tra
import helpers as hp
import test_gpu_arm_traj as at
from torch_robotics_amd import _abi, jit, ops
from torch_robotics_amd._lib import lib

pytestmark = pytest.mark.gpu

DEV = at.DEV
TA = at.TA
# (T, H, n): 7 trajectories per wavefront, one idle lane, ragged last wavefront | 16 per wavefront | 3 per wavefront, 13 idle lanes, n = 1 |
# one per wavefront | 31 idle lanes | one segment per trajectory, 32 per wavefront | the smallest case
SHAPES = [(37, 9, 5), (21, 4, 3), (13, 17, 1), (3, 64, 5), (5, 33, 2), (70, 2, 16), (1, 2, 1)]
CASES = at.CASES
W = (1.0, 1.0, 1.0, 0.0)
TOL_COST = 1e-5
MAX_KINK_ROWS = 3
_refs = {}

dev, host = at.dev, at.host


def weights(n):
    a, b = ops.via_point_weights(n, DEV)
    return host(a), host(b)


def via32(x, n):
    """the via points (T, H - 1, n, D) in fp32, each product and the sum rounded once (numpy's float32 arithmetic does)"""
    a, b = weights(n)
    x = np.asarray(x, np.float32)
    v = x[:, :-1, None, :] * a[None, None, :, None] + x[:, 1:, None, :] * b[None, None, :, None]
    assert v.dtype == np.float32
    return v


def fold64(g, n, seed=None):
    """way-point gradient (T, H, D) in fp64 of per-via-point gradients g (T, H - 1, n, D)"""
    a, b = (v.astype(np.float64) for v in weights(n))
    g = np.asarray(g, np.float64)
    T, S, _, D = g.shape
    if seed is not None:
        g = g * np.asarray(seed, np.float64).reshape(T, S, n, 1)
    out = np.zeros((T, S + 1, D))
    out[:, :-1] += (g * a[None, None, :, None]).sum(2)
    out[:, 1:] += (g * b[None, None, :, None]).sum(2)
    return out


def reference(key, o, x, n, w=W):
    """fp64 oracle on the fp32 via points: (v, cost (T, W), g (T, H - 1, n, D)); computed once per (case, shape, weights)"""
    k = (key, x.shape, n, tuple(w))
    if k not in _refs:
        v = via32(x, n)
        T, S, _, D = v.shape
        _, c, g = o.rollout(v.reshape(-1, D).astype(np.float64), w, "f64", want_pos=False)
        _refs[k] = (v, c.reshape(T, S * n), g.reshape(T, S, n, D))
    return _refs[k]


def fused(h, cm, w, x, n, seed=None, want_cost=True):
    res = ops.rollout_via_cost_grad(h, cm, w, dev(x) if isinstance(x, np.ndarray) else x, n,
                                    seed=None if seed is None else (dev(seed) if isinstance(seed, np.ndarray) else seed), want_cost=want_cost)
    assert res is not None, lib().trk_last_error()
    assert ops.last_dispatch() == "generated via-point cost"
    return res


def kernel_via_gradients(h, cm, w, x, n):
    """the kernel's own gradient at every via point (T, H - 1, n, D): with a seed that is 1 on via point a of every second segment,
    gq[t, i] = alpha[a] g(v[t, i, a]) on those segments' first way points"""
    T, H, D = x.shape
    a, _ = weights(n)
    out = np.zeros((T, H - 1, n, D))
    for k in range(n):
        for par in (0, 1):
            seed = np.zeros((T, H - 1, n), np.float32)
            seed[:, par::2, k] = 1.0
            gq = host(fused(h, cm, w, x, n, seed=seed.reshape(T, -1), want_cost=False)[1]).astype(np.float64)
            out[:, par::2, k] = gq[:, :-1][:, par::2] / float(a[k])
    return out


def check(what, o, h, cm, w, x, n, cost, gq, ref, seed=None, oracle_grad=None):
    """cost and way-point gradient against `ref` = (v, cost, per-via gradient), the module's bounds; returns the number of rows at a kink"""
    v, rc, rg = ref
    T, H, D = x.shape
    if cost is not None:
        err = np.abs(host(cost).astype(np.float64) - rc).max()
        print(f"{what}: cost abs err {err:.3e}, bound {TOL_COST * np.abs(rc).max():.3e} (max {np.abs(rc).max():.4g})")
        assert err <= TOL_COST * max(1e-30, np.abs(rc).max()), what
    r = fold64(rg, n, seed).reshape(T * H, D)
    g = host(gq).astype(np.float64).reshape(T * H, D)
    bound = hp.GRAD_RTOL * np.abs(r) + hp.GRAD_ATOL * max(1e-30, np.abs(r).max())
    bad = (np.abs(g - r) > bound).any(-1)
    print(f"{what}: {int(bad.sum())} of {T * H} way-point rows miss the bound; excess of the rest "
          f"{(np.abs(g - r) / bound)[~bad].max() if (~bad).any() else 0.0:.3f}")
    assert int(bad.sum()) <= MAX_KINK_ROWS, what
    if bad.any():
        og = oracle_grad or (lambda qp: o.rollout(qp, w, "f64", want_pos=False)[2])
        kg = kernel_via_gradients(h, cm, w, x, n).reshape(-1, D)
        rv = np.asarray(rg, np.float64).reshape(-1, D)
        vbound = hp.GRAD_RTOL * np.abs(rv) + hp.GRAD_ATOL * max(1e-30, np.abs(rv).max())
        vbad = (np.abs(kg - rv) > vbound).any(-1).reshape(T, H - 1, n)
        for row in np.flatnonzero(bad):
            t, i = divmod(int(row), H)
            touched = np.zeros((T, H - 1, n), bool)
            touched[t, max(0, i - 1):min(H - 1, i + 1)] = True
            mask = (touched & vbad).reshape(-1)
            assert mask.any(), (what, t, i, "no via point of this way point is off in the kernel's own gradient")
            assert hp.kink_rows_ok(kg, rv, v.reshape(-1, D), og, mask), (what, t, i)
    return int(bad.sum())


def two_step(h, cm, w, x, n):
    """the route that exists without the kernel: materialised via points, the rollout on them -> (v, cost (T, W), g (T, H - 1, n, D))"""
    T, H, D = x.shape
    v = ops.interpolate_traj_via_points(dev(x), n)
    _, c, g = ops.rollout_cost_grad(h, cm, w, v, want_pos=False)
    assert ops.last_dispatch() == "generated"
    return host(v).reshape(T, H - 1, n, D), host(c).astype(np.float64), host(g).astype(np.float64).reshape(T, H - 1, n, D)


# 1 + 2 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,clamp,base", CASES)
def test_cost_and_gradient_against_the_oracle_and_the_two_step_route(scene, clamp, base, oracle_lib):
    kin, spec, h, cm, o, _ = at.setup(scene, clamp, base)
    kinks = 0
    for T, H, n in SHAPES:
        x = at.inputs(kin, T, H)[0]
        cost, gq = fused(h, cm, W, x, n)
        assert tuple(cost.shape) == (T, (H - 1) * n) and tuple(gq.shape) == (T, H, kin.n_dofs)
        ref = reference((scene, clamp, base), o, x, n)
        what = f"{scene} clamp={clamp} {base} {(T, H, n)}"
        kinks += check(what + " vs fp64", o, h, cm, W, x, n, cost, gq, ref)
        v2, c2, g2 = two_step(h, cm, W, x, n)
        assert np.array_equal(v2.view(np.uint32), ref[0].view(np.uint32)), what       # the reference's via points are the kernel route's bits
        kinks += check(what + " vs two-step", o, h, cm, W, x, n, cost, gq, (v2, c2, g2))
    print(f"{scene} clamp={clamp} {base}: {kinks} rows at a kink over all shapes")


def ee_setup(scene, square):
    env = (tra.EnvSpheres3D if scene == "spheres" else tra.EnvTableShelf)(tensor_args=TA)
    task = tra.PlanningTask(env=env, robot=tra.RobotPanda(tensor_args=TA), obstacle_cutoff_margin=0.05, clamp_sdf=True, tensor_args=TA)
    Ht = np.eye(4, dtype=np.float32)
    Ht[:3, :3] = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], np.float32)
    Ht[:3, 3] = (0.4, 0.1, 0.5)
    task.set_ee_target(Ht, w_pos=1.0, w_rot=0.5, square=square)
    spec = task.build_cost_spec()
    from oracle.oracle import Oracle
    kin = hp.model("panda_arm_no_gripper")
    return kin, ops.ModelHandle(kin), ops.CostHandle(spec, DEV), Oracle(kin, spec)


@pytest.mark.parametrize("square", [True, False])
def test_the_via_points_are_the_two_step_routes(square, oracle_lib):
    """only the EE term (w_obj = w_self = w_ws = 0): smooth, and a way point's successor is far away -- on (21, 4, 3) a segment spans a
    third of the walk -- so alpha and beta swapped, or the via points of a segment in reverse order, move the cost by orders of
    magnitude more than the tolerance (asserted on the reference itself)"""
    kin, h, cm, o = ee_setup("spheres", square)
    T, H, n = 21, 4, 3
    w = (0.0, 0.0, 0.0, 1.0)
    x = at.inputs(kin, T, H)[0]
    cost, gq = fused(h, cm, w, x, n)
    ref = reference(("ee", square), o, x, n, w)
    tol = TOL_COST * np.abs(ref[1]).max()
    D = kin.n_dofs
    swapped = via32(x[:, ::-1], n)[:, ::-1]               # x[i] * beta + x[i + 1] * alpha, segment order restored
    c_sw = o.rollout(swapped.reshape(-1, D).astype(np.float64), w, "f64", want_pos=False)[1].reshape(T, -1)
    moved = np.abs(c_sw - ref[1])
    # a = 1 of n = 3 is the midpoint (alpha = beta): the swap leaves it alone; the two outer via points of every segment move
    outer = np.ones((T, H - 1, n), bool)
    outer[:, :, 1] = False
    print(f"ee_square={square}: tolerance {tol:.3e}; a swap moves the outer via points' cost by {moved.reshape(T, H - 1, n)[outer].min():.3e} .. {moved.max():.3e}")
    assert moved.reshape(T, H - 1, n)[outer].min() > 1e2 * tol and np.median(moved.reshape(T, H - 1, n)[outer]) > 1e3 * tol
    check(f"ee only, square={square}, vs fp64", o, h, cm, w, x, n, cost, gq, ref)
    v2, c2, g2 = two_step(h, cm, w, x, n)
    check(f"ee only, square={square}, vs two-step", o, h, cm, w, x, n, cost, gq, (v2, c2, g2))


# 3 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,clamp,base", [("spheres", True, "identity"), ("shelf", False, "identity"), ("spheres", True, "moved")])
def test_seeds(scene, clamp, base, oracle_lib):
    kin, spec, h, cm, o, _ = at.setup(scene, clamp, base)
    for T, H, n in [(37, 9, 5), (13, 17, 1), (3, 64, 5), (70, 2, 16)]:
        x = at.inputs(kin, T, H)[0]
        rng = np.random.default_rng(7 * T + H)
        seed = rng.standard_normal((T, (H - 1) * n)).astype(np.float32)
        seed[rng.random(seed.shape) < 0.25] = 0.0
        assert (seed == 0).any() and (seed < 0).any() and (seed > 0).any()
        ref = reference((scene, clamp, base), o, x, n)
        cost, gq = fused(h, cm, W, x, n, seed=seed)
        check(f"{scene} {base} {(T, H, n)} seeded", o, h, cm, W, x, n, cost, gq, ref, seed=seed)
        c0, g0 = fused(h, cm, W, x, n)
        c1, g1 = fused(h, cm, W, x, n, seed=np.ones_like(seed))
        assert torch.equal(c0, c1) and torch.equal(c0, cost) and torch.equal(g0.view(torch.int32), g1.view(torch.int32))
        _, gz = fused(h, cm, W, x, n, seed=np.zeros_like(seed), want_cost=False)
        assert not gz.any()
    # one-hot seeds read the kernel's gradient at single via points out (what `check` falls back on for a row at a kink)
    T, H, n = 21, 4, 3
    x = at.inputs(kin, T, H)[0]
    rv = reference((scene, clamp, base), o, x, n)[2].reshape(-1, kin.n_dofs)
    kg = kernel_via_gradients(h, cm, W, x, n).reshape(rv.shape)
    off = (np.abs(kg - rv) > hp.GRAD_RTOL * np.abs(rv) + hp.GRAD_ATOL * np.abs(rv).max()).any(-1)
    print(f"{scene} {base}: {int(off.sum())} of {len(rv)} via points off in the kernel's own per-via gradient")
    assert int(off.sum()) <= MAX_KINK_ROWS and hp.kink_rows_ok(kg, rv, via32(x, n).reshape(rv.shape), lambda qp: o.rollout(qp, W, "f64", want_pos=False)[2], off)


# 4 -----------------------------------------------------------------------------------------------------------------------------------
def task_weights(task):
    return (1.0 if task.df_collision_self is not None else 0.0, 1.0, 1.0, 0.0)


@pytest.mark.parametrize("scene,clamp", [("spheres", True), ("shelf", False)])
def test_autograd_through_the_task(scene, clamp, oracle_lib):
    kin, spec, h, cm, o, task = at.setup(scene, clamp, "identity")
    w = task_weights(task)
    T, H, n = 37, 9, 5
    x = at.inputs(kin, T, H)[0]
    ref = reference((scene, clamp, "identity"), o, x, n, w)
    r = np.random.default_rng(3).standard_normal((T, (H - 1) * n)).astype(np.float32)
    for name, reduce, seed in (("sum", lambda c: c.sum(), None), ("weighted", lambda c: (c * dev(r)).sum(), r),
                               ("mean", lambda c: c.mean(), np.full_like(r, 1.0 / r.size))):
        q = dev(x).requires_grad_(True)
        cost = task.compute_collision_cost_via(q, num_interpolation=n)
        assert ops.last_dispatch() == "generated via-point cost" and tuple(cost.shape) == (T, (H - 1) * n)
        reduce(cost).backward()
        check(f"{scene} autograd {name}", o, h, cm, w, x, n, cost, q.grad, ref, seed=seed)
    # a state with velocity columns: sliced off, zero gradient there
    full = np.concatenate([x, at.inputs(kin, T, H)[1]], -1)
    q = dev(full).requires_grad_(True)
    cost = task.compute_collision_cost_via(q, num_interpolation=n)
    cost.sum().backward()
    assert tuple(q.grad.shape) == full.shape and not q.grad[..., kin.n_dofs:].any()
    check(f"{scene} autograd, velocity columns", o, h, cm, w, x, n, cost, q.grad[..., :kin.n_dofs], ref)
    # without autograd: the same costs; num_interpolation = 0: the way points' own cost
    assert torch.equal(task.compute_collision_cost_via(dev(x), num_interpolation=n), cost.detach())
    assert torch.equal(task.compute_collision_cost_via(dev(x), num_interpolation=0), task.compute_collision_cost(dev(x)))


# 5 -----------------------------------------------------------------------------------------------------------------------------------
def raw(h, cm, w, x, n, seed, cost, gq):
    T, H, _ = x.shape
    a, b = ops.via_point_weights(n, DEV)
    ws = _abi.RolloutWeights(*[float(v) for v in w])
    rc = lib().trk_rollout_via_cost_grad(h._h, cm._h, C.byref(ws), x.data_ptr(), T, H, n, a.data_ptr(), b.data_ptr(),
                                         None if seed is None else seed.data_ptr(), None if cost is None else cost.data_ptr(), gq.data_ptr(),
                                         torch.cuda.current_stream(DEV).cuda_stream)
    assert rc == 0, lib().trk_last_error()


@pytest.mark.parametrize("scene,clamp,base", [("spheres", True, "identity"), ("shelf", False, "identity"), ("spheres", False, "moved")])
def test_determinism_sharding_sentinels_and_alignment(scene, clamp, base):
    kin, spec, h, cm, o, _ = at.setup(scene, clamp, base)
    D, PAD, S = kin.n_dofs, 64, 12345.0
    for (T, H, n), cut in (((37, 9, 5), 10), ((21, 4, 3), 5), ((13, 17, 1), 4), ((3, 64, 5), 1), ((70, 2, 16), 33), ((5, 33, 2), 2)):
        assert cut % (64 // H) != 0 or 64 // H == 1
        x = dev(at.inputs(kin, T, H)[0])
        x0 = x.clone()
        Wn = (H - 1) * n
        cbuf = torch.full((PAD + T * Wn + PAD,), S, **TA)
        gbuf = torch.full((PAD + T * H * D + PAD,), S, **TA)
        cost, gq = cbuf[PAD:PAD + T * Wn].view(T, Wn), gbuf[PAD:PAD + T * H * D].view(T, H, D)
        raw(h, cm, W, x, n, None, cost, gq)
        c1, g1 = cost.clone(), gq.clone()
        for b in (cbuf, gbuf):
            assert (b[:PAD] == S).all() and (b[-PAD:] == S).all()
        assert torch.isfinite(c1).all() and torch.isfinite(g1).all() and torch.equal(x, x0)
        cost.fill_(S)
        gq.fill_(S)
        raw(h, cm, W, x, n, None, cost, gq)                                  # again, into the same (not zeroed) buffers
        assert torch.equal(c1.view(torch.int32), cost.view(torch.int32)) and torch.equal(g1.view(torch.int32), gq.view(torch.int32))
        # the batch split at a trajectory that is no multiple of 64 / H: the second part starts mid-wavefront and at an odd address
        ca, ga = fused(h, cm, W, x[:cut], n)
        cb, gb = fused(h, cm, W, x[cut:], n)
        assert torch.equal(torch.cat([ca, cb]).view(torch.int32), c1.view(torch.int32))
        assert torch.equal(torch.cat([ga, gb]).view(torch.int32), g1.view(torch.int32))
        # a trajectory of NaNs spoils its own rows only: its neighbours in the wavefront keep their bits
        if T >= 3:
            xn = x.clone()
            xn[1] = float("nan")
            cn, gn = fused(h, cm, W, xn, n)
            for t in (0, 2):
                assert torch.equal(cn[t].view(torch.int32), c1[t].view(torch.int32)) and torch.equal(gn[t].view(torch.int32), g1[t].view(torch.int32)), t
        # views that are not 16-byte aligned: x, cost and gq one float into their buffers
        xb = torch.empty(1 + x.numel(), **TA)
        xv = xb[1:].view(T, H, D)
        xv.copy_(x)
        cb2, gb2 = torch.full((2 + T * Wn,), S, **TA), torch.full((2 + T * H * D,), S, **TA)
        assert xv.data_ptr() % 16 == 4 and cb2[1:].data_ptr() % 16 == 4
        raw(h, cm, W, xv, n, None, cb2[1:1 + T * Wn], gb2[1:1 + T * H * D])
        assert torch.equal(cb2[1:-1].view(T, Wn).view(torch.int32), c1.view(torch.int32))
        assert torch.equal(gb2[1:-1].view(T, H, D).view(torch.int32), g1.view(torch.int32))
        assert cb2[0] == S and cb2[-1] == S and gb2[0] == S and gb2[-1] == S


# 6 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("square", [True, False])
def test_weights(square, oracle_lib):
    kin, h, cm, o = ee_setup("shelf", square)
    T, H, n = 37, 9, 5
    x = at.inputs(kin, T, H)[0]
    for w in [(0.0, 1.0, 1.0, 1.0), (1.0, 0.0, 1.0, 0.5), (1.0, 1.0, 0.0, 0.0), (0.7, 2.5, 0.3, 0.25), (0.0, 0.0, 0.0, 1.0), (1.0, 0.0, 0.0, 0.0)]:
        cost, gq = fused(h, cm, w, x, n)
        check(f"shelf + ee (square={square}) weights {w}", o, h, cm, w, x, n, cost, gq, reference(("w", square), o, x, n, w))
    cost, gq = fused(h, cm, (0.0, 0.0, 0.0, 0.0), x, n)
    assert not cost.any() and not gq.any()


# 7 -----------------------------------------------------------------------------------------------------------------------------------
def robot_setup(urdf, scene, ee=True):
    """a bundled robot under its default collision template, as its ahead-of-time unit bakes it"""
    from oracle.oracle import Oracle
    from torch_robotics_amd import codegen
    from torch_robotics_amd.costmodel import CostModelSpec
    kin = hp.model(urdf)
    tmpl = codegen.default_template(kin)
    base = at.setup(scene, True, "identity")[1]
    spec = CostModelSpec(n_links_in=kin.n_links)
    spec.obj_link_idx = np.asarray(tmpl.obj_links, np.int32)
    spec.obj_link_margin = np.full(len(tmpl.obj_links), 0.08, np.float32)
    spec.objects, spec.grid = base.objects, base.grid
    spec.ws_min, spec.ws_max = base.ws_min, base.ws_max
    spec.clamp_fields = base.clamp_fields
    if ee:
        spec.ee_link = tmpl.ee_link
        spec.ee_target = np.eye(4, dtype=np.float32)
        spec.ee_target[:3, 3] = (0.3, 0.2, 0.4)
    spec.validate()
    return kin, spec, ops.ModelHandle(kin), ops.CostHandle(spec, DEV), Oracle(kin, spec)


@pytest.mark.parametrize("urdf", ["iiwa7", "ur10"])
@pytest.mark.parametrize("scene", ["spheres", "shelf"])
def test_other_bundled_units(urdf, scene, oracle_lib):
    kin, spec, h, cm, o = robot_setup(urdf, scene)
    T, H, n = 21, 12, 3
    w = (0.0, 1.0, 1.0, 0.5)
    x = at.inputs(kin, T, H)[0]
    cost, gq = fused(h, cm, w, x, n)
    check(f"{urdf} {scene}", o, h, cm, w, x, n, cost, gq, reference((urdf, scene), o, x, n, w))


def test_a_run_time_unit_with_another_template(oracle_lib):
    """the Panda with fewer collision links than its bundled unit bakes: jit.specialize compiles the unit and its via unit"""
    from oracle.oracle import Oracle
    assert jit.hipcc_available()             # (the hipRTC fall-back carries no via-point cost kernel)
    kin, spec0, _, _, _, _ = at.setup("spheres", True, "identity")
    import copy
    spec = copy.deepcopy(spec0)
    keep = np.arange(len(spec.obj_link_idx)) % 2 == 0
    spec.obj_link_idx, spec.obj_link_margin = spec.obj_link_idx[keep], spec.obj_link_margin[keep]
    spec.validate()
    ident = jit.specialize_for_cost_spec(kin, spec)
    assert ident is not None and ident.startswith("jit_") and f"{ident}_via" in jit._loaded
    h, cm, o = ops.ModelHandle(kin), ops.CostHandle(spec, DEV), Oracle(kin, spec)
    T, H, n = 21, 12, 3
    x = at.inputs(kin, T, H)[0]
    cost, gq = fused(h, cm, W, x, n)
    check("run-time unit", o, h, cm, W, x, n, cost, gq, reference(("jit",), o, x, n, W))


# 8 -----------------------------------------------------------------------------------------------------------------------------------
def test_dispatch_of_the_task_method(oracle_lib):
    kin, spec, h, cm, o, task = at.setup("spheres", True, "identity")
    w = task_weights(task)
    # H = 65: the two-step route
    T, H, n = 3, 65, 2
    x = at.inputs(kin, T, H)[0]
    assert ops.rollout_via_cost_grad(h, cm, w, dev(x), n) is None and b"64" in lib().trk_last_error()
    q = dev(x).requires_grad_(True)
    cost = task.compute_collision_cost_via(q, num_interpolation=n)
    assert ops.last_dispatch() == "generated" and "65" in task.via_cost_declined
    cost.sum().backward()
    check("H = 65, two-step", o, h, cm, w, x, n, cost, q.grad, reference(("d65",), o, x, n, w))
    # H = 64 on the same task: the kernel
    task.compute_collision_cost_via(dev(x[:, :64]), num_interpolation=n)
    assert ops.last_dispatch() == "generated via-point cost" and task.via_cost_declined is None
    # a grasped-box Panda: attached points, the two-step route
    from oracle.oracle import Oracle
    robot = tra.RobotPanda(grasped_object=tra.GraspedObjectPandaBox(tensor_args=TA), tensor_args=TA)
    gtask = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=TA), robot=robot, obstacle_cutoff_margin=0.05, clamp_sdf=True, tensor_args=TA)
    gkin = robot.diff_panda._kin
    pl, po = robot.collision_point_set()
    go = Oracle(gkin, gtask.build_cost_spec())
    gw = task_weights(gtask)
    T, H, n = 9, 9, 3
    xg = at.walks(gkin_limits(gkin), T, H, seed=99)[0]
    q = dev(xg).requires_grad_(True)
    cost = gtask.compute_collision_cost_via(q, num_interpolation=n)
    assert ops.last_dispatch() in ("generated", "table-driven") and tuple(cost.shape) == (T, (H - 1) * n)
    assert "not the links" in gtask.via_cost_declined
    cost.sum().backward()
    v = via32(xg, n)
    D = gkin.n_dofs
    _, c, g = go.rollout_points(pl, po, v.reshape(-1, D).astype(np.float64), gw, "f64")
    ref = (v, c.reshape(T, -1), g.reshape(T, H - 1, n, D))
    err = np.abs(host(cost).astype(np.float64) - ref[1]).max()
    assert err <= TOL_COST * np.abs(ref[1]).max()
    r = fold64(ref[2], n).reshape(T * H, D)
    gg = host(q.grad).astype(np.float64).reshape(T * H, D)
    bad = (np.abs(gg - r) > hp.GRAD_RTOL * np.abs(r) + hp.GRAD_ATOL * np.abs(r).max()).any(-1)
    print(f"grasped box, two-step: cost err {err:.3e}, {int(bad.sum())} rows off")
    assert int(bad.sum()) <= MAX_KINK_ROWS
    if bad.any():                                        # the two-step route's per-via gradients are the rollout's own output
        vt = dev(v.reshape(T, -1, D))
        _, _, gv = ops.rollout_points_cost_grad(gtask._points(DEV), gtask._fused_handles(DEV)[1], gw, vt, want_pos=False)
        kg, rv = host(gv).astype(np.float64).reshape(-1, D), ref[2].reshape(-1, D)
        vbad = (np.abs(kg - rv) > hp.GRAD_RTOL * np.abs(rv) + hp.GRAD_ATOL * np.abs(rv).max()).any(-1).reshape(T, H - 1, n)
        for row in np.flatnonzero(bad):
            t, i = divmod(int(row), H)
            touched = np.zeros((T, H - 1, n), bool)
            touched[t, max(0, i - 1):min(H - 1, i + 1)] = True
            mask = (touched & vbad).reshape(-1)
            assert mask.any()
            assert hp.kink_rows_ok(kg, rv, v.reshape(-1, D), lambda qp: go.rollout_points(pl, po, qp, gw, "f64")[2], mask)


def gkin_limits(kin):
    if not hasattr(kin, "lower_dof"):
        kin.lower_dof, kin.upper_dof = at.dof_limits(kin)
    return kin


def test_strict_mode_and_switched_off_units():
    kin, spec, h, cm, o, _ = at.setup("spheres", True, "identity")
    x = dev(at.inputs(kin, 5, 8)[0])
    # a cost model no unit bakes (one collision link dropped, no run-time unit for it): declined, strict or not
    import copy
    spec2 = copy.deepcopy(spec)
    spec2.obj_link_idx, spec2.obj_link_margin = spec2.obj_link_idx[1:], spec2.obj_link_margin[1:]
    spec2.validate()
    cm2 = ops.CostHandle(spec2, DEV)
    for strict in (False, True):
        with ops.strict_specialized(strict):
            assert ops.rollout_via_cost_grad(h, cm2, W, x, 3) is None
            assert b"bakes this cost model" in lib().trk_last_error()
            with pytest.raises(NotImplementedError, match="bakes this cost model"):
                ops.rollout_via_cost(h, cm2, W, x, 3)
            with pytest.raises(NotImplementedError, match="bakes this cost model"):
                ops.RolloutViaPlan(h, cm2, W, x, 3).launch()
            assert fused(h, cm, W, x, 3)[0].shape == (5, 21)
    # weights that switch the unmatched term off are served
    assert ops.rollout_via_cost_grad(h, cm2, (1.0, 0.0, 0.0, 0.0), x, 3) is not None
    h2 = ops.ModelHandle(kin)
    h2.enable_specialized(False)
    assert ops.rollout_via_cost_grad(h2, cm, W, x, 3) is None and b"switched off" in lib().trk_last_error()
    with pytest.raises(ValueError, match="num_interpolation"):
        ops.rollout_via_cost_grad(h, cm, W, x, 0)
    with pytest.raises(ValueError, match="two way points"):
        ops.rollout_via_cost_grad(h, cm, W, x[:, :1], 3)
    assert ops.rollout_via_cost_grad(h, cm, W, x[:0], 3)[1].shape == (0, 8, 7)


# 9 -----------------------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay():
    kin, spec, h, cm, o, _ = at.setup("shelf", True, "identity")
    T, H, n = 37, 9, 5
    x = dev(at.inputs(kin, T, H)[0])
    seed = dev(np.random.default_rng(5).standard_normal((T, (H - 1) * n)).astype(np.float32))
    plan = ops.RolloutViaPlan(h, cm, W, x, n, seed=seed)
    plan.launch()
    torch.cuda.synchronize()
    c0, g0 = plan.cost.clone(), plan.gq.clone()
    ce, ge = fused(h, cm, W, x, n, seed=seed)
    assert torch.equal(c0, ce) and torch.equal(g0.view(torch.int32), ge.view(torch.int32))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.launch()
    for _ in range(2):
        plan.cost.fill_(-1.0)
        plan.gq.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(plan.cost.view(torch.int32), c0.view(torch.int32)) and torch.equal(plan.gq.view(torch.int32), g0.view(torch.int32))
    # the plan reads x in place: other way points, other results, equal to the eager launch on them
    x.copy_(dev(at.inputs(kin, T, H, seed=77)[0]))
    graph.replay()
    ce, ge = fused(h, cm, W, x, n, seed=seed)
    assert torch.equal(plan.cost, ce) and torch.equal(plan.gq.view(torch.int32), ge.view(torch.int32)) and not torch.equal(plan.cost, c0)
