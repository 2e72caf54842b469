"""The arm's planning loop with the via-point term (trk_rollout_gp_via_adam_steps, generated kernels k_traj_via_adam;
ops.ArmAdamPlan(..., w_via=, num_interpolation=), PlanningTask.rollout_adam_plan) on the smallest shapes at which the layout can go
wrong: (5, 64, 5) a ragged last workgroup, (17, 4, 1) trajectory boundaries inside a wavefront and a last wavefront of 4 rows,
(33, 2, 5) every lane first or last, (3, 1, 5) no segment, (2, 16, 2).

Evaluation: the cost at lr = 0 and the gradient read out of m after one step from zero state (m1 / 0.1f), against the fp64 oracle
on the way points plus the via points interpolated in fp32 (test_gpu_via_cost.via32) with the fold in fp64, and against what the
same GPU gives in pieces: ArmAdamPlan without the term + w_via x RolloutViaPlan.
Bounds: the cost within test_gpu_arm_traj.cost_bound, whose collision half is the way points' plus w_via x the segment's via points'
(rel 1e-5 of each half's batch maximum).  The gradient within DESIGN section 2's element-wise bound helpers.GRAD_RTOL |ref| +
helpers.GRAD_ATOL max|ref|; at most 3 rows per case may miss it, and each must be the fp64 gradient of the SAME objective at a way
point within 3e-6 of the sample's (helpers.kink_rows_ok: its via points move with it), a kink of the minimum over primitives.
The fold (test_the_fold_follows_the_stated_order): every pass of the kernel's loop runs the same instructions, so the gradient of a
pass is one function G of the pass's configuration, and the kernel itself reads it out: at H = 1 there is no segment and gc = G(x)
exactly (include/trk.h), so a batch of one-sample trajectories placed on the way points and on the fp32 via points (whose bits are
the kernel's: each product and the sum rounded once) returns m1 = fl(0.1f G) for each of them -- every input of the fold with ONE
rounding.  Folded in fp64 in the header's order -- wa = fl(w_via alpha[a]), wb = fl(w_via beta[a]), L = g0 + sum wa g_a,
U = sum wb g_a, gc = L + U[t-1] -- the kernel's gc, read out with one more rounding, may deviate by: at most n + 2 roundings on a
term (its weight's product is exact in the reference, so: the fused multiply-adds from its own to the last, n at the most, and the
final sum), one for each input's read-out and one for the result's.  Bound: (n + 4) 2^-24 S (1 + 2^-10), S the sum of the terms'
magnitudes, the last factor for the second-order terms.  No oracle tolerance enters.  alpha and beta swapped in the reference must
miss that bound on most rows.
Update: test_gpu_arm_traj.check_update against the composed GPU gradient at steps 1, 2, 33 and 34; grouping into calls, pin masks,
off-means-off, isolation of a non-finite trajectory, sentinels, unaligned views, graph replay and dispatch to bit equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as hp
import test_gpu_arm_traj as at
import test_gpu_arm_traj_terms as tt
import test_gpu_via_cost as vc
from torch_robotics_amd import _abi, ops
from torch_robotics_amd._lib import lib

pytestmark = pytest.mark.gpu

DEV, TA = at.DEV, at.TA
dev, host = at.dev, at.host
SHAPES = [(5, 64, 5), (17, 4, 1), (33, 2, 5), (3, 1, 5), (2, 16, 2)]
W = (1.0, 1.0, 1.0, 0.0)
W_VIA = {5: 0.2, 1: 1.0, 2: 0.7}                # per n: 1 / n as the example, equal weight, and one that is neither
GP_ON, GP_OFF = (at.DT, at.SIGMA, at.GPW), (at.DT, at.SIGMA, 0.0)
LR = at.LR
MAX_KINK_ROWS = 3
NAME = "generated planning loop with the via-point term"
_refs = {}


def plan_of(h, cm, q, qd, n=0, wv=0.0, lr=LR, pin=3, w=W, gp=GP_ON):
    dt, sigma, gpw = gp
    return ops.ArmAdamPlan(h, cm, w, q, qd, dt, sigma, gpw, lr, pin_start=bool(pin & 1), pin_goal=bool(pin & 2),
                           pin_start_vel=bool(pin & 4), pin_goal_vel=bool(pin & 8), w_via=wv, num_interpolation=n)


def via_reference(key, o, q0, n, w):
    """fp64 oracle on the fp32 via points of q0: (v (B, H-1, n, D), cost (B, H-1, n), gradient (B, H-1, n, D)); once per key"""
    k = (key, q0.shape, n, tuple(w))
    if k not in _refs:
        B, H, D = q0.shape
        v = vc.via32(q0, n)
        _, c, g = o.rollout(v.reshape(-1, D).astype(np.float64), w, "f64", want_pos=False)
        _refs[k] = (v, c.reshape(B, H - 1, n), g.reshape(B, H - 1, n, D))
    return _refs[k]


def total_reference(key, o, oracle_lib, q0, qd0, w, n, wv, gp):
    """test_gpu_arm_traj.reference plus w_via x the via term: the segment t -> t + 1 at sample t, the gradient folded in fp64"""
    B, H, D = q0.shape
    k = ("tot", key, q0.shape, n, tuple(w), wv, gp)
    if k not in _refs:
        ref = at.reference(o, oracle_lib, q0, qd0, w, *gp)
        Cv, Gv = np.zeros((B, H)), np.zeros((B, H, D))
        if H > 1:
            _, cv, gv = via_reference(key, o, q0, n, w)
            Cv[:, :-1] = cv.sum(-1)
            Gv = vc.fold64(gv, n)
        _refs[k] = dict(ref, hinge=ref["hinge"] + wv * Cv, cost=ref["cost"] + wv * Cv, gc=ref["gc"] + wv * Gv, gq=ref["gq"] + wv * Gv)
    return _refs[k]


def total_gradient_at(o, w, n, wv, q0, prior_q):
    """oracle_grad of helpers.kink_rows_ok: the fp64 gradient of the whole objective with respect to ONE way point moved to qp, its
    neighbours where they are: its own term, its two segments' via points (which move with it) and the prior's share"""
    B, H, D = q0.shape
    flat = q0.reshape(B * H, D).astype(np.float64)
    a, b = (x.astype(np.float64) for x in vc.weights(n)) if H > 1 else (np.zeros(0), np.zeros(0))

    def grad(qp):
        idx = at.rows_of(qp, flat)
        out = np.zeros_like(qp)
        for j, (p, r) in enumerate(zip(qp, idx)):
            t = int(r) % H
            cfg, wt = [p], [1.0]
            if t < H - 1:
                cfg += [p * a[k] + flat[r + 1] * b[k] for k in range(n)]
                wt += [wv * a[k] for k in range(n)]
            if t > 0:
                cfg += [flat[r - 1] * a[k] + p * b[k] for k in range(n)]
                wt += [wv * b[k] for k in range(n)]
            g = o.rollout(np.asarray(cfg), w, "f64", want_pos=False)[2]
            out[j] = (np.asarray(wt)[:, None] * g).sum(0) + prior_q[r]
        return out
    return grad


def check_gq(what, got, ref_gq, q0, oracle_grad, rows=None):
    B, H, D = q0.shape
    keep = np.ones(B * H, bool) if rows is None else np.asarray(rows, bool).reshape(B * H)
    g, r = np.asarray(got, np.float64).reshape(B * H, D), np.asarray(ref_gq, np.float64).reshape(B * H, D)
    bound = hp.GRAD_RTOL * np.abs(r) + hp.GRAD_ATOL * max(1e-30, np.abs(r[keep]).max())
    bad = (np.abs(g - r) > bound).any(-1) & keep
    rest = keep & ~bad
    print(f"{what}: {int(bad.sum())} of {int(keep.sum())} judged rows miss the bound; worst error / bound of the rest "
          f"{(np.abs(g - r) / bound)[rest].max() if rest.any() else 0.0:.3f}")
    assert int(bad.sum()) <= MAX_KINK_ROWS, what
    assert hp.kink_rows_ok(g, r, q0.reshape(B * H, D), oracle_grad, bad, max_rows=MAX_KINK_ROWS), what
    return int(bad.sum())


def gradient_of(plan):
    """one step from zero state: m1 = fl(0.1f g) -- the kernel's gradient (q part, qd part) up to one rounding"""
    assert plan.t == 0 and plan.pin == 0
    plan.step(1)
    D = plan.q.shape[-1]
    g = host(plan.m).astype(np.float64) / float(np.float32(0.1))
    return g[..., :D], g[..., D:]


def evaluate(what, key, kin, h, cm, o, oracle_lib, w, shape, gp, grid_of=None):
    B, H, n = shape
    D, wv = kin.n_dofs, W_VIA[n]
    q0, qd0 = at.inputs(kin, B, H)
    tot = total_reference(key, o, oracle_lib, q0, qd0, w, n, wv, gp)
    rows = np.ones((B, H), bool)
    if grid_of is not None:              # judged: the way point and the via points of its two segments off the cell faces in fp64
        rows = tt.grid_rows(o, grid_of, q0, strict=False).reshape(B, H)
        if H > 1:
            vr = tt.grid_rows(o, grid_of, vc.via32(q0, n), strict=False).reshape(B, H - 1, n).all(-1)
            rows[:, :-1] &= vr
            rows[:, 1:] &= vr
        assert rows.mean() >= 0.5, (what, float(rows.mean()))
    # --- cost: lr = 0 writes nothing but cost
    q, qd = dev(q0), dev(qd0)
    ev = plan_of(h, cm, q, qd, n, wv, lr=0.0, w=w, gp=gp)
    ev.m.fill_(7.0); ev.v.fill_(7.0)
    cost = host(ev.step(1)).copy()
    assert ops.last_dispatch() == NAME, what
    assert torch.equal(q, dev(q0)) and torch.equal(qd, dev(qd0)) and bool((ev.m == 7.0).all()) and bool((ev.v == 7.0).all()) and ev.t == 0
    plain = host(plan_of(h, cm, q, qd, lr=0.0, w=w, gp=gp).step(1)).astype(np.float64)
    assert ops.last_dispatch() == "generated"
    via = ops.RolloutViaPlan(h, cm, w, q, n) if H > 1 else None
    pieces, gvia = plain.copy(), np.zeros((B, H, D))
    if via is not None:
        via.launch()
        pieces[:, :-1] += wv * host(via.cost).astype(np.float64).reshape(B, H - 1, n).sum(-1)
        gvia = host(via.gq).astype(np.float64)
    bound = at.cost_bound(dict(hinge=tot["hinge"][rows], prior=tot["prior"][rows]))
    e64, egpu = np.abs(cost - tot["cost"])[rows].max(), np.abs(cost - pieces)[rows].max()
    print(f"{what} {shape}: cost vs fp64 {e64:.3e}, vs the GPU's pieces {egpu:.3e}, bound {bound:.3e}, judged {int(rows.sum())} of {B * H}")
    assert e64 <= bound and egpu <= bound, (what, shape)
    if H == 1:                            # no segment: the plan without the term, within the cost bound
        assert np.abs(cost - plain).max() <= bound
    # --- gradient
    gq, gqd = gradient_of(plan_of(h, cm, dev(q0), dev(qd0), n, wv, pin=0, w=w, gp=gp))
    pq, pqd = gradient_of(plan_of(h, cm, dev(q0), dev(qd0), pin=0, w=w, gp=gp))
    og = total_gradient_at(o, w, n, wv, q0, (tot["gq"] - tot["gc"]).reshape(B * H, D))
    kinks = check_gq(f"{what} {shape} gq vs fp64", gq, tot["gq"], q0, og, rows)
    check_gq(f"{what} {shape} gq vs the GPU's pieces", gq, pq + wv * gvia, q0, og, rows)
    if H > 1 and gp[2] != 0.0:
        assert hp.grad_close(gqd, tot["gqd"], 1e-4) and hp.grad_close(gqd, pqd, 1e-4), what
    else:
        assert not gqd.any(), what
    return kinks


# 1 -- evaluation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,clamp,base", [("spheres", True, "identity"), ("spheres", False, "moved"), ("shelf", True, "identity"),
                                              ("shelf", False, "moved"), ("spheres", True, "moved"), ("shelf", False, "identity")])
def test_evaluation_on_sphere_and_box_scenes(scene, clamp, base, oracle_lib):
    """bi / bg x BOX off (spheres) and on (the shelf's boxes), joints clamped and not"""
    kin, spec, h, cm, o, _ = at.setup(scene, clamp, base)
    for shape in SHAPES:
        for gp in (GP_ON, GP_OFF):       # (the walks' prior is far larger than the collision terms: without it they are held to their own size)
            evaluate(f"{scene} clamp={clamp} {base} gpw={gp[2]:g}", (scene, clamp, base), kin, h, cm, o, oracle_lib, W, shape, gp)


@pytest.mark.parametrize("base", tt.BASES)
def test_evaluation_on_a_voxel_grid(base, oracle_lib):
    """BOX on for a voxel grid, bi and bg; part of the arm outside the grid's limits"""
    kin = tt.panda_kin(base)
    spec = tt.grid_spec(hp.ROLLOUT_GRID_DIMS[0])
    h, cm, o = tt.handles(kin, spec)
    for shape in SHAPES:
        evaluate(f"grid {base}", ("grid", base), kin, h, cm, o, oracle_lib, (1.0, 1.0, 1.0, 1.0), shape, GP_OFF, grid_of=spec)


def test_evaluation_on_the_bundled_ur10_unit(oracle_lib):
    """D = 6 moves the transposes, the moment layout and every D + d"""
    kin, spec = tt.unit_case("ur10", "shelf", True, "moved")
    h, cm, o = tt.handles(kin, spec)
    for shape in [(5, 64, 5), (17, 4, 1)]:
        evaluate("ur10 shelf moved", ("ur10",), kin, h, cm, o, oracle_lib, (0.3, 2.5, 0.7, 1.7), shape, GP_OFF)


def test_evaluation_on_a_run_time_compiled_iiwa7_unit(oracle_lib):
    """the unit of test_gpu_arm_traj.test_a_run_time_compiled_iiwa7_unit (compiled once per checkout, loaded once per process):
    its spec_<ident>_vadam unit is built and loaded when a plan first binds the term (jit.load_satellite_units)"""
    from oracle.oracle import Oracle
    from torch_robotics_amd import codegen, jit
    from torch_robotics_amd.costmodel import CostModelSpec
    import torch_robotics_amd as tra
    kin, tmpl = codegen.template_for("iiwa7")
    obj = list(tmpl.obj_links)[1:]
    spec = CostModelSpec(n_links_in=kin.n_links)
    spec.obj_link_idx = np.asarray(obj, np.int32)
    spec.obj_link_margin = np.linspace(0.08, 0.12, len(obj)).astype(np.float32)
    spec.objects = [ob.as_object() for ob in tra.EnvSpheres3D(tensor_args=TA).obj_fixed_list]
    spec.ws_min, spec.ws_max = np.float32([-1, -1, -1]), np.float32([1, 1, 1])
    spec.clamp_fields = 7
    spec.validate()
    ident = jit.specialize_for_cost_spec(kin, spec)
    assert ident is not None and ident.startswith("jit_")
    # compiled and loaded on the first request for the term, not with the main unit
    assert ((ident, "vadam") in jit._pending) != (f"{ident}_vadam" in jit._loaded)
    h, cm, o = ops.ModelHandle(kin), ops.CostHandle(spec, DEV), Oracle(kin, spec)
    q, qd = (dev(x) for x in at.inputs(kin, 5, 64))
    plan_of(h, cm, q, qd)                                        # the term off: nothing is compiled for it
    assert ((ident, "vadam") in jit._pending) != (f"{ident}_vadam" in jit._loaded)
    plan_of(h, cm, q, qd, 5, 0.2)
    assert f"{ident}_vadam" in jit._loaded and (ident, "vadam") not in jit._pending and jit.load_satellite_units(kin, "vadam") == []
    for shape in [(5, 64, 5), (17, 4, 1)]:
        evaluate("iiwa7 (run-time unit)", ("iiwa7 jit",), kin, h, cm, o, oracle_lib, W, shape, GP_OFF)


def pass_gradients(h, cm, w, cfg):
    """G of the kernel's loop body at configurations cfg (N, D): one-sample trajectories (H = 1: gc = G(x) exactly), the term
    switched on so that the same kernel runs, read out of m after one step from zero state -- one rounding"""
    N, D = cfg.shape
    q = dev(np.ascontiguousarray(cfg.reshape(N, 1, D), np.float32))
    g, _ = gradient_of(plan_of(h, cm, q, torch.zeros_like(q), 5, 0.2, pin=0, w=w, gp=GP_OFF))
    assert ops.last_dispatch() == NAME
    return g.reshape(N, D)


@pytest.mark.parametrize("case", ["ee identity", "ee moved", "spheres identity", "shelf moved"])
def test_the_fold_follows_the_stated_order(case, oracle_lib):
    """the EE term alone (smooth; a way point's successor is far away on the short horizons) at both bases, and the collision terms on
    spheres (bi<false>) and on the shelf's boxes at a moved base (bg<true>): the inputs are the kernel's own bits, so kinks do not matter"""
    if case.startswith("ee"):
        kin = tt.panda_kin(case.split()[1])
        (h, cm, o), w = tt.handles(kin, tt.panda_ee_spec("spheres")), (0.0, 0.0, 0.0, 1.0)
    else:
        scene, base = case.split()
        (kin, spec, h, cm, o, _), w = at.setup(scene, True, base), W
    worst = 0.0
    for B, H, n in [(33, 2, 5), (2, 16, 2), (5, 64, 5), (17, 4, 1)]:
        D, wv = kin.n_dofs, W_VIA[n]
        q0, qd0 = at.inputs(kin, B, H)
        got, _ = gradient_of(plan_of(h, cm, dev(q0), dev(qd0), n, wv, pin=0, w=w, gp=GP_OFF))
        g0 = pass_gradients(h, cm, w, q0.reshape(-1, D)).reshape(B, H, D)
        kg = pass_gradients(h, cm, w, vc.via32(q0, n).reshape(-1, D)).reshape(B, H - 1, n, D)
        a32, b32 = vc.weights(n)

        def folded(al, be):
            wa, wb = (np.float32(wv) * al).astype(np.float64), (np.float32(wv) * be).astype(np.float64)      # fl(w_via alpha[a])
            r, S = g0.copy(), np.abs(g0)
            for arr, fn in ((r, lambda x: x), (S, np.abs)):
                arr[:, :-1] += (fn(kg) * wa[None, None, :, None]).sum(2)
                arr[:, 1:] += (fn(kg) * wb[None, None, :, None]).sum(2)
            return r, (n + 4) * 2.0 ** -24 * S * (1.0 + 2.0 ** -10) + 2.0 ** -140

        r, bound = folded(a32, b32)
        err = np.abs(got - r)
        worst = max(worst, float((err / bound).max()))
        print(f"fold {case} {(B, H, n)}: worst error / rounding-count bound {float((err / bound).max()):.3f}, max |gc| {np.abs(r).max():.4g}")
        assert (err <= bound).all(), (case, B, H, n)
        live = (np.abs(kg).reshape(-1, D).max(-1) > 0).mean()          # the via points do contribute (the EE term: at every one)
        assert np.abs(r).max() > 0 and live > (0.9 if case.startswith("ee") else 0.0), (case, B, H, n, live)
        if n > 1:                         # (n = 1: alpha = beta = 1/2, a swap changes nothing)
            r_sw, bound_sw = folded(b32, a32)
            moved = (np.abs(r_sw - r) > 2.0 * (bound + bound_sw)).any(-1)          # rows on which the swap changes the reference at all
            missed = (np.abs(got - r_sw) > bound_sw).any(-1)
            print(f"fold {case} {(B, H, n)}: alpha and beta swapped: {int(missed.sum())} of {B * H} rows miss the bound ({int(moved.sum())} "
                  f"moved), worst error / bound {float((np.abs(got - r_sw) / bound_sw).max()):.1f}")
            assert moved.any() and missed[moved].all() and (np.abs(got - r_sw) / bound_sw).max() > 100.0, (case, B, H, n)
    print(f"fold {case}: worst error / bound over the shapes {worst:.3f}")


# 2 -- update -------------------------------------------------------------------------------------------------------------------------
def pieces_gradient(h, cm, q, qd, n, wv, w=W, gp=GP_ON):
    """the objective's gradient at the current q, qd from the GPU's pieces: RolloutGpPlan + w_via x RolloutViaPlan"""
    g = ops.RolloutGpPlan(h, cm, w, q, qd, *gp, want_pos=False)
    g.launch()
    v = ops.RolloutViaPlan(h, cm, w, q, n)
    v.launch()
    return tt.cat(host(g.gq).astype(np.float64) + wv * host(v.gq).astype(np.float64), host(g.gqd).astype(np.float64))


@pytest.mark.parametrize("t", [0, 1, 32, 33])
def test_update_against_the_formula(t):
    """iterations 1, 2, 33 and 34 -- the last of a launch's schedule and the first of the next among them"""
    kin, spec, h, cm, o, _ = at.setup("spheres", True, "identity")
    for B, H, n in [(5, 64, 5), (17, 4, 1)]:
        q, qd = (dev(x) for x in at.inputs(kin, B, H))
        plan = plan_of(h, cm, q, qd, n, W_VIA[n], pin=0)
        plan.step(t)
        assert plan.t == t
        x, m, v = tt.cat(host(q), host(qd)), host(plan.m).copy(), host(plan.v).copy()
        g = pieces_gradient(h, cm, q, qd, n, W_VIA[n])
        plan.step(1)
        at.check_update(t + 1, x, m, v, g, tt.cat(host(q), host(qd)), host(plan.m), host(plan.v))


@pytest.mark.parametrize("scene,base", [("spheres", "identity"), ("shelf", "moved")])
def test_grouping_of_iterations_is_bit_neutral(scene, base):
    kin, spec, h, cm, o, _ = at.setup(scene, scene == "spheres", base)
    for B, H, n in [(5, 64, 5), (17, 4, 1)]:
        q0, qd0 = at.inputs(kin, B, H)
        qb, qdb = dev(q0), dev(qd0)
        pb = plan_of(h, cm, qb, qdb, n, W_VIA[n])
        singles, c_first = {}, None
        for k in range(1, 71):           # 70 calls of one iteration, the state kept at the counts that are compared
            c = pb.step(1)
            c_first = c.clone() if c_first is None else c_first
            if k in (1, 32, 33, 70):
                singles[k] = [x.clone() for x in (qb, qdb, pb.m, pb.v)]
        for K in (1, 32, 33, 70):
            qa, qda = dev(q0), dev(qd0)
            pa = plan_of(h, cm, qa, qda, n, W_VIA[n])
            ca = pa.step(K)
            assert pa.t == K and torch.equal(ca, c_first), (B, H, K)
            for x, y in zip((qa, qda, pa.m, pa.v), singles[K]):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (B, H, K)
            assert bool(torch.isfinite(qa).all()) and bool(torch.isfinite(pa.v).all())


def test_all_pin_masks():
    kin, spec, h, cm, o, _ = at.setup("spheres", True, "identity")
    B, H, n = 17, 4, 1
    D = kin.n_dofs
    q0, qd0 = at.inputs(kin, B, H)
    for pin in range(16):
        q, qd = dev(q0), dev(qd0)
        plan = plan_of(h, cm, q, qd, n, W_VIA[n], pin=pin)
        plan.step(3)
        pm = at.pin_masks(pin, B, H, D)
        x0, x1 = tt.cat(q0, qd0), tt.cat(host(q), host(qd))
        assert np.array_equal(x1[pm], x0[pm]) and not host(plan.m)[pm].any() and not host(plan.v)[pm].any(), pin
        assert (host(plan.v)[~pm] > 0).mean() > 0.9, pin


# 3 -- off means off, isolation ------------------------------------------------------------------------------------------------------
def test_off_means_off():
    kin, spec, h, cm, o, _ = at.setup("spheres", True, "identity")
    q0, qd0 = at.inputs(kin, 5, 64)
    qa, qda = dev(q0), dev(qd0)
    base = at.plan_of(h, cm, qa, qda)
    ca = base.step(3).clone()
    assert ops.last_dispatch() == "generated"
    for kw in (dict(wv=0.0, n=5), dict(wv=0.2, n=0), dict(wv=0.0, n=0)):
        qb, qdb = dev(q0), dev(qd0)
        p = plan_of(h, cm, qb, qdb, **kw)
        assert p._fn is base._fn and len(p._args) == len(base._args)          # the same entry point by construction
        cb = p.step(3)
        assert ops.last_dispatch() == "generated"
        for x, y in ((ca, cb), (qa, qb), (qda, qdb), (base.m, p.m), (base.v, p.v)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), kw


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_trajectory_stays_in_its_own_rows(bad):
    """16 (H = 4) and 4 (H = 16) trajectories per wavefront: every neighbour of the spoilt one keeps its bits in q, qd, m, v and cost"""
    kin, spec, h, cm, o, _ = at.setup("shelf", True, "identity")
    for (B, H, n), victims in (((17, 4, 1), (1, 16)), ((5, 16, 5), (2,))):
        q0, qd0 = at.inputs(kin, B, H)
        qa, qda = dev(q0), dev(qd0)
        pa = plan_of(h, cm, qa, qda, n, W_VIA[n], pin=0)
        ca = pa.step(3).clone()
        qb, qdb = dev(q0), dev(qd0)
        for t in victims:
            qb[t] = bad
            qdb[t, H // 2] = bad
        pb = plan_of(h, cm, qb, qdb, n, W_VIA[n], pin=0)
        cb = pb.step(3)
        keep = [t for t in range(B) if t not in victims]
        for x, y in ((ca, cb), (qa, qb), (qda, qdb), (pa.m, pb.m), (pa.v, pb.v)):
            assert torch.equal(x[keep].view(torch.int32), y[keep].view(torch.int32)), (B, H, n)
            assert bool(torch.isfinite(x).all()) and not bool(torch.isfinite(y[list(victims)]).all())


# 4 -- buffers and routing -----------------------------------------------------------------------------------------------------------
def raw_steps(h, cm, w, gp, n, wv, lr, pin, first, steps, q, qd, m, v, cost):
    a, b = ops.via_point_weights(n, DEV)
    ws, g = _abi.RolloutWeights(*[float(x) for x in w]), _abi.GpPrior(*[float(x) for x in gp])
    via, ad = _abi.TrajVia(float(wv), n, a.data_ptr(), b.data_ptr()), _abi.TrajAdam(float(lr), pin, first, steps)
    B, H = q.shape[:2]
    rc = lib().trk_rollout_gp_via_adam_steps(h._h, cm._h, C.byref(ws), C.byref(g), C.byref(via), C.byref(ad), q.data_ptr(), qd.data_ptr(),
                                             m.data_ptr(), v.data_ptr(), B, H, cost.data_ptr(), torch.cuda.current_stream(DEV).cuda_stream)
    assert rc == 0, lib().trk_last_error()


@pytest.mark.parametrize("pad", [64, 65])            # 65: every buffer starts 4 bytes off a 16-byte boundary
def test_sentinels_and_unaligned_views(pad):
    kin, spec, h, cm, o, _ = at.setup("spheres", True, "identity")
    D = kin.n_dofs
    for B, H, n in [(5, 64, 5), (33, 2, 5), (3, 1, 5)]:
        q0, qd0 = at.inputs(kin, B, H)
        q, qd = dev(q0), dev(qd0)
        plan = plan_of(h, cm, q, qd, n, W_VIA[n], pin=5)
        c = plan.step(34).clone()
        bufs = [tt.guarded(x, pad) for x in (q0, qd0, np.zeros((B, H, 2 * D), np.float32), np.zeros((B, H, 2 * D), np.float32),
                                             np.zeros((B, H), np.float32))]
        views = [v for _, v in bufs]
        assert all(v.data_ptr() % 16 == (4 * pad) % 16 for v in views)
        raw_steps(h, cm, W, GP_ON, n, W_VIA[n], LR, 5, 1, 34, *views)
        assert ops.last_dispatch() == NAME
        for (buf, view), want in zip(bufs, (q, qd, plan.m, plan.v, c)):
            assert torch.equal(view.view(torch.int32), want.view(torch.int32)), (B, H, n)
            assert bool((buf[:pad] == tt.SENTINEL).all()) and bool((buf[pad + view.numel():] == tt.SENTINEL).all()), (B, H, n)


def test_target_changed_under_a_live_plan(oracle_lib):
    """TrajViaAdamArgs.C is copied from the cost model on every call: CostHandle.set_ee_target between two steps takes effect"""
    from oracle.oracle import Oracle
    kin = tt.panda_kin("identity")
    h, cm, o_old = tt.handles(kin, tt.panda_ee_spec("spheres", clamp=True))
    T2 = tt.far_target()
    o_new = Oracle(kin, tt.panda_ee_spec("spheres", clamp=True, target=T2))
    w, (B, H, n) = (1.0, 1.0, 1.0, 1.0), (2, 16, 2)
    q0, qd0 = at.inputs(kin, B, H)
    q, qd = dev(q0), dev(qd0)
    plan = plan_of(h, cm, q, qd, n, W_VIA[n], w=w)
    c1 = host(plan.step(1)).copy()
    ref0 = total_reference(("t0",), o_old, oracle_lib, q0, qd0, w, n, W_VIA[n], GP_ON)
    assert np.abs(c1 - ref0["cost"]).max() <= at.cost_bound(ref0)
    x1q, x1qd = host(q).copy(), host(qd).copy()
    cm.set_ee_target(T2)
    c2 = host(plan.step(1)).copy()
    old = total_reference(("t1old",), o_old, oracle_lib, x1q, x1qd, w, n, W_VIA[n], GP_ON)
    new = total_reference(("t1new",), o_new, oracle_lib, x1q, x1qd, w, n, W_VIA[n], GP_ON)
    bound = max(at.cost_bound(old), at.cost_bound(new))
    assert (np.abs(new["cost"] - old["cost"]) > 20.0 * bound).mean() > 0.9          # the two targets are far apart on the reference
    assert np.abs(c2 - new["cost"]).max() <= at.cost_bound(new)
    assert (np.abs(c2 - old["cost"]) > 10.0 * bound).mean() > 0.9


def test_through_the_task_and_dispatch():
    kin, spec, h, cm, o, task = at.setup("spheres", True, "identity")
    B, H, n = 5, 64, 5
    q0, qd0 = at.inputs(kin, B, H)
    qa, qda, qb, qdb = dev(q0), dev(qd0), dev(q0), dev(qd0)
    pa = task.rollout_adam_plan(qa, qda, at.DT, at.SIGMA, gp_weight=at.GPW, w_self=W[0], w_obj=W[1], w_ws=W[2], lr=LR, w_via=0.2,
                                num_interpolation=n)
    pb = plan_of(h, cm, qb, qdb, n, 0.2)
    assert pa._fn is lib().trk_rollout_gp_via_adam_steps or pa._fn.__name__ == "trk_rollout_gp_via_adam_steps"
    ca = pa.step(33)
    assert ops.last_dispatch() == NAME and int(lib().trk_last_dispatch()) == 5
    cb = pb.step(33)
    assert torch.equal(ca, cb) and torch.equal(qa, qb) and torch.equal(qda, qdb) and torch.equal(pa.m, pb.m) and torch.equal(pa.v, pb.v)
    assert not torch.equal(qa, dev(q0)) and pa._weights[0].data_ptr() == pa._via.alpha          # the plan keeps alpha / beta alive
    plain = task.rollout_adam_plan(dev(q0), dev(qd0), at.DT, at.SIGMA, lr=LR)
    plain.step(1)
    assert ops.last_dispatch() == "generated"
    # the refusals of the plain plan hold with the keywords
    t = torch.zeros((2, 48, kin.n_dofs), **TA)
    with pytest.raises(NotImplementedError, match="power of two"):
        task.rollout_adam_plan(t, t.clone(), at.DT, at.SIGMA, w_via=0.2, num_interpolation=n)
    h2 = ops.ModelHandle(kin)
    h2.enable_specialized(False)
    with pytest.raises(NotImplementedError, match="switched off"):
        plan_of(h2, cm, qa, qda, n, 0.2).step(1)
    e = torch.empty((0, 64, kin.n_dofs), **TA)
    plan_of(h, cm, e, e.clone(), n, 0.2).step(5)                  # batch = 0


def test_the_launch_loop_and_the_dispatch_bookkeeping():
    """What the two planning-loop entries share on the host and no kernel's text shows: the loop over the launches with its slice of
    the bias-correction schedule, and trk_last_dispatch.  Panda, sphere scene, 2 x 8: 34 iterations from first_step = 31 in ONE call
    (launches of 32 + 2) against the same entry called twice, 32 and 2 iterations with first_step advanced by hand -- bit for bit,
    for either entry; the dispatch value after each entry, and that an early TRK_OK return (an empty batch) leaves it alone."""
    GENERATED, VIA_COST, VIA_ADAM = 1, 4, 5                       # TRK_DISPATCH_* of include/trk.h
    kin, spec, h, cm, o, _ = at.setup("spheres", True, "identity")
    (B, H, n), D, L = (2, 8, 2), kin.n_dofs, lib()
    q0, qd0 = at.inputs(kin, B, H)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    ws, g = _abi.RolloutWeights(*W), _abi.GpPrior(*GP_ON)
    a, b = ops.via_point_weights(n, DEV)
    via = _abi.TrajVia(W_VIA[n], n, a.data_ptr(), b.data_ptr())

    def steps(with_via, batch, calls):
        q, qd = dev(q0), dev(qd0)
        m, v, cost = (torch.zeros(s, **TA) for s in ((B, H, 2 * D), (B, H, 2 * D), (B, H)))
        for k, (first, count) in enumerate(calls):
            ad = _abi.TrajAdam(LR, 3, first, count)
            head = (h._h, cm._h, C.byref(ws), C.byref(g)) + ((C.byref(via),) if with_via else ())
            fn = L.trk_rollout_gp_via_adam_steps if with_via else L.trk_rollout_gp_adam_steps
            # (the cost is that of the state as passed in: the second call of a split run would overwrite it)
            rc = fn(*head, C.byref(ad), q.data_ptr(), qd.data_ptr(), m.data_ptr(), v.data_ptr(), batch, H, cost.data_ptr() if k == 0 else None,
                    stream)
            assert rc == 0, L.trk_last_error()
            if batch > 0:
                assert int(L.trk_last_dispatch()) == (VIA_ADAM if with_via else GENERATED)
        return [host(x).copy() for x in (q, qd, m, v, cost)]

    for with_via in (False, True):
        one, two = steps(with_via, B, [(31, 34)]), steps(with_via, B, [(31, 32), (63, 2)])
        for x, y in zip(one, two):
            assert np.array_equal(x, y), with_via
        assert not np.array_equal(one[0], q0) and np.isfinite(one[4]).all() and (one[4] > 0).any()
        assert not np.array_equal(one[0], steps(with_via, B, [(31, 32), (62, 2)])[0])       # ... and the schedule's slice is looked at
    x = dev(q0)
    cost, gq = torch.zeros((B, (H - 1) * n), **TA), torch.zeros((B, H, D), **TA)

    def via_cost(n_traj):
        return L.trk_rollout_via_cost_grad(h._h, cm._h, C.byref(ws), x.data_ptr(), n_traj, H, n, a.data_ptr(), b.data_ptr(), None,
                                           cost.data_ptr(), gq.data_ptr(), stream)

    assert via_cost(B) == 0 and int(L.trk_last_dispatch()) == VIA_COST
    assert via_cost(0) == 0 and int(L.trk_last_dispatch()) == VIA_COST
    for with_via in (False, True):
        steps(with_via, 0, [(1, 3)])
        assert int(L.trk_last_dispatch()) == VIA_COST


def test_capture_and_replay():
    kin, spec, h, cm, o, _ = at.setup("shelf", True, "identity")
    B, H, n = 5, 64, 5
    q0, qd0 = at.inputs(kin, B, H)
    qa, qda = dev(q0), dev(qd0)
    pa = plan_of(h, cm, qa, qda, n, W_VIA[n])
    ca = pa.step(32).clone()
    torch.cuda.synchronize()
    qb, qdb = dev(q0), dev(qd0)
    pb = plan_of(h, cm, qb, qdb, n, W_VIA[n])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pb.step(32)
    for x, x0 in ((qb, q0), (qdb, qd0)):                          # (capturing launched nothing)
        assert torch.equal(x, dev(x0))
    assert not pb.m.any()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in ((ca, pb.cost), (qa, qb), (qda, qdb), (pa.m, pb.m), (pa.v, pb.v)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# 5 -- the example --------------------------------------------------------------------------------------------------------------------
def test_the_example_fused_with_the_via_term(capsys):
    import importlib.util
    import re
    path = hp.ROOT / "examples" / "plan_trajectories.py"
    sp = importlib.util.spec_from_file_location("plan_trajectories", path)
    mod = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(mod)
    stats = {}
    q, n_free, coll0 = mod.main(batch=64, horizon=64, iters=100, device="cuda:0", verbose=True, fused=True, stats=stats, via_cost=5)
    out = capsys.readouterr().out
    print(out)
    m = re.search(r"collision-free without the via-point cost: (\d+)/64\s+with it \(5 per segment, w_via = 1/5\): (\d+)/64", out)
    assert m, out                                                # both free counts are printed
    plain, with_via = int(m.group(1)), int(m.group(2))
    assert (plain, with_via) == (stats["n_free_plain"], stats["n_free_via"]) and n_free == with_via
    assert bool(torch.isfinite(q).all())
    assert 0 <= plain <= 64 and 0 <= with_via <= 64
    assert stats["cost_after"] < stats["cost_before"]
