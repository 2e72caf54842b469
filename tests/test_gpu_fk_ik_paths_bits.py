"""The answers of the entries that go through the shared host path of the FK, Jacobian, IK, field and rotation / frame families
(csrc/trk_capi.hip: launched, run_utility, unit_or_table, unit_tracking, fill_ik_args, trk_launch.h: trk_jacobian_columns;
ops.py: _call, _fk_reverse, _ik_target, _Rotation, _rot_layout).

tests/golden/fk_ik_paths_bits.json holds, for every call of the tables below: the kind of return and the SHA-256 of the raw bytes of
every output tensor -- or, where the call raises, the exception type and its message -- or, for the calls made on the C ABI itself,
the code and the trk_last_error() text.  It was recorded by record() of this module on an MI355X with the library and the Python of
the commit BEFORE these paths were given one body ("Test pack, reduce and row-scale kernels to the bit; keep -0 in fp16") and was
equal in a second process of that commit.  The kernels are that commit's, bit for bit, so equality is the bound: a difference is a
finding, not noise.  The digests hold for the toolchain they were recorded with (ROCm 7.2, gfx950); a toolchain change re-records the
file on UNCHANGED source, with PYTHONPATH = the repository and tests/ (python tests/test_gpu_fk_ik_paths_bits.py [path]), and says so.

Models: the bundled Panda (panda_arm_no_gripper; the cost model of tests/golden/cost_spheres3d.npz; the Panda holding the grasped box
as the point set), batches of 1, 63 and 65 rows: one row, and either side of a wavefront.  The IK entries also run on the bundled
UR10 and on the Panda-with-hand unit that tracks panda_rightfinger (tests/ik_helpers.py), which is found by the registry scan.
Routing states: generated, and the generated kernels off (`enable_specialized(False)` of the model, or of the cost model for the
fields on given positions); trk_ik_gn_steps has no table-driven form and answers with its refusal."""
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import ik_helpers as ik
import torch_robotics_amd as tra
from helpers import gold, model, panda_cost_spec
from oracle.oracle import Oracle
from torch_robotics_amd import jit, ops
from torch_robotics_amd._abi import FIELD_OBJECTS, FIELD_SELF, FIELD_WS
from torch_robotics_amd._lib import lib

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "fk_ik_paths_bits.json"
DEV = torch.device("cuda:0")
TA = dict(device=DEV, dtype=torch.float32)
NS = (1, 63, 65)
ALLF = FIELD_SELF | FIELD_OBJECTS | FIELD_WS
IK_UNITS = (("ur10", None), ("panda_arm_hand", "panda_rightfinger"))


def digest(t):
    return None if t is None else hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def seen(call):
    """what a caller sees of one call: the digests of what it returns, or the exception's type and words"""
    try:
        r = call()
    except Exception as e:
        return {"kind": "raise", "error": f"{type(e).__name__}: {e}"}
    if isinstance(r, torch.Tensor):
        return {"kind": "tensor", "dtype": str(r.dtype), "shape": list(r.shape), "out": [digest(r)]}
    return {"kind": "tuple", "out": [digest(t) for t in r]}


def seen_c(rc):
    """what a caller of the C ABI sees: the code, and the error text where there is one"""
    return {"kind": "code", "rc": rc, "error": None if rc == 0 else lib().trk_last_error().decode("utf-8")}


def rand(seed, *shape):
    return dev(np.random.default_rng(seed).normal(0.0, 1.0, shape).astype(np.float32))


def poses(seed, n):
    """(n, 4, 4) fp32 transforms: random unit quaternions, positions in a box of the arm's reach"""
    rng = np.random.default_rng(seed)
    H = np.tile(np.eye(4), (n, 1, 1))
    H[:, :3, :3] = ik._rot64(rng.normal(size=(n, 4)))
    H[:, :3, 3] = rng.uniform(-0.6, 0.6, (n, 3))
    return H.astype(np.float32)


class Panda:
    """the handles every FK / Jacobian / field case runs on"""

    def __init__(self):
        kin = model("panda_arm_no_gripper")
        self.kin, self.model = kin, ops.ModelHandle(kin)
        assert self.model.specialized
        self.lo, self.hi = ik.limits(kin)
        self.cm = ops.CostHandle(panda_cost_spec(gold("cost_spheres3d"), gold("panda_robot"), ee_target=poses(7, 1)[0]), DEV)
        self.robot = tra.RobotPanda(grasped_object=tra.GraspedObjectPandaBox(tensor_args=TA), tensor_args=TA)
        self.ps = self.robot._point_set(DEV)
        assert self.ps.specialized
        self.L, self.mid, self.last = kin.n_links, kin.n_links // 2, kin.n_links - 1

    def q(self, n, seed, model_=None):
        lo, hi = (self.lo, self.hi) if model_ is None else ik.limits(model_)
        return dev(ik._uniform(np.random.default_rng(seed), lo, hi, n))


_panda = []


def panda():
    if not _panda:
        _panda.append(Panda())
    return _panda[0]


def both_routes(handle, calls):
    """{state: id: answer} of calls(state) with the handle's generated kernels on, then off"""
    out = calls("generated")
    handle.enable_specialized(False)
    try:
        out.update(calls("kernels off"))
    finally:
        handle.enable_specialized(True)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
def fk_answers():
    p = panda()

    def calls(state):
        out = {}
        for n in NS:
            q = p.q(n, 10 + n)
            for name, sel in (("all links", None), ("one link", [p.last]), ("two links", [p.mid, 2])):
                ncol = p.L if sel is None else len(sel)
                gH, gpos = rand(20 + n + ncol, n, ncol, 4, 4), rand(30 + n + ncol, n, ncol, 3)
                tag = f"{state}: n = {n}, {name}"
                out[f"fk_forward {tag}"] = seen(lambda: ops.fk_forward(p.model, q, sel))
                out[f"fk_positions {tag}"] = seen(lambda: ops.fk_positions(p.model, q, sel))
                out[f"fk_backward {tag}"] = seen(lambda: ops.fk_backward(p.model, q, gH, sel))
                out[f"fk_positions_backward {tag}"] = seen(lambda: ops.fk_positions_backward(p.model, q, gpos, sel))
        return out
    return both_routes(p.model, calls)


def points_answers():
    p = panda()
    m, P = p.ps.model, p.ps.n_points

    def calls(state):
        out = {}
        for n in NS:
            q = p.q(n, 40 + n, m.kin)
            gpos = rand(50 + n, n, P, 3)
            tag = f"{state}: n = {n}"
            out[f"fk_points {tag}"] = seen(lambda: ops.fk_points(p.ps, q))
            out[f"fk_points_backward {tag}"] = seen(lambda: ops.fk_points_backward(p.ps, q, gpos))
            # an output / adjoint 4 bytes off a 16-byte boundary: the generated kernels decline it, the table-driven ones serve it
            buf = torch.zeros(n * P * 3 + 4, **TA)
            off = next(k for k in range(1, 5) if (buf.data_ptr() + 4 * k) % 16 == 4)
            view = buf[off:off + n * P * 3].view(n, P, 3)

            def misaligned_out():
                with ops._on(DEV):
                    rc = lib().trk_fk_points(m._h, p.ps._h, q.data_ptr(), n, view.data_ptr(), ops._stream_of(DEV))
                assert rc == 0, lib().trk_last_error()
                return view
            out[f"fk_points {tag}, misaligned output"] = seen(misaligned_out)
            view_g = buf.clone()[off:off + n * P * 3].view(n, P, 3).copy_(gpos)
            assert view_g.data_ptr() % 16 == 4 and view_g.is_contiguous()
            out[f"fk_points_backward {tag}, misaligned adjoint"] = seen(lambda: ops.fk_points_backward(p.ps, q, view_g))
        return out
    return both_routes(m, calls)


def jacobian_answers():
    p = panda()

    def calls(state):
        out = {}
        for n in NS:
            q, qd = p.q(n, 60 + n), rand(70 + n, n, 7)
            for name, link in (("last link", p.last), ("mid-chain link", p.mid)):
                tag = f"{state}: n = {n}, {name}"
                out[f"fk_jacobian {tag}"] = seen(lambda: ops.fk_jacobian(p.model, q, None, link))
                out[f"fk_jacobian {tag}, qd"] = seen(lambda: ops.fk_jacobian(p.model, q, qd, link, want_vel=True))

                def plan():
                    pl = ops.JacobianPlan(p.model, q, link)
                    pl.launch()
                    return pl.pos, pl.quat, pl.lin_jac, pl.ang_jac
                out[f"JacobianPlan {tag}"] = seen(plan)
            out[f"fk_analytic_jacobian {state}: n = {n}"] = seen(lambda: ops.fk_analytic_jacobian(p.model, q))
        return out
    return both_routes(p.model, calls)


def field_answers():
    p = panda()

    def calls(state):
        out = {}
        for n in NS:
            pos = ops.fk_positions(p.model, p.q(n, 80 + n)) + 0.01 * rand(81 + n, n, p.L, 3)
            H = dev(poses(90 + n, n))
            gc = rand(91 + n, n)
            tag = f"{state}: n = {n}"
            for f in (FIELD_SELF, FIELD_OBJECTS | FIELD_WS, ALLF):
                out[f"cost_fields {tag}, mask {f}"] = seen(lambda: ops.cost_fields(p.cm, f, pos))
                out[f"cost_fields {tag}, mask {f}, gcost"] = seen(lambda: ops.cost_fields(p.cm, f, pos, gcost=gc, want_grad=True))
                for mg in (None, 0.07):
                    out[f"collision_fields {tag}, mask {f}, margin {mg}"] = seen(lambda: ops.collision_fields(p.cm, f, pos, mg))
            out[f"ee_cost {tag}"] = seen(lambda: ops.ee_cost(p.cm, H))
            out[f"ee_cost {tag}, gcost"] = seen(lambda: ops.ee_cost(p.cm, H, gcost=gc, want_grad=True))
            out[f"ee_cost {tag}, one target"] = seen(lambda: ops.ee_cost(p.cm, H, target=dev(poses(3, 1)[0]), want_grad=True))
            out[f"ee_cost {tag}, a target per sample"] = seen(lambda: ops.ee_cost(p.cm, H, target=dev(poses(4, n)), gcost=gc, want_grad=True))
        return out
    return both_routes(p.cm, calls)


_ik_units = {}


def ik_unit(u):
    """(handle, KinModel, tracked link, lower, upper) of a unit of tests/ik_helpers.py; the run-time unit is compiled or found in the cache"""
    if u not in _ik_units:
        kin, tmpl, link = ik.unit(*u)
        if u[1] is not None:
            jit.specialize(kin, tmpl.obj_links, (), ee_link=link)
        h = ops.ModelHandle(kin)
        assert h.specialized, u
        lo, hi = ik.limits(kin, ik.ADAM_SHRINK)
        _ik_units[u] = (h, kin, link, dev(lo), dev(hi))
    return _ik_units[u]


def ik_answers(u):
    h, kin, link, lo, hi = ik_unit(u)
    orc = Oracle(kin)

    def start_np(n):
        return ik._uniform(np.random.default_rng(100 + n), *ik.limits(kin), n)

    def start(n):
        q0 = dev(start_np(n))
        return q0, torch.zeros_like(q0), torch.zeros_like(q0), torch.zeros(n, **TA), torch.zeros(n, device=DEV, dtype=torch.bool)

    def near(n, rows, seed):
        """targets (rows, 4, 4) a short way from the start: the link's pose (fp64 oracle) at the start moved by 0.05 rad of noise per
        joint, so that the SE3 distances of a batch lie on both sides of se3_eps = 0.1 and `valid` holds both answers"""
        qt = start_np(n)[:rows].astype(np.float64) + 0.05 * np.random.default_rng(seed).normal(size=(rows, kin.n_dofs))
        return orc.fk(qt, "f64")[:, link].astype(np.float32)

    def adam(n, Ht, first, steps, lr, one=False):
        def run():
            q, m, v, loss, valid = start(n)
            if one:
                ops.ik_step(h, link, Ht, lo, hi, q, m, v, first, lr=lr, loss=loss, valid=valid)
            else:
                ops.ik_steps(h, link, Ht, lo, hi, q, m, v, first, steps, lr=lr, loss=loss, valid=valid)
            return q, m, v, loss, valid
        return run

    def gn(n, Ht, steps):
        def run():
            q, _, _, err, valid = start(n)
            ops.ik_gn_steps(h, link, Ht, lo, hi, q, steps, err=err, valid=valid)
            return q, err, valid
        return run

    def calls(state):
        out = {}
        for n in NS:
            for name, Ht in (("one target", dev(near(n, 1, 120)[0])), ("a target per sample", dev(near(n, n, 121 + n)))):
                tag = f"{state}: n = {n}, {name}"
                out[f"ik_step {tag}"] = seen(adam(n, Ht, 1, 1, 1e-2, one=True))
                for steps in (1, 32, 33):
                    out[f"ik_steps {tag}, {steps} steps from 31"] = seen(adam(n, Ht, 31, steps, 1e-2))
                out[f"ik_steps {tag}, lr = 0"] = seen(adam(n, Ht, 1, 1, 0.0))
                for steps in (1, 3):
                    out[f"ik_gn_steps {tag}, {steps} steps"] = seen(gn(n, Ht, steps))      # kernels off: the refusal
        return out
    return both_routes(h, calls)


def rotation_answers():
    out = {}

    def with_grad(fn, x, *rest):
        """forward digests and, through autograd with a fixed adjoint per output, the gradient of x"""
        x = x.clone().requires_grad_(True)
        r = fn(x, *rest)
        outs = [t for t in (r if isinstance(r, (tuple, list)) else (r,)) if t is not None]
        sum((t * rand(7 + k, *t.shape)).sum() for k, t in enumerate(outs)).backward()
        return (*outs, x.grad)
    for n in NS:
        for kind in (0, 1, 2):
            a = rand(200 + n + kind, n)
            out[f"axis_rotation kind {kind}, n = {n}"] = seen(lambda: ops.axis_rotation(kind, a))
            out[f"axis_rotation kind {kind}, n = {n}, backward"] = seen(lambda: with_grad(lambda x: ops.axis_rotation(kind, x), a))
        qt = rand(210 + n, n, 4)
        out[f"quat_to_rotmat n = {n}"] = seen(lambda: ops.quat_to_rotmat(qt))
        out[f"quat_to_rotmat n = {n}, backward"] = seen(lambda: with_grad(ops.quat_to_rotmat, qt))
        H = dev(poses(220 + n, n))
        for name, R in (("3x3", H[:, :3, :3].contiguous()), ("4x4", H)):
            tag = f"{name}, n = {n}"
            out[f"rotmat_to_quat {tag}"] = seen(lambda: ops.rotmat_to_quat(R))
            for wq, we in ((True, False), (False, True), (True, True)):
                out[f"frame_quat_euler {tag}, quat {wq}, euler {we}"] = seen(lambda: tuple(t for t in ops.frame_quat_euler(R, wq, we) if t is not None))
                out[f"frame_quat_euler {tag}, quat {wq}, euler {we}, backward"] = seen(lambda: with_grad(lambda x: ops.frame_quat_euler(x, wq, we), R))
        Ra, ta = H[:, :3, :3].contiguous(), H[:, :3, 3].contiguous()
        Hb = dev(poses(230 + n, n))
        Rb, tb = Hb[:, :3, :3].contiguous(), Hb[:, :3, 3].contiguous()
        for op in (ops.FRAME_COMPOSE, ops.FRAME_INVERSE, ops.FRAME_INV_COMPOSE):
            out[f"frame_compose op {op}, n = {n}"] = seen(lambda: ops.frame_compose(op, Ra, ta, Rb, tb))
            out[f"frame_compose op {op}, n = {n}, one b"] = seen(lambda: ops.frame_compose(op, Ra, ta, Rb[:1], tb[:1]))
            out[f"frame_compose op {op}, n = {n}, backward"] = seen(lambda: with_grad(lambda x: ops.frame_compose(op, x, ta, Rb, tb), Ra))
            out[f"frame_compose op {op}, n = {n}, backward to b"] = seen(lambda: with_grad(lambda x: ops.frame_compose(op, Ra, ta, Rb, x), tb))
        pts = rand(240, 5, 3)
        out[f"frame_transform_points n = {n}"] = seen(lambda: ops.frame_transform_points(Ra, ta, pts))
        out[f"frame_transform_points n = {n}, backward"] = seen(lambda: with_grad(lambda x: ops.frame_transform_points(x, ta, pts), Ra))
    return out


def ladder_answers():
    """the C entries' own argument ladders behind the link check, on a live model (the Panda); nothing here reaches a kernel"""
    p = panda()
    L, m = lib(), p.model._h
    buf = torch.zeros(4096, **TA)
    B, st = buf.data_ptr(), ops._stream_of(DEV)
    out = {}

    def jac(q=B, n=2, link=0, pos=B, quat=B, lin=B, ang=B):
        return seen_c(L.trk_fk_jacobian(m, q, None, n, link, pos, quat, lin, ang, None, None, st))

    def iks(link=0, H=B, lower=B, upper=B, lr=0.01, first=1, steps=2, n=2, q=B, am=B, av=B):
        return seen_c(L.trk_ik_steps(m, link, H, 0, lower, upper, 300.0, 0.1, lr, first, steps, n, q, am, av, None, None, st))

    def gn(link=0, H=B, lower=B, upper=B, damping=1e-4, lm=0.1, scale=1.0, steps=2, n=2, q=B):
        return seen_c(L.trk_ik_gn_steps(m, link, H, 0, lower, upper, damping, lm, scale, 0.1, steps, n, q, None, None, st))
    for name, fn in (("trk_fk_jacobian", jac), ("trk_ik_steps", iks), ("trk_ik_gn_steps", gn)):
        out[f"{name}: link = n_links"] = fn(link=p.L)
        out[f"{name}: link = -1"] = fn(link=-1)
        out[f"{name}: negative batch"] = fn(n=-1)
        out[f"{name}: empty batch"] = fn(n=0)
        out[f"{name}: null q"] = fn(q=None)
        out[f"{name}: null q, empty batch"] = fn(q=None, n=0)
        out[f"{name}: link = n_links + negative batch"] = fn(link=p.L, n=-1)
    for a in ("pos", "quat", "lin", "ang"):
        out[f"trk_fk_jacobian: null {a}"] = jac(**{a: None})
    out["trk_fk_jacobian: null outputs, empty batch"] = jac(n=0, pos=None, quat=None, lin=None, ang=None)
    for name, fn in (("trk_ik_steps", iks), ("trk_ik_gn_steps", gn)):
        for a in ("H", "lower", "upper"):
            out[f"{name}: null {a}"] = fn(**{a: None})
            out[f"{name}: null {a}, empty batch"] = fn(**{a: None}, n=0)
        out[f"{name}: n_steps = 0"] = fn(steps=0)
    out["trk_ik_steps: first_step = 0"] = iks(first=0)
    out["trk_ik_steps: null adam_m"] = iks(am=None)
    out["trk_ik_steps: null adam_v"] = iks(av=None)
    out["trk_ik_steps: lr = 0, two steps"] = iks(lr=0.0)
    out["trk_ik_steps: lr = 0, two steps, first_step = 0: the first ladder speaks"] = iks(lr=0.0, first=0)
    out["trk_ik_steps: lr = 0, two steps, empty batch"] = iks(lr=0.0, n=0)
    out["trk_ik_steps: lr = 0, null Adam state, empty batch"] = iks(lr=0.0, steps=1, am=None, av=None, n=0)
    for label, kw in (("damping = -1", dict(damping=-1.0)), ("damping = nan", dict(damping=float("nan"))), ("lm_gain = -1", dict(lm=-1.0)),
                      ("damping = lm_gain = 0", dict(damping=0.0, lm=0.0)), ("step_scale = inf", dict(scale=float("inf"))),
                      ("damping = 0", dict(damping=0.0, n=0)), ("lm_gain = 0", dict(lm=0.0, n=0))):
        out[f"trk_ik_gn_steps: {label}"] = gn(**kw)
    return out


def refusal_answers():
    """the Python side's own refusals of the touched wrappers, with their words"""
    p = panda()
    h, kin, link, lo, hi = ik_unit(IK_UNITS[0])
    q = dev(ik._uniform(np.random.default_rng(5), *ik.limits(kin), 4))
    m, v = torch.zeros_like(q), torch.zeros_like(q)
    Ht5 = dev(poses(6, 5))
    cpu = torch.zeros(4, 7)
    return {
        "fk_backward: q on the host": seen(lambda: ops.fk_backward(p.model, cpu, rand(1, 4, p.L, 4, 4))),
        "fk_backward: gH on the host": seen(lambda: ops.fk_backward(p.model, p.q(4, 1), torch.zeros(4, p.L, 4, 4))),
        "fk_positions_backward: q not a tensor": seen(lambda: ops.fk_positions_backward(p.model, [0.0] * 7, rand(1, 1, p.L, 3))),
        "fk_positions_backward: gpos on the host": seen(lambda: ops.fk_positions_backward(p.model, p.q(4, 1), torch.zeros(4, p.L, 3))),
        "fk_points_backward: q on the host": seen(lambda: ops.fk_points_backward(p.ps, cpu, rand(1, 4, p.ps.n_points, 3))),
        "fk_backward: a link out of range": seen(lambda: ops.fk_backward(p.model, p.q(4, 1), rand(1, 4, 1, 4, 4), [p.L])),
        "fk_backward: a link twice": seen(lambda: ops.fk_backward(p.model, p.q(4, 1), rand(1, 4, 2, 4, 4), [1, 1])),
        "fk_jacobian: a link out of range": seen(lambda: ops.fk_jacobian(p.model, p.q(4, 1), None, p.L)),
        "fk_jacobian: q on the host": seen(lambda: ops.fk_jacobian(p.model, cpu, None, 1)),
        "fk_analytic_jacobian: q on the host": seen(lambda: ops.fk_analytic_jacobian(p.model, cpu)),
        "ik_step: targets for another batch": seen(lambda: ops.ik_step(h, link, Ht5, lo, hi, q, m, v, 1)),
        "ik_steps: targets for another batch": seen(lambda: ops.ik_steps(h, link, Ht5, lo, hi, q, m, v, 1, 2)),
        "ik_gn_steps: targets for another batch": seen(lambda: ops.ik_gn_steps(h, link, Ht5, lo, hi, q, 2)),
        "ik_steps: targets on the host": seen(lambda: ops.ik_steps(h, link, torch.eye(4), lo, hi, q, m, v, 1, 2)),
        "ik_gn_steps: targets on the host": seen(lambda: ops.ik_gn_steps(h, link, torch.eye(4), lo, hi, q, 2)),
        "ik_steps: no Adam state": seen(lambda: ops.ik_steps(h, link, Ht5[0], lo, hi, q, None, None, 1, 2)),
        "ik_steps: a link out of range": seen(lambda: ops.ik_steps(h, kin.n_links, Ht5[0], lo, hi, q.clone(), m, v, 1, 2)),
        "ik_steps: lr = 0 with two steps": seen(lambda: ops.ik_steps(h, link, Ht5[0], lo, hi, q.clone(), m, v, 1, 2, lr=0.0)),
        "ik_gn_steps: no damping at all": seen(lambda: ops.ik_gn_steps(h, link, Ht5[0], lo, hi, q.clone(), 2, damping=0.0, lm_gain=0.0)),
        "rotmat_to_quat: a 2x2": seen(lambda: ops.rotmat_to_quat(rand(1, 4, 2, 2))),
        "frame_quat_euler: a 2x2": seen(lambda: ops.frame_quat_euler(rand(1, 4, 2, 2))),
        "frame_compose: sizes 2 and 3": seen(lambda: ops.frame_compose(0, rand(1, 2, 3, 3), rand(2, 2, 3), rand(3, 3, 3, 3), rand(4, 3, 3))),
        "frame_compose: an unknown op": seen(lambda: ops.frame_compose(3, rand(1, 2, 3, 3), rand(2, 2, 3), rand(3, 2, 3, 3), rand(4, 2, 3))),
        "axis_rotation: an unknown kind": seen(lambda: ops.axis_rotation(4, rand(1, 3))),
        "cost_fields: no field": seen(lambda: ops.cost_fields(p.cm, 0, rand(1, 2, p.L, 3))),
        "collision_fields: an unknown field": seen(lambda: ops.collision_fields(p.cm, 8, rand(1, 2, p.L, 3))),
        "ee_cost: targets for another batch": seen(lambda: ops.ee_cost(p.cm, dev(poses(1, 4)), target=Ht5)),
    }


GROUPS = {"fk": fk_answers, "points": points_answers, "jacobian": jacobian_answers, "fields": field_answers,
          "ik/ur10": lambda: ik_answers(IK_UNITS[0]), "ik/panda_rightfinger": lambda: ik_answers(IK_UNITS[1]),
          "rotations and frames": rotation_answers, "ladders": ladder_answers, "refusals": refusal_answers}


def record(path=GOLDEN):
    """writes the file the test compares against: the same calls, so the table and the recording cannot drift apart"""
    got = {g: fn() for g, fn in GROUPS.items()}
    Path(path).write_text(dump(got))
    return got


def dump(got):
    """the file's layout: one line per call, sorted"""
    groups = [f'"{g}": {{\n' + ",\n".join(f"{json.dumps(c)}: {json.dumps(v, sort_keys=True)}" for c, v in sorted(calls.items())) + "\n}"
              for g, calls in sorted(got.items())]
    return "{\n" + ",\n".join(groups) + "\n}\n"


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_the_recorded_file_holds_both_routes_and_every_kind_of_answer(golden):
    assert set(golden) == set(GROUPS)
    for g in ("fk", "points", "jacobian", "fields", "ik/ur10", "ik/panda_rightfinger"):
        rec = golden[g]
        on = {c: v for c, v in rec.items() if "generated: " in c}
        off = {c.replace("kernels off: ", "generated: "): v for c, v in rec.items() if "kernels off: " in c}
        assert set(on) == set(off) and len(on) + len(off) == len(rec)
        served = [c for c in on if not c.startswith("ik_gn_steps")]
        assert all(on[c]["kind"] != "raise" and off[c]["kind"] != "raise" for c in served), g
        # the two kernel families round differently somewhere: the routing switch did switch
        assert any(on[c] != off[c] for c in served), g
        for c in on:
            if c.startswith("ik_gn_steps"):
                assert on[c]["kind"] == "tuple" and off[c]["kind"] == "raise" and "no generated unit of this model tracks this link" in off[c]["error"]
    pts = golden["points"]
    for n in NS:        # a misaligned buffer is served by the table-driven kernel in either state
        for c in (f"fk_points {{}}: n = {n}, misaligned output", f"fk_points_backward {{}}: n = {n}, misaligned adjoint"):
            assert pts[c.format("generated")] == pts[c.format("kernels off")]
    assert all(v["kind"] == "raise" for v in golden["refusals"].values())
    lad = golden["ladders"]
    assert {v["rc"] for v in lad.values()} == {0, -1} and all(v["rc"] == 0 for c, v in lad.items() if c.endswith(": empty batch"))


@pytest.mark.parametrize("group", list(GROUPS))
def test_the_shared_host_path_returns_the_recorded_answers(group, golden):
    got, want = GROUPS[group](), golden[group]
    assert set(got) == set(want)
    wrong = {c: (got[c], want[c]) for c in want if got[c] != want[c]}
    for c, (g, w) in wrong.items():
        print(f"{c}:\n  got  {g}\n  want {w}")
    assert not wrong, sorted(wrong)


if __name__ == "__main__":
    record(*sys.argv[1:2])
