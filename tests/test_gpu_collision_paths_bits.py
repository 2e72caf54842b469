"""The answers and the routing of the host paths that the link models and the attached-point models share: the boolean check
(ops.rollout_collision, rollout_points_collision and their _via forms; csrc/trk_capi.hip: coll_unit_for, nothing_to_test, launch_coll,
via_samples) and the host side of the rollouts (ops.rollout_cost_grad, rollout_points_cost_grad, RolloutPlan, PointsRolloutPlan,
RolloutViaPlan).

tests/golden/collision_paths_bits.json holds, for every call of the tables below: the kind of return (tensor, tuple, none), the SHA-256
of the raw bytes of every output tensor, `ops.last_dispatch()` after the call -- and, where the call raises, the exception type and its
message.  It was recorded by record() of this module on an MI355X with the library and the Python of the commit BEFORE these paths were
given one body each ("2-D point mass: one planning-loop body, one host path, one plan base").  Booleans are exact and the kernels are
that commit's, so equality is the bound: a difference is a finding, not noise.  The rollouts' digests hold for the toolchain they were
recorded with (ROCm 7.2, gfx950); a toolchain change re-records the file on UNCHANGED source, with PYTHONPATH = the repository and
tests/ (python tests/test_gpu_collision_paths_bits.py [path]), and says so.

Models: the bundled Panda link model ("link": panda_arm_no_gripper, the cost model of tests/golden/cost_spheres3d.npz) and the Panda
with the grasped box as a point set ("points": the task of test_gpu_points_collision.py), both on EnvSpheres3D.
Way-point shapes: (1,) one sample; (63,) and (65,) either side of a wavefront; (3, 5) a (B, H) batch.  Via shapes (T, H, n): (1, 2, 1)
one sample in all; (3, 5, 4) 16 samples per trajectory; (2, 64, 5) 315 samples per trajectory, several wavefronts each.
Routing states: generated; the model's generated kernels off (the way-point forms answer through the scratch as "table-driven", the
via forms return None); a cost model that no unit serves, plain and under strict mode; a cost model with nothing to test.
last_dispatch() is thread state that a declined call (None) leaves as it was: every group below starts with a call that sets it."""
import copy
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import torch_robotics_amd as tra
from helpers import gold, model, panda_cost_spec
from torch_robotics_amd import ops
from torch_robotics_amd._abi import FIELD_OBJECTS, FIELD_SELF, FIELD_WS

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "collision_paths_bits.json"
DEV = torch.device("cuda:0")
TA = dict(device=DEV, dtype=torch.float32)
ALLF = FIELD_SELF | FIELD_OBJECTS | FIELD_WS
MASKS = (FIELD_SELF, FIELD_OBJECTS | FIELD_WS, ALLF)
MARGINS = (None, 0.07)
SHAPES = ((1,), (63,), (65,), (3, 5))
VIA_SHAPES = ((1, 2, 1), (3, 5, 4), (2, 64, 5))
ROLLOUT_SHAPES = ((3, 5), (1, 65))
WEIGHTS = (1.0, 1.0, 1.0, 0.0)
KINDS = ("link", "points")


def digest(t):
    return None if t is None else hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _strip(spec, drop_column=False, nothing=False):
    """the same cost model with one object column less than any unit bakes (drop_column), or with nothing to test (nothing)"""
    s = copy.copy(spec)
    if drop_column:
        s.obj_link_idx = np.asarray(spec.obj_link_idx)[:-1].copy()
        s.obj_link_margin = np.asarray(spec.obj_link_margin)[:-1].copy()
    if nothing:
        s.self_link_idx, s.self_pairs, s.self_margin = np.zeros((0,), np.int32), np.zeros((0, 2), np.int32), np.zeros((0,), np.float32)
        s.ws_min = s.ws_max = None
        s.objects, s.grid = [], None
    s.validate()
    return s


class Side:
    """One column kind: the handles, the cost models of the routing states and the four public functions, called alike."""

    def __init__(self, kind):
        self.kind = kind
        robot = tra.RobotPanda(grasped_object=tra.GraspedObjectPandaBox(tensor_args=TA) if kind == "points" else None, tensor_args=TA)
        self.q_min, self.q_max = robot.q_min_np.astype(np.float32), robot.q_max_np.astype(np.float32)
        self.limits = (dev(self.q_min), dev(self.q_max))
        if kind == "points":
            self.robot = robot
            self.task = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=TA), robot=robot, obstacle_cutoff_margin=0.03, tensor_args=TA)
            spec = self.task.build_cost_spec()
            self.model, self.cm = self.task._fused_handles(DEV)
            self.head = robot._point_set(DEV)
            assert self.head.specialized
            self.coll, self.via = ops.rollout_points_collision, ops.rollout_points_collision_via
            self.cost_grad, self.Plan = ops.rollout_points_cost_grad, ops.PointsRolloutPlan
        else:
            spec = panda_cost_spec(gold("cost_spheres3d"), gold("panda_robot"))
            self.model = self.head = ops.ModelHandle(model("panda_arm_no_gripper"))
            self.cm = ops.CostHandle(spec, DEV)
            assert self.model.specialized
            self.coll, self.via = ops.rollout_collision, ops.rollout_collision_via
            self.cost_grad, self.Plan = ops.rollout_cost_grad, ops.RolloutPlan
        self.cm_unserved = ops.CostHandle(_strip(spec, drop_column=True), DEV)
        self.cm_nothing = ops.CostHandle(_strip(spec, nothing=True), DEV)

    def q(self, shape, seed, cols=7):
        """joint positions uniform in the limits; further columns (a state with velocities) noise"""
        rng = np.random.default_rng(seed)
        x = rng.normal(0.0, 1.0, tuple(shape) + (cols,)).astype(np.float32)
        x[..., :7] = rng.uniform(self.q_min, self.q_max, tuple(shape) + (7,)).astype(np.float32)
        return dev(x)

    def trajs(self, T, H, seed, cols=7):
        x = self.q((T, H), seed, cols)
        x[::2, H // 2, 2] = float(self.q_max[2]) + 0.25              # some way points outside the limits
        return x


_sides = {}


def side(kind):
    if kind not in _sides:
        _sides[kind] = Side(kind)
    return _sides[kind]


def seen(call, validate=None):
    """what a caller sees of one call"""
    try:
        r = call()
    except Exception as e:                                    # the type and the words are the answer
        return {"kind": "raise", "error": f"{type(e).__name__}: {e}"}
    dispatch = ops.last_dispatch()
    if r is None:
        return {"kind": "none", "dispatch": dispatch}
    if isinstance(r, torch.Tensor):
        return {"kind": "tensor", "dispatch": dispatch, "dtype": str(r.dtype), "shape": list(r.shape), "out": [digest(r)]}
    if not isinstance(r, (tuple, list)):
        return {"kind": type(r).__name__, "dispatch": dispatch}
    outs = [digest(t) for t in (validate(r) if validate else r)]
    return {"kind": "tuple", "dispatch": dispatch, "out": outs}


def boolean_calls(s, cm, state):
    """{call id: answer} of the way-point and via forms on one cost model"""
    out = {}
    for shape in SHAPES:
        q = s.q(shape, 10 + len(shape) + shape[0])
        for f in MASKS:
            for mg in MARGINS:
                out[f"{state}: way points {shape} mask {f} margin {mg}"] = seen(lambda: s.coll(s.head, cm, f, q, margin=mg))
    for T, H, n in VIA_SHAPES:
        x = s.trajs(T, H, 40 + H, cols=7 if H != 5 else 9)

        def with_flags(r):
            part = ops.traj_validate(None, x, 7, *s.limits, flags=r[1])
            assert r[1][1] == (H - 1) * n
            return r[0], part.flags, part.idx
        for f in MASKS:
            for mg in MARGINS:
                cid = f"{state}: via ({T}, {H}, {n}) mask {f} margin {mg}"
                out[cid] = seen(lambda: s.via(s.head, cm, f, x, n, margin=mg))
                out[cid + " limits"] = seen(lambda: s.via(s.head, cm, f, x, n, margin=mg, limits=s.limits), with_flags)
    return out


def boolean_answers(kind):
    s = side(kind)
    out = boolean_calls(s, s.cm, "generated")
    s.model.enable_specialized(False)
    try:
        out.update(boolean_calls(s, s.cm, "kernels off"))
    finally:
        s.model.enable_specialized(True)
    out.update(boolean_calls(s, s.cm_unserved, "unserved"))
    with ops.strict_specialized():
        out.update(boolean_calls(s, s.cm_unserved, "unserved, strict"))
    out.update(boolean_calls(s, s.cm_nothing, "nothing to test"))
    return out


def _plan(make, **kw):
    def run():
        plan = make(**kw)
        plan.launch()
        return plan.link_pos, plan.cost, plan.gq, kw.get("gq_out")
    return run


def rollout_answers(kind):
    s = side(kind)
    out = {}
    for B, H in ROLLOUT_SHAPES:
        q = s.q((B, H), 70 + H)
        tag = f"({B}, {H})"
        out[f"cost_grad {tag}"] = seen(lambda: s.cost_grad(s.head, s.cm, WEIGHTS, q))
        out[f"cost_grad {tag} want_pos=False"] = seen(lambda: s.cost_grad(s.head, s.cm, WEIGHTS, q, want_pos=False))
        out[f"cost_grad {tag} flat"] = seen(lambda: s.cost_grad(s.head, s.cm, WEIGHTS, q.reshape(-1, 7)))
        make = lambda **kw: s.Plan(s.head, s.cm, WEIGHTS, q, **kw)
        out[f"plan {tag}"] = seen(_plan(make))
        out[f"plan {tag} want_pos=False"] = seen(_plan(make, want_pos=False))
        out[f"plan {tag} gq_out"] = seen(_plan(make, gq_out=torch.zeros(B * H * 7, **TA)))
        out[f"plan {tag} gq_out of the wrong size"] = seen(_plan(make, gq_out=torch.zeros(B * H * 7 + 1, **TA)))
        out[f"plan {tag} gq_out of the wrong dtype"] = seen(_plan(make, gq_out=torch.zeros(B * H * 7, device=DEV, dtype=torch.float64)))
        out[f"plan {tag} unserved"] = seen(_plan(lambda **kw: s.Plan(s.head, s.cm_unserved, WEIGHTS, q, **kw)))
        out[f"plan {tag} unserved strict=False"] = seen(_plan(lambda **kw: s.Plan(s.head, s.cm_unserved, WEIGHTS, q, strict=False, **kw)))
        out[f"plan {tag} 2-D q"] = seen(lambda: s.Plan(s.head, s.cm, WEIGHTS, q.reshape(-1, 7)))
        if kind == "link":
            h = q.half()
            out[f"cost_grad {tag} fp16 grad_scale 0.25"] = seen(lambda: ops.rollout_cost_grad(s.head, s.cm, WEIGHTS, h, grad_scale=0.25))
            out[f"cost_grad {tag} fp16 mixed"] = seen(lambda: ops.rollout_cost_grad(s.head, s.cm, WEIGHTS, h, grad_dtype=torch.float32, grad_scale=0.5))
            out[f"cost_grad {tag} fp32 with the wrong grad_scale 0.5"] = seen(lambda: ops.rollout_cost_grad(s.head, s.cm, WEIGHTS, q, grad_scale=0.5))
            bufs = (None, torch.zeros(B * H, **TA), torch.zeros(B * H * 7, **TA))
            out[f"cost_grad {tag} out="] = seen(lambda: ops.rollout_cost_grad(s.head, s.cm, WEIGHTS, q, out=bufs) + bufs[1:])
            out[f"plan {tag} fp16 grad_scale 0.25"] = seen(_plan(lambda **kw: ops.RolloutPlan(s.head, s.cm, WEIGHTS, h, grad_scale=0.25, **kw)))
            out[f"plan {tag} fp16 gq_out fp32"] = seen(_plan(lambda **kw: ops.RolloutPlan(s.head, s.cm, WEIGHTS, h, grad_dtype=torch.float32, **kw),
                                                             gq_out=torch.zeros(B * H * 7, **TA)))

            def via_plan(**kw):
                plan = ops.RolloutViaPlan(s.head, s.cm, WEIGHTS, q, 3, **kw)
                plan.launch()
                return plan.cost, plan.gq, kw.get("gq_out")
            out[f"via plan {tag}"] = seen(via_plan)
            out[f"via plan {tag} gq_out"] = seen(lambda: via_plan(gq_out=torch.zeros(B * H * 7, **TA)))
            out[f"via plan {tag} gq_out of the wrong size"] = seen(lambda: via_plan(gq_out=torch.zeros(B * H * 7 - 1, **TA)))
            out[f"via plan {tag} gq_out of the wrong dtype"] = seen(lambda: via_plan(gq_out=torch.zeros(B * H * 7, device=DEV, dtype=torch.float16)))
    return out


def refusal_answers(kind):
    """the Python side's own refusals, with their words"""
    s = side(kind)
    q8, x = s.q((4,), 3, cols=8), s.trajs(3, 5, 5)
    short = (s.limits[0][:6].contiguous(), s.limits[1])
    return {
        "first: a sound call": seen(lambda: s.coll(s.head, s.cm, ALLF, q8[:, :7].contiguous())),
        "way points: wrong last dimension of q": seen(lambda: s.coll(s.head, s.cm, ALLF, q8)),
        "way points: a 0-d q": seen(lambda: s.coll(s.head, s.cm, ALLF, torch.zeros((), **TA))),
        "cost_grad: wrong last dimension of q": seen(lambda: s.cost_grad(s.head, s.cm, WEIGHTS, q8)),
        "plan: wrong last dimension of q": seen(lambda: s.Plan(s.head, s.cm, WEIGHTS, q8.reshape(2, 2, 8))),
        "cost_grad: a cost_sum that is too short": seen(lambda: s.cost_grad(s.head, s.cm, WEIGHTS, s.q((3, 5), 1), cost_sum=torch.zeros(0, **TA))),
        "via: way points with fewer columns than DOF": seen(lambda: s.via(s.head, s.cm, ALLF, x[..., :6].contiguous(), 2)),
        "via: limits of the wrong length": seen(lambda: s.via(s.head, s.cm, ALLF, x, 2, limits=short)),
        "via: limits of the wrong dtype": seen(lambda: s.via(s.head, s.cm, ALLF, x, 2, limits=(s.limits[0].double(), s.limits[1]))),
        "validate: a flags buffer that is too short": seen(lambda: ops.traj_validate(None, x, 7, *s.limits, flags=(torch.zeros(40, device=DEV, dtype=torch.uint8), 8)).flags),
    }


GROUPS = {"boolean": boolean_answers, "rollouts": rollout_answers, "refusals": refusal_answers}
CASES = [(g, k) for g in GROUPS for k in KINDS]


def record(path=GOLDEN):
    """writes the file the test compares against: the same calls, so the table and the recording cannot drift apart"""
    got = {f"{g}/{k}": GROUPS[g](k) for g, k in CASES}
    Path(path).write_text(json.dumps(got, indent=1, sort_keys=True) + "\n")
    return got


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_the_recorded_file_holds_every_routing_state_and_kind_of_answer(golden):
    assert set(golden) == {f"{g}/{k}" for g, k in CASES}
    for k in KINDS:
        rec = golden[f"boolean/{k}"]
        assert len(rec) == 5 * (len(SHAPES) + 2 * len(VIA_SHAPES)) * len(MASKS) * len(MARGINS)

        def of(state, form, mask=""):
            return [v for c, v in rec.items() if c.startswith(f"{state}: {form}") and mask in c]
        assert all(v["dispatch"] == "generated" and v["kind"] == ("tuple" if "limits" in c else "tensor")
                   for c, v in rec.items() if c.startswith("generated: "))
        assert all(v["kind"] == "tensor" and v["dispatch"] == "table-driven" for v in of("kernels off", "way") + of("unserved", "way", "mask 7"))
        assert all(v["kind"] == "none" for v in of("kernels off", "via") + of("unserved", "via", "mask 7"))
        assert all(v["kind"] == "raise" and v["error"].startswith("NotImplementedError: ") and "strict mode" in v["error"]
                   for v in of("unserved, strict", "way", "mask 7"))
        zeros = {hashlib.sha256(bytes(n)).hexdigest() for n in (1, 63, 65, 15)}
        assert all(v["dispatch"] == "none" and v["out"][0] in zeros for v in of("nothing to test", "way"))
        assert all(v["kind"] == "raise" for c, v in golden[f"refusals/{k}"].items() if not c.startswith("first"))
        roll = golden[f"rollouts/{k}"]
        assert all(v["kind"] == "raise" and v["error"].startswith("ValueError: ") for c, v in roll.items()
                   if ("of the wrong" in c or "2-D" in c) and not c.startswith("via plan (1, 65)"))      # (there the horizon is refused first)
        assert all(v["kind"] == "tuple" and v["dispatch"] == "generated" for c, v in roll.items()
                   if c.startswith(("cost_grad", "plan")) and "wrong" not in c and "2-D" not in c and "unserved" not in c)


@pytest.mark.parametrize("group,kind", CASES)
def test_the_shared_host_paths_return_the_recorded_answers(group, kind, golden):
    got, want = GROUPS[group](kind), golden[f"{group}/{kind}"]
    assert set(got) == set(want)
    wrong = {c: (got[c], want[c]) for c in want if got[c] != want[c]}
    for c, (g, w) in wrong.items():
        print(f"{c}:\n  got  {g}\n  want {w}")
    assert not wrong, sorted(wrong)


if __name__ == "__main__":
    record(*sys.argv[1:2])
