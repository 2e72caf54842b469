"""The bits of the 2-D point mass's three persistent-loop entries (trk_scene2d_traj_adam_steps, trk_scene2d_traj_via_adam_steps,
trk_scene2d_traj_via_cost_grad; csrc/trk_planar.hip: k_planar_traj_adam, k_planar_traj_via) on the synthetic scenes of
tests/golden/pointmass2d_synth_*.npz.

tests/golden/planar_traj_bits.json holds SHA-256 digests of the raw bytes of every output of the calls below.  It was recorded by
record() of this module on an MI355X with the library built from the commit BEFORE the two kernels were given one loop body ("Test the
Adam and Gauss-Newton IK kernels off the Panda's happy path"), where each kernel still carried its own copy of the loop.  The source
fixes every rounding (-ffp-contract=off, explicit fmaf, __fadd_rn), so a change that only moves code or reorders instructions returns
these bits.  The digests hold for the toolchain they were recorded with (ROCm 7.2, gfx950): the expansions of the square root and the
division are the compiler's, so a toolchain change re-records the file on UNCHANGED source, with PYTHONPATH = the repository and
tests/ (python tests/test_gpu_planar_traj_bits.py [path]), and says so.

Shapes, the smallest at which the loop can go wrong: (1, 1) no neighbour at all; (3, 3) room for 85 trajectories in a workgroup, most
lanes idle; (5, 63) the LDS form with 4 trajectories per workgroup, a ragged second workgroup, and lane tid - 1 of a trajectory's first
sample belonging to another trajectory; (5, 64) the WAVE form, the second workgroup with one live wavefront and three that leave early;
(2, 256) the upper limit.  33 iterations from first_step = 1 are two launches, the cost from the first only.
TRK_PLANAR_ADAM_LDS64 is read once per process, so this file does not toggle it."""
import hashlib
import json
import sys
from pathlib import Path

import pytest
import torch

import test_gpu_planar2d_edges as edges
import test_gpu_planar_traj as tp
from torch_robotics_amd import ops

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "planar_traj_bits.json"
SHAPES = [(1, 1), (3, 3), (5, 63), (5, 64), (2, 256)]
PINS = (3, 12)
N_STEPS, N_INTERP, W_VIA = 33, 5, 0.37


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def case_id(scene, clamp):
    return f"{scene[0]}/grid={int(scene[1])},analytic={int(scene[2])},ws={int(scene[3])}/clamp={int(clamp)}"


def answers(scene, clamp):
    """{call id: {output name: digest}} of one (scene, clamp): per shape the plain loop and the via loop under either pin mask, and one
    via cost_grad evaluation"""
    h, _ = edges.variant(*scene)
    out = {}
    for k, (B, H) in enumerate(SHAPES):
        par = tp.params_of(k)
        dt, sigma, w, w_obj = par
        q0, qd0 = tp.inputs(scene[0], B, H)
        for pin in PINS:
            for via in (False, True):
                q, qd = tp.dev(q0), tp.dev(qd0)
                plan = ops.PlanarAdamPlan(h, q, qd, dt, sigma, w, w_obj, clamp, tp.LR, pin_start=bool(pin & 1), pin_goal=bool(pin & 2),
                                          pin_start_vel=bool(pin & 4), pin_goal_vel=bool(pin & 8), w_via=W_VIA if via else 0.0,
                                          num_interpolation=N_INTERP if via else 0)
                assert plan._fn.__name__ == ("trk_scene2d_traj_via_adam_steps" if via else "trk_scene2d_traj_adam_steps")
                cost = plan.step(N_STEPS)
                assert plan.t == N_STEPS
                out[f"{B}x{H} {'via' if via else 'plain'} loop pin={pin}"] = dict(q=digest(q), qd=digest(qd), m=digest(plan.m), v=digest(plan.v),
                                                                                  cost=digest(cost))
        q, qd = tp.dev(q0), tp.dev(qd0)
        cost, gq, gqd = ops.planar_traj_via_cost_grad(h, q, qd, dt, sigma, w, w_obj, W_VIA, N_INTERP, clamp)
        assert torch.equal(q, tp.dev(q0)) and torch.equal(qd, tp.dev(qd0))
        out[f"{B}x{H} via cost_grad"] = dict(cost=digest(cost), gq=digest(gq), gqd=digest(gqd))
    return out


def record(path=GOLDEN):
    """writes the file the test compares against: the same calls, so the table and the recording cannot drift apart"""
    got = {case_id(s, c): answers(s, c) for s, c in tp.CASES}
    Path(path).write_text(json.dumps(got, indent=1, sort_keys=True) + "\n")
    return got


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_the_recorded_file_holds_these_calls(golden):
    assert set(golden) == {case_id(s, c) for s, c in tp.CASES}
    calls = {f"{B}x{H} {what}" for B, H in SHAPES
             for what in [f"{loop} loop pin={pin}" for loop in ("plain", "via") for pin in PINS] + ["via cost_grad"]}
    for cid, rec in golden.items():
        assert set(rec) == calls, cid
        for call, outs in rec.items():
            assert set(outs) == ({"cost", "gq", "gqd"} if call.endswith("cost_grad") else {"q", "qd", "m", "v", "cost"}), (cid, call)


@pytest.mark.parametrize("scene,clamp", tp.CASES)
def test_the_loop_entries_return_the_recorded_bits(scene, clamp, golden):
    got, want = answers(scene, clamp), golden[case_id(scene, clamp)]
    wrong = {(call, name) for call in want for name in want[call] if got[call][name] != want[call][name]}
    assert not wrong, sorted(wrong)


if __name__ == "__main__":
    record(*sys.argv[1:2])
