"""CPU-only checks of the 2-D point mass's trajectory entry points (trk_scene2d_traj_cost_grad, trk_scene2d_traj_adam_steps): header,
EXPORTS and library agree, the ctypes structs have the header's sizes, bad arguments are refused before any device work (the scene
pointer of these calls is a block of zeros that is never read), and only a planar task hands out the optimiser."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

import torch_robotics_amd as tra
from torch_robotics_amd import _abi, _lib

ROOT = Path(__file__).resolve().parent.parent
CPU = dict(device=torch.device("cpu"), dtype=torch.float32)
NEW = ("trk_scene2d_traj_cost_grad", "trk_scene2d_traj_adam_steps")
INVALID, UNSUPPORTED = _abi.TRK_ERR_INVALID_ARG, _abi.TRK_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def trk():
    if not _lib.LIB_PATH.exists():
        _lib.build()
    return _lib.lib()


def test_header_exports_and_library_agree(trk):
    header = (ROOT / "include" / "trk.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(trk_[a-z0-9_]+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(trk, name)
        assert name in (ROOT / "INTEGRATION.md").read_text()


def test_struct_layouts_match_header():
    src = '#include <stdio.h>\n#include "trk.h"\nint main(){printf("%zu %zu %d\\n",sizeof(TrkPlanarObjective),sizeof(TrkPlanarAdam),' \
          'TRK_PLANAR_MAX_HORIZON);}'
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")], check=True)
        out = subprocess.run([str(Path(d) / "s")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(_abi.PlanarObjective), C.sizeof(_abi.PlanarAdam), _abi.TRK_PLANAR_MAX_HORIZON]
    assert _abi.PlanarObjective.gp.offset == 8 and _abi.PlanarAdam.n_steps.offset == 12


def objective(w_obj=1.0, dt=0.08, sigma=1.0, weight=1.0):
    return _abi.PlanarObjective(w_obj, 1, _abi.GpPrior(dt, sigma, weight))


NAN, INF = float("nan"), float("inf")
BAD_OBJECTIVES = [dict(dt=0.0), dict(dt=-0.1), dict(dt=NAN), dict(dt=INF), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=NAN),
                  dict(sigma=INF), dict(w_obj=NAN), dict(w_obj=INF), dict(w_obj=-INF)]


def test_bad_arguments_are_refused_before_any_device_work(trk):
    scene = (C.c_char * 4096)()             # stands for a TrkScene2D*: no call below may reach the point where it is read
    buf = (C.c_float * 4096)()              # host memory standing for the device buffers, never read either
    o, ad = objective(), _abi.PlanarAdam(5e-3, 3, 1, 1)

    def cost_grad(s=scene, ob=o, batch=2, horizon=8):
        return trk.trk_scene2d_traj_cost_grad(s, C.byref(ob) if ob is not None else None, buf, buf, batch, horizon, buf, buf, buf, None)

    def steps(s=scene, ob=o, a=ad, batch=2, horizon=8):
        return trk.trk_scene2d_traj_adam_steps(s, C.byref(ob) if ob is not None else None, C.byref(a) if a is not None else None,
                                               buf, buf, buf, buf, batch, horizon, buf, None)

    for fn in (cost_grad, steps):
        assert fn(s=None) == INVALID and fn(ob=None) == INVALID
        assert fn(batch=-1) == INVALID and fn(horizon=0) == INVALID and fn(horizon=-3) == INVALID
        for kw in BAD_OBJECTIVES:
            assert fn(ob=objective(**kw)) == INVALID, kw
    assert b"trk_scene2d_traj_cost_grad" in trk.trk_last_error() or b"trk_scene2d_traj_adam_steps" in trk.trk_last_error()
    assert steps(a=None) == INVALID
    for bad in (_abi.PlanarAdam(5e-3, 3, 1, -1), _abi.PlanarAdam(5e-3, 3, 0, 1), _abi.PlanarAdam(5e-3, 3, -4, 1),
                _abi.PlanarAdam(NAN, 3, 1, 1), _abi.PlanarAdam(INF, 3, 1, 1), _abi.PlanarAdam(5e-3, 16, 1, 1), _abi.PlanarAdam(5e-3, -1, 1, 1)):
        assert steps(a=bad) == INVALID, (bad.lr, bad.pin, bad.first_step, bad.n_steps)
    # gq and gqd are nullable together only
    assert trk.trk_scene2d_traj_cost_grad(scene, C.byref(o), buf, buf, 2, 8, buf, buf, None, None) == INVALID
    # the persistent kernel holds whole trajectories in a workgroup
    assert steps(horizon=257) == UNSUPPORTED and steps(horizon=257, batch=0) == UNSUPPORTED
    assert b"256" in trk.trk_last_error()
    # an empty batch returns at once
    assert steps(batch=0, horizon=256) == _abi.TRK_OK and cost_grad(batch=0, horizon=100000) == _abi.TRK_OK


def test_only_a_planar_task_has_the_trajectory_optimizer():
    task = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=CPU), robot=tra.RobotPointMass3D(tensor_args=CPU), tensor_args=CPU)
    assert not task._planar
    q = torch.zeros(2, 8, 3)
    with pytest.raises(NotImplementedError, match="2-D point mass"):
        task.trajectory_optimizer(q, q.clone(), 0.1, 1.0)
    planar = tra.PlanningTask(env=tra.EnvNarrowPassageDense2D(tensor_args=CPU), robot=tra.RobotPointMass(tensor_args=CPU), tensor_args=CPU)
    assert planar._planar and callable(planar.trajectory_optimizer)
