"""CPU-only checks of the 2-D point mass's via-point entry points (trk_scene2d_traj_via_cost_grad, trk_scene2d_traj_via_adam_steps):
header, EXPORTS, library and INTEGRATION.md agree, the ctypes struct has the header's layout, bad arguments are refused before any
device work (the scene pointer of these calls is a block of zeros that is never read), only a planar task hands out the optimiser, and
every instantiation of the two loop kernels compiles for gfx950 without scratch at the occupancy DESIGN.md 6b records."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

import torch_robotics_amd as tra
import test_planar_traj_cpu as base
from torch_robotics_amd import _abi, _lib

ROOT = Path(__file__).resolve().parent.parent
CPU = dict(device=torch.device("cpu"), dtype=torch.float32)
NEW = ("trk_scene2d_traj_via_cost_grad", "trk_scene2d_traj_via_adam_steps")
INVALID, UNSUPPORTED = _abi.TRK_ERR_INVALID_ARG, _abi.TRK_ERR_UNSUPPORTED
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def trk():
    if not _lib.LIB_PATH.exists():
        _lib.build()
    return _lib.lib()


def test_header_exports_library_and_integration_agree(trk):
    header = (ROOT / "include" / "trk.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(trk_[a-z0-9_]+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(trk, name)
        assert name in (ROOT / "INTEGRATION.md").read_text()
    assert re.search(r"#define\s+TRK_ABI_VERSION\s+5\b", header) and _abi.TRK_ABI_VERSION == 5      # additive: the version stays


def test_struct_layout_matches_header():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "trk.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n",' \
          'sizeof(TrkPlanarViaObjective),offsetof(TrkPlanarViaObjective,w_via),offsetof(TrkPlanarViaObjective,n_interp),' \
          'offsetof(TrkPlanarViaObjective,alpha),offsetof(TrkPlanarViaObjective,beta));}'
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")], check=True)
        out = subprocess.run([str(Path(d) / "s")], capture_output=True, text=True, check=True).stdout.split()
    V = _abi.PlanarViaObjective
    assert [int(v) for v in out] == [C.sizeof(V), V.w_via.offset, V.n_interp.offset, V.alpha.offset, V.beta.offset]
    assert V.base.offset == 0 and V.w_via.offset == C.sizeof(_abi.PlanarObjective)


def test_bad_arguments_are_refused_before_any_device_work(trk):
    scene = (C.c_char * 4096)()             # stands for a TrkScene2D*: no call below may reach the point where it is read
    buf = (C.c_float * 4096)()              # host memory standing for the device buffers and weights, never read either
    w = C.addressof(buf)
    ad = _abi.PlanarAdam(5e-3, 3, 1, 1)

    def via(ob=None, w_via=1.0, n=5, alpha=w, beta=w):
        return _abi.PlanarViaObjective(ob if ob is not None else base.objective(), w_via, n, alpha, beta)

    o = via()

    def cost_grad(s=scene, ob=o, batch=2, horizon=8, q=buf, qd=buf, cost=buf):
        return trk.trk_scene2d_traj_via_cost_grad(s, C.byref(ob) if ob is not None else None, q, qd, batch, horizon, cost, buf, buf, None)

    def steps(s=scene, ob=o, a=ad, batch=2, horizon=8, q=buf, qd=buf, cost=buf):
        return trk.trk_scene2d_traj_via_adam_steps(s, C.byref(ob) if ob is not None else None, C.byref(a) if a is not None else None,
                                                   q, qd, buf, buf, batch, horizon, cost, None)

    for fn in (cost_grad, steps):
        assert fn(s=None) == INVALID and fn(ob=None) == INVALID
        assert fn(q=None) == INVALID and fn(qd=None) == INVALID
        assert fn(ob=via(alpha=None)) == INVALID and fn(ob=via(beta=None)) == INVALID
        assert fn(ob=via(n=0)) == INVALID and fn(ob=via(n=-2)) == INVALID
        for bad in (NAN, INF, -INF):
            assert fn(ob=via(w_via=bad)) == INVALID, bad
        assert fn(batch=-1) == INVALID and fn(horizon=0) == INVALID and fn(horizon=-3) == INVALID
        for kw in base.BAD_OBJECTIVES:
            assert fn(ob=via(ob=base.objective(**kw))) == INVALID, kw
        assert (b"trk_scene2d_traj_via_cost_grad" if fn is cost_grad else b"trk_scene2d_traj_via_adam_steps") in trk.trk_last_error()
        # one layout: a workgroup owns whole trajectories in BOTH calls
        assert fn(horizon=257) == UNSUPPORTED and fn(horizon=257, batch=0) == UNSUPPORTED
        assert b"256" in trk.trk_last_error() and b"trk_scene2d_traj_via" in trk.trk_last_error()
        # an empty batch returns at once
        assert fn(batch=0, horizon=256) == _abi.TRK_OK and fn(batch=0, horizon=1) == _abi.TRK_OK
    assert cost_grad(cost=None) == INVALID
    assert steps(a=None) == INVALID
    for bad in (_abi.PlanarAdam(5e-3, 3, 1, -1), _abi.PlanarAdam(5e-3, 3, 0, 1), _abi.PlanarAdam(5e-3, 3, -4, 1),
                _abi.PlanarAdam(NAN, 3, 1, 1), _abi.PlanarAdam(INF, 3, 1, 1), _abi.PlanarAdam(5e-3, 16, 1, 1), _abi.PlanarAdam(5e-3, -1, 1, 1)):
        assert steps(a=bad) == INVALID, (bad.lr, bad.pin, bad.first_step, bad.n_steps)
    # gq and gqd are nullable together only
    assert trk.trk_scene2d_traj_via_cost_grad(scene, C.byref(o), buf, buf, 2, 8, buf, buf, None, None) == INVALID
    assert trk.trk_scene2d_traj_via_cost_grad(scene, C.byref(o), buf, buf, 2, 8, buf, None, buf, None) == INVALID
    # cost is nullable in the loop; with lr = 0 as well there is nothing to do, and the call returns before the scene is read
    assert steps(a=_abi.PlanarAdam(0.0, 3, 1, 4), cost=None) == _abi.TRK_OK


def test_only_a_planar_task_takes_the_via_keywords():
    task = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=CPU), robot=tra.RobotPointMass3D(tensor_args=CPU), tensor_args=CPU)
    q = torch.zeros(2, 8, 3)
    with pytest.raises(NotImplementedError, match="2-D point mass"):
        task.trajectory_optimizer(q, q.clone(), 0.1, 1.0, num_interpolation=5)
    with pytest.raises(NotImplementedError, match="2-D point mass"):
        task.trajectory_optimizer(q, q.clone(), 0.1, 1.0, w_via=4.0, num_interpolation=5, pin_goal_vel=True)


# DESIGN.md 6b, "via-point term": wavefronts per SIMD of k_planar_traj_via by variant -- 7 where the analytic objects are walked
# (66 - 68 VGPRs), 8 everywhere else (41 - 55 VGPRs); 32 instantiations = grid x analytic x workspace x clamp x WAVE
MIN_WAVES = {True: 7, False: 8}
# k_planar_traj_adam, the same loop body without the via term: 8 in all 32 (30 - 55 VGPRs) -- what a compile of the commit before the
# two kernels shared their body gives for every variant, and what DESIGN.md 6b's paragraph on the kernel records
MIN_WAVES_PLAIN = 8


def test_every_instantiation_compiles_without_scratch_at_the_recorded_occupancy():
    csrc = ROOT / "torch_robotics_amd" / "csrc"
    make = (csrc / "Makefile").read_text()
    hipcc = re.search(r"^HIPCC \?= (.*)$", make, flags=re.M).group(1).strip()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", make, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    with tempfile.TemporaryDirectory() as d:
        res = subprocess.run([hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                              "trk_planar.hip", "-o", str(Path(d) / "planar_device.o")], cwd=csrc, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    seen = {"adam": {}, "via": {}}
    for block in re.split(r"remark: [^\n]*Function Name: ", res.stderr)[1:]:
        name = block.split()[0]
        m = re.match(r"_ZN\d+_GLOBAL__N_1\d+k_planar_traj_(adam|via)ILb([01])ELb([01])ELb([01])ELb([01])ELb([01])EEE", name)
        if not m:
            continue
        num = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))
        seen[m.group(1)][tuple(int(v) for v in m.groups()[1:])] = (num("ScratchSize [bytes/lane]"), num("Occupancy [waves/SIMD]"),
                                                                    num("VGPRs"), num("LDS Size [bytes/block]"))
    for kernel, lds_form in (("adam", 8192), ("via", 10240)):
        assert len(seen[kernel]) == 32, (kernel, sorted(seen[kernel]))
        for variant, (scratch, waves, vgprs, lds) in sorted(seen[kernel].items()):
            print(f"k_planar_traj_{kernel}<grid, analytic, workspace, clamp, wave> = {variant}: {vgprs} VGPRs, {waves} waves / SIMD, "
                  f"{lds} B of LDS")
            assert scratch == 0, (kernel, variant)
            assert waves >= (MIN_WAVES_PLAIN if kernel == "adam" else MIN_WAVES[bool(variant[1])]), (kernel, variant, waves, vgprs)
            assert lds == (0 if variant[4] else lds_form), (kernel, variant, lds)
