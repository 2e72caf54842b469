"""CPU-only checks of the 3-D point mass's trajectory entries (trk_point3d_traj_cost_grad, trk_point3d_traj_adam_steps): header,
EXPORTS, library and INTEGRATION.md agree; every refusal of include/trk.h comes before any device work (the cost model of these calls
is a block of zeros with fields of its header set through a ctypes mirror of DevCostHdr, never read beyond the header, and the
buffers are host memory that is never read); the four instantiations of k_point3d_traj compile for gfx950 without scratch, with the LDS and at the occupancy DESIGN.md 6d records; the task
hands the plan out only where it holds, and the older plan methods still refuse the 3-D point mass in their own words; the cases of
point3d_traj_helpers exercise the hinge; and the fp64 reference's gradient is the derivative of its own cost."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

import torch_robotics_amd as tra
import point3d_traj_helpers as p3
from torch_robotics_amd import _abi, _lib

ROOT = Path(__file__).resolve().parent.parent
CPU = dict(device=torch.device("cpu"), dtype=torch.float32)
NEW = ("trk_point3d_traj_cost_grad", "trk_point3d_traj_adam_steps", "trk_point3d_last_form")
OK, INVALID, UNSUPPORTED = _abi.TRK_OK, _abi.TRK_ERR_INVALID_ARG, _abi.TRK_ERR_UNSUPPORTED
NAN, INF = float("nan"), float("inf")
W, G, A, V = _abi.RolloutWeights, _abi.GpPrior, _abi.TrajAdam, _abi.TrajVia
BUF = (C.c_float * 4096)()
PTR = C.addressof(BUF)


@pytest.fixture(scope="module")
def trk():
    if not _lib.LIB_PATH.exists():
        _lib.build()
    return _lib.lib()


class DevGrid(C.Structure):             # csrc/trk_device.h
    _fields_ = [("nb1", C.c_int32), ("nb2", C.c_int32), ("_pad", C.c_int32 * 2), ("cells", C.c_void_p), ("dims", C.c_int32 * 3),
                ("lim_min", C.c_float * 3), ("map_dim", C.c_float * 3), ("fdims", C.c_float * 3)]


class DevCostHdr(C.Structure):          # csrc/trk_device.h, field for field; the first member of TrkCostModel (csrc/trk_capi.hip)
    _fields_ = [("n_links_in", C.c_int32), ("n_obj_links", C.c_int32), ("n_objects", C.c_int32), ("has_grid", C.c_int32), ("has_ws", C.c_int32),
                ("n_self_links", C.c_int32), ("n_self_pairs", C.c_int32), ("ee_link", C.c_int32), ("ee_square", C.c_int32),
                ("ee_w_pos", C.c_float), ("ee_w_rot", C.c_float), ("ws_min", C.c_float * 3), ("ws_max", C.c_float * 3),
                ("ws_c", C.c_float * 3), ("ws_h", C.c_float * 3), ("ee_target", C.c_float * 16),
                ("ee2_link", C.c_int32), ("_pad_ee2", C.c_int32), ("ee2_target", C.c_float * 16),
                ("obj_link_idx", C.c_void_p), ("obj_link_margin", C.c_void_p), ("objects", C.c_void_p), ("prims", C.c_void_p),
                ("self_pairs", C.c_void_p), ("self_margin", C.c_void_p), ("spheres", C.c_void_p), ("spheres_sel", C.c_void_p),
                ("n_spheres", C.c_int32), ("spheres_uniform_r", C.c_int32), ("sphere_r", C.c_float), ("n_box_objects", C.c_int32),
                ("box_objects", C.c_void_p), ("grid", DevGrid), ("sphere_pairs", C.c_void_p),
                ("n_sphere_pairs", C.c_int32), ("clamp_fields", C.c_int32), ("n_virtual", C.c_int32), ("self_single", C.c_int32),
                ("virtual_src", C.c_void_p), ("virtual_w", C.c_void_p), ("n_prims", C.c_int32), ("_pad_prims", C.c_int32),
                ("sphere_o", C.c_float * 3), ("sphere_rho2", C.c_float)]


def cost_model(n_links_in=1, n_obj_links=1, n_self_pairs=0, ee_link=-1, ee2_link=-1, n_virtual=0):
    """stands for a TrkCostModel*: a block of zeros with these fields of its header set (no tracked link unless one is asked for);
    the entries read nothing but the header"""
    cm = (C.c_char * 8192)()
    h = DevCostHdr.from_buffer(cm)
    h.n_links_in, h.n_obj_links, h.n_self_pairs, h.ee_link, h.ee2_link, h.n_virtual = n_links_in, n_obj_links, n_self_pairs, ee_link, ee2_link, n_virtual
    return cm


def test_the_header_mirror_has_the_library_layout(trk):
    """the ctypes DevCostHdr above against the library's own sizeof(DevCostHdr) (trk_spec_layout_stamp) and the offsets that the C
    compiler gives the fields these tests set: a drifted mirror would make the refusal tests below set other fields than they name"""
    stamp = (C.c_int64 * 3)()
    assert trk.trk_spec_layout_stamp(stamp) == 0 and stamp[2] == C.sizeof(DevCostHdr)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include <stdint.h>\ntypedef struct { float x, y, z, w; } float4;\n'
           + re.search(r"struct DevGrid \{.*?\n\};", (ROOT / "torch_robotics_amd" / "csrc" / "trk_device.h").read_text(), flags=re.S).group(0)
           + "\n" + re.search(r"struct DevCostHdr \{.*?\n\};", (ROOT / "torch_robotics_amd" / "csrc" / "trk_device.h").read_text(), flags=re.S).group(0)
           + '\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n",sizeof(DevCostHdr),offsetof(DevCostHdr,n_obj_links),'
             'offsetof(DevCostHdr,n_self_pairs),offsetof(DevCostHdr,ee_link),offsetof(DevCostHdr,ee2_link),offsetof(DevCostHdr,n_virtual),'
             'offsetof(DevCostHdr,virtual_src));}')
    src = src.replace("const DevObj*", "const void*").replace("const DevPrim*", "const void*")
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.cpp").write_text(src)
        subprocess.run(["g++", str(Path(d) / "s.cpp"), "-o", str(Path(d) / "s")], check=True)
        out = subprocess.run([str(Path(d) / "s")], capture_output=True, text=True, check=True).stdout.split()
    H = DevCostHdr
    assert [int(v) for v in out] == [C.sizeof(H), H.n_obj_links.offset, H.n_self_pairs.offset, H.ee_link.offset, H.ee2_link.offset,
                                     H.n_virtual.offset, H.virtual_src.offset]


CM = cost_model()


def _ref(s):
    return C.byref(s) if s is not None else None


def cost_grad(trk, cm=CM, w=(0.0, 1.0, 1.0, 0.0), g=(0.08, 1.0, 1.0), v=None, alpha=PTR, beta=PTR, q=BUF, qd=BUF, batch=2, horizon=8,
              cost=BUF, gq=BUF, gqd=BUF):
    w, g = (None if x is None else T(*x) for T, x in ((W, w), (G, g)))
    via = None if v is None else V(v[0], v[1], alpha, beta)
    return trk.trk_point3d_traj_cost_grad(cm, _ref(w), _ref(g), _ref(via), q, qd, batch, horizon, cost, gq, gqd, None)


def adam_steps(trk, cm=CM, w=(0.0, 1.0, 1.0, 0.0), g=(0.08, 1.0, 1.0), v=None, alpha=PTR, beta=PTR, a=(5e-3, 3, 1, 1), q=BUF, qd=BUF,
               am=BUF, av=BUF, batch=2, horizon=8, cost=BUF):
    w, g, a = (None if x is None else T(*x) for T, x in ((W, w), (G, g), (A, a)))
    via = None if v is None else V(v[0], v[1], alpha, beta)
    return trk.trk_point3d_traj_adam_steps(cm, _ref(w), _ref(g), _ref(via), _ref(a), q, qd, am, av, batch, horizon, cost, None)


def err(trk):
    return trk.trk_last_error().decode()


def test_header_exports_library_and_integration_agree(trk):
    header = (ROOT / "include" / "trk.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(trk_[a-z0-9_]+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(trk, name)
        assert name in (ROOT / "INTEGRATION.md").read_text()
    assert re.search(r"#define\s+TRK_POINT3D_MAX_HORIZON\s+256\b", header) and _abi.TRK_POINT3D_MAX_HORIZON == 256
    assert re.search(r"#define\s+TRK_ABI_VERSION\s+5\b", header) and _abi.TRK_ABI_VERSION == 5      # additive: the version stays
    assert trk.trk_point3d_last_form() == _abi.TRK_POINT3D_FORM_NONE          # nothing was launched by this thread
    assert re.search(r"TRK_POINT3D_FORM_NONE = 0, TRK_POINT3D_FORM_DPP = 1, TRK_POINT3D_FORM_LDS = 2", header)
    assert (_abi.TRK_POINT3D_FORM_DPP, _abi.TRK_POINT3D_FORM_LDS) == (1, 2)
    assert hasattr(tra.ops, "point3d_traj_cost_grad") and hasattr(tra.ops, "Point3DAdamPlan")
    assert hasattr(tra.PlanningTask, "point_mass_3d_optimizer")


@pytest.mark.parametrize("entry", (cost_grad, adam_steps), ids=lambda e: e.__name__)
def test_invalid_arguments_are_refused_before_any_device_work(trk, entry):
    who = "trk_point3d_traj_" + entry.__name__
    # ---- null pointers
    for name in ("cm", "w", "g", "q", "qd"):
        assert entry(trk, **{name: None}) == INVALID and err(trk).startswith(who + ":"), name
    if entry is cost_grad:
        assert entry(trk, cost=None) == INVALID
        # gq and gqd are nullable together only
        assert entry(trk, gq=None) == INVALID and "only one of gq / gqd" in err(trk)
        assert entry(trk, gqd=None) == INVALID and "only one of gq / gqd" in err(trk)
    else:
        assert entry(trk, a=None) == INVALID and "TrkTrajAdam" in err(trk)
        assert entry(trk, am=None) == INVALID and entry(trk, av=None) == INVALID
    # ---- non-finite weights / dt / sigma (or <= 0) / lr
    for k in range(4):
        for bad in (NAN, INF, -INF):
            w = [0.0, 1.0, 1.0, 0.0]
            w[k] = bad
            assert entry(trk, w=tuple(w)) == INVALID and "weights must be finite" in err(trk), (k, bad)
    for bad in (NAN, INF, 0.0, -0.1):
        assert entry(trk, g=(bad, 1.0, 1.0)) == INVALID and entry(trk, g=(0.08, bad, 1.0)) == INVALID, bad
    for bad in (NAN, INF):
        assert entry(trk, g=(0.08, 1.0, bad)) == INVALID, bad
    if entry is adam_steps:
        for bad in ((NAN, 3, 1, 1), (INF, 3, 1, 1), (5e-3, -1, 1, 1), (5e-3, 16, 1, 1), (5e-3, 3, 0, 1), (5e-3, 3, -4, 1), (5e-3, 3, 1, -1)):
            assert entry(trk, a=bad) == INVALID and "pin in 0 .. 15" in err(trk), bad
    # ---- the via struct
    assert entry(trk, v=(1.0, 2), alpha=None) == INVALID and "alpha / beta" in err(trk)
    assert entry(trk, v=(1.0, 2), beta=None) == INVALID and "alpha / beta" in err(trk)
    for n in (0, -1):
        assert entry(trk, v=(1.0, n)) == INVALID and "n_interp" in err(trk), n
    for bad in (NAN, INF, -INF):
        assert entry(trk, v=(bad, 2)) == INVALID and "w_via" in err(trk), bad
    # ---- batch and horizon
    assert entry(trk, batch=-1) == INVALID and entry(trk, horizon=0) == INVALID and entry(trk, horizon=-3) == INVALID
    # ---- an argument error speaks before the horizon's and the cost model's refusals, and with an empty batch too
    assert entry(trk, horizon=257, g=(NAN, 1.0, 1.0)) == INVALID
    assert entry(trk, batch=0, horizon=257, w=None) == INVALID
    assert entry(trk, cm=cost_model(n_links_in=7), batch=0, v=(NAN, 2)) == INVALID


@pytest.mark.parametrize("entry", (cost_grad, adam_steps), ids=lambda e: e.__name__)
def test_unsupported_calls_say_why_before_any_device_work(trk, entry):
    # the horizon, with the route for other horizons -- also with an empty batch
    for batch in (2, 0):
        assert entry(trk, horizon=257, batch=batch) == UNSUPPORTED
        assert "TRK_POINT3D_MAX_HORIZON (256)" in err(trk) and "trk_cost_fields + trk_gp_prior_cost_grad" in err(trk)
    # columns that are not exactly one point
    # columns that are not exactly one point: n_links_in != 1, virtual columns, no or more than one object-collision column
    for kw in (dict(n_links_in=0), dict(n_links_in=11, n_obj_links=1), dict(n_obj_links=0), dict(n_obj_links=2), dict(n_virtual=1),
               dict(n_virtual=3)):
        for batch in (2, 0):
            assert entry(trk, cm=cost_model(**kw), batch=batch) == UNSUPPORTED and "exactly one point" in err(trk), kw
    # self pairs / a tracked link (either of the two), each alone, with a weight that is not zero ...
    for kw, w in ((dict(n_self_pairs=1), (1.0, 1.0, 1.0, 0.0)), (dict(ee_link=0), (0.0, 1.0, 1.0, 0.5)), (dict(ee2_link=0), (0.0, 1.0, 1.0, 0.5))):
        for batch in (2, 0):
            assert entry(trk, cm=cost_model(**kw), w=w, batch=batch) == UNSUPPORTED and "w_self / w_ee" in err(trk), kw
    # ... and not the other term's weight, nor a weight on a term the cost model does not have; with zero weights all are served
    assert entry(trk, cm=cost_model(n_self_pairs=1), w=(0.0, 1.0, 1.0, 0.5), batch=0) == OK
    assert entry(trk, cm=cost_model(ee_link=0), w=(1.0, 1.0, 1.0, 0.0), batch=0) == OK
    assert entry(trk, cm=cost_model(ee2_link=0), w=(1.0, 1.0, 1.0, 0.0), batch=0) == OK
    assert entry(trk, w=(1.0, 1.0, 1.0, 0.5), batch=0) == OK
    assert entry(trk, cm=cost_model(n_self_pairs=1, ee_link=0, ee2_link=0), batch=0) == OK
    # the horizon speaks before the cost model
    assert entry(trk, cm=cost_model(n_links_in=7), horizon=300) == UNSUPPORTED and "TRK_POINT3D_MAX_HORIZON" in err(trk)


@pytest.mark.parametrize("entry", (cost_grad, adam_steps), ids=lambda e: e.__name__)
def test_an_empty_batch_returns_ok_without_a_launch(trk, entry):
    for horizon in (1, 64, 256):
        assert entry(trk, batch=0, horizon=horizon) == OK
        assert entry(trk, batch=0, horizon=horizon, v=(1.0, 5)) == OK
        assert entry(trk, batch=0, horizon=horizon, q=None, qd=None) == OK          # nothing to point at
    if entry is adam_steps:
        # no update and no cost asked for: nothing to do, whatever the batch
        assert entry(trk, a=(0.0, 3, 1, 4), cost=None) == OK and entry(trk, a=(5e-3, 3, 1, 0), cost=None, am=None, av=None) == OK


# wavefronts per SIMD of k_point3d_traj<WAVE, VIA> (69 - 71 VGPRs without the via term, 82 with it) and the LDS of the
# exchange: 2 buffers x 6 components x 256 lanes x 4 bytes, + 3 x 256 x 4 for U with the via term
MIN_WAVES = {False: 7, True: 5}         # by VIA
LDS_BYTES = {False: 12288, True: 15360}


def test_every_instantiation_compiles_without_scratch_at_the_recorded_occupancy():
    csrc = ROOT / "torch_robotics_amd" / "csrc"
    make = (csrc / "Makefile").read_text()
    assert re.search(r"^SRCS := .*\btrk_point3d\.hip\b", make, flags=re.M)
    hipcc = re.search(r"^HIPCC \?= (.*)$", make, flags=re.M).group(1).strip()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", make, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    with tempfile.TemporaryDirectory() as d:
        res = subprocess.run([hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "trk_point3d.hip", "-o",
                              str(Path(d) / "point3d_device.o")], cwd=csrc, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    seen = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", res.stderr)[1:]:
        m = re.match(r"_ZN\d+_GLOBAL__N_1\d+k_point3d_trajILb([01])ELb([01])EEE", block.split()[0])
        if not m:
            continue
        num = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))
        seen[tuple(bool(int(v)) for v in m.groups())] = (num("ScratchSize [bytes/lane]"), num("Occupancy [waves/SIMD]"), num("VGPRs"),
                                                         num("LDS Size [bytes/block]"))
    assert sorted(seen) == [(False, False), (False, True), (True, False), (True, True)], sorted(seen)
    for (wave, via), (scratch, waves, vgprs, lds) in sorted(seen.items()):
        print(f"k_point3d_traj<WAVE={wave}, VIA={via}>: {vgprs} VGPRs, {waves} waves / SIMD, {lds} B of LDS")
        assert scratch == 0, (wave, via)
        assert waves >= MIN_WAVES[via], (wave, via, waves, vgprs)
        assert lds == (0 if wave else LDS_BYTES[via]), (wave, via, lds)


def test_the_task_hands_the_plan_out_only_where_it_holds():
    q = torch.zeros(2, 8, 3)
    # a robot with a tree, the 2-D point mass and a self-collision field are sent to the right method
    arm = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=CPU), robot=tra.RobotPanda(tensor_args=CPU), tensor_args=CPU)
    with pytest.raises(NotImplementedError, match="rollout_adam_plan"):
        arm.point_mass_3d_optimizer(torch.zeros(2, 8, 7), torch.zeros(2, 8, 7), 0.1, 1.0)
    grasp = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=CPU),
                             robot=tra.RobotPanda(grasped_object=tra.GraspedObjectPandaBox(tensor_args=CPU), tensor_args=CPU), tensor_args=CPU)
    with pytest.raises(NotImplementedError, match="points_adam_plan"):
        grasp.point_mass_3d_optimizer(torch.zeros(2, 8, 7), torch.zeros(2, 8, 7), 0.1, 1.0)
    planar = tra.PlanningTask(env=tra.EnvNarrowPassageDense2D(tensor_args=CPU), robot=tra.RobotPointMass(tensor_args=CPU), tensor_args=CPU)
    with pytest.raises(NotImplementedError, match="trajectory_optimizer"):
        planar.point_mass_3d_optimizer(torch.zeros(2, 8, 2), torch.zeros(2, 8, 2), 0.1, 1.0)
    task = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=CPU), robot=tra.RobotPointMass3D(tensor_args=CPU), tensor_args=CPU)
    assert task.df_collision_self is None
    task.df_collision_self = object()
    with pytest.raises(NotImplementedError, match="self-collision"):
        task.point_mass_3d_optimizer(q, q.clone(), 0.1, 1.0)
    task.df_collision_self = None
    # the four older plan methods refuse the 3-D point mass as before, word for word
    with pytest.raises(NotImplementedError) as e:
        task.rollout_adam_plan(q, q.clone(), 0.1, 1.0)
    assert str(e.value) == "rollout_adam_plan needs a robot with a kinematic tree (the 2-D point mass has trajectory_optimizer)"
    with pytest.raises(NotImplementedError) as e:
        task.points_adam_plan(q, q.clone(), 0.1, 1.0)
    assert str(e.value) == ("points_adam_plan is for attached-point cost models (link spheres / a grasped object); "
                            "rollout_adam_plan is the planning loop of the link-column models")
    with pytest.raises(NotImplementedError) as e:
        task.trajectory_optimizer(q, q.clone(), 0.1, 1.0)
    assert str(e.value) == ("trajectory_optimizer serves the 2-D point mass (RobotPointMass in a 2-D scene); other robots "
                            "optimise on rollout_gp_plan's gradients")
    with pytest.raises(NotImplementedError) as e:
        task.rollout_via_plan(q)
    assert str(e.value) == ("rollout_via_plan is for link-column cost models of robots with a kinematic tree "
                            "(compute_collision_cost_via serves the others)")
    # the plan itself: tensors on a GPU only, (B, H, 3) fp32, at most 256 samples per trajectory
    cm = object.__new__(tra.ops.CostHandle)
    with pytest.raises(ValueError, match="same GPU"):
        tra.ops.Point3DAdamPlan(cm, (0, 1, 1, 0), q, q.clone(), 0.1, 1.0)
    with pytest.raises(ValueError, match="same GPU"):
        tra.ops.point3d_traj_cost_grad(cm, (0, 1, 1, 0), q, q.clone(), 0.1, 1.0)


@pytest.mark.parametrize("name", list(p3.SCENES))
def test_the_cases_exercise_the_hinge(name, oracle_lib):
    """pooled over the ten shapes, the clamped hinge is positive on at least 10 % of the samples -- on the fp64 reference alone"""
    live, total = 0, 0
    for B, H in p3.SHAPES:
        q, _ = p3.walks(name, B, H)
        f = p3.raw_fields(oracle_lib, name, q.reshape(-1, 3))
        live += int((np.maximum(f, 0.0).sum(-1) > 0).sum())
        total += B * H
    print(f"{name}: the clamped hinge is positive on {live} of {total} samples ({live / total:.3f})")
    assert live >= 0.10 * total


@pytest.mark.parametrize("name", ["spheres", "posed"])
@pytest.mark.parametrize("clamp", (False, True))
def test_the_reference_gradient_is_the_derivative_of_its_cost(name, clamp, oracle_lib):
    """objective64's gradient, via term included, against central differences of its own total cost in fp64 (step 1e-6), on samples away
    from the kinks: rows where every field value of the sample, of its via points and of the via points before it lies more than 1e-4
    from the relu's corner, and where no difference quotient of the row changes when the step is halved (a switch between primitives or
    box faces inside the step).  The voxel grid is left out: its stored gradient is data, not the derivative of its piecewise constant
    distance."""
    spec, raw = p3.spec_of(name, clamp), p3.spec_of(name, False)
    dt, sigma, w = p3.PARAMS[1][:3]
    via = (0.37, 2)
    for B, H in [(3, 3), (4, 12)]:
        q, qd = (x.copy() for x in p3.walks(name, B, H))
        x = np.concatenate([q, qd], -1).astype(np.float64)

        def total(x64):
            # the reference takes fp32 inputs; here its pieces are evaluated on fp64 ones
            q64, qd64 = np.ascontiguousarray(x64[..., :3]), np.ascontiguousarray(x64[..., 3:])
            orc = p3.oracle_of(oracle_lib, spec)
            c = p3.hinge64(orc, q64, *p3.WEIGHTS)[0].sum()
            alpha, beta = (v.astype(np.float64).reshape(1, 1, via[1], 1) for v in p3.via_weights(via[1]))
            pts = q64[:, :-1, None, :] * alpha + q64[:, 1:, None, :] * beta
            c += via[0] * p3.hinge64(orc, pts, *p3.WEIGHTS)[0].sum()
            return c + oracle_lib.gp_prior(q64, qd64, dt, sigma, w, "f64")[0].sum()

        ref = p3.objective64(oracle_lib, spec, q, qd, dt, sigma, w, *p3.WEIGHTS, via=via)
        got = np.concatenate([ref["gq"], ref["gqd"]], -1)
        fd = {}
        for h in (1e-6, 5e-7):
            d = np.zeros_like(x)
            for idx in np.ndindex(*x.shape):
                e = np.zeros_like(x)
                e[idx] = h
                d[idx] = (total(x + e) - total(x - e)) / (2 * h)
            fd[h] = d
        # rows away from kinks
        f0 = p3.raw_fields(oracle_lib, name, q.reshape(-1, 3)).reshape(B, H, 2)
        fv = p3.raw_fields(oracle_lib, name, p3.via_points(q, via[1]).reshape(-1, 3)).reshape(B, H - 1, via[1] * 2)
        far = (np.abs(f0) > 1e-4).all(-1)
        far[:, :H - 1] &= (np.abs(fv) > 1e-4).all(-1)
        far[:, 1:] &= (np.abs(fv) > 1e-4).all(-1)
        scale = max(1.0, np.abs(got).max())
        stable = (np.abs(fd[1e-6] - fd[5e-7]) <= 1e-5 * scale).all(-1)
        rows = far & stable
        print(f"{name} clamp={clamp} {B}x{H}: {int(rows.sum())} of {B * H} rows judged, worst |fd - grad| "
              f"{np.abs(fd[5e-7] - got)[rows].max():.2e} on a scale of {scale:.3g}")
        assert rows.sum() >= 0.5 * B * H
        # absolute, so that it binds on the hinge's gradient (entries of order 1) and not only on the prior's (order 1e3): the
        # difference quotient of a total of ~1e4 carries 1e4 x 2^-53 / 5e-7 ~ 2e-6 of rounding
        assert (np.abs(fd[5e-7] - got)[rows] <= 2e-5).all()
