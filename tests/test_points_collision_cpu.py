"""CPU-only checks of the boolean kernels of the attached-point models (k_pcoll_bi / k_pcoll_bg; trk_rollout_points_collision,
trk_rollout_points_collision_via): the generator writes a unit of its own that defines exactly those two kernels, starts only them
and announces its launcher under the main unit's ident and hashes, without touching the main unit's text; generate_sources lists the
three units; both entry points refuse bad arguments before any device work (point set and cost model are blocks of zeros, never read
beyond their own headers); header, EXPORTS, library and INTEGRATION.md agree; the six compiled kernels use no scratch and fit the
occupancy the generator states."""
import ctypes as C
import hashlib
import json
import re
from pathlib import Path

import pytest

from torch_robotics_amd import _abi, _lib, codegen
from torch_robotics_amd.kinematics import URDF_DIR
from torch_robotics_amd.kinmodel import KinModel
import test_isa_entry_chain_cpu as isa

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "torch_robotics_amd" / "csrc"
NAMES = ("trk_rollout_points_collision", "trk_rollout_points_collision_via")
OK, INVALID = _abi.TRK_OK, _abi.TRK_ERR_INVALID_ARG
IDENTS = list(codegen.SPEC_POINT_ROBOTS)


@pytest.fixture(scope="module")
def trk():
    if not _lib.LIB_PATH.exists():
        _lib.build()
    return _lib.lib()


def _unit(ident):
    urdf, fn = codegen.SPEC_POINT_ROBOTS[ident]
    kin = KinModel.from_urdf(str(URDF_DIR / urdf))
    return kin, fn(kin)


@pytest.mark.parametrize("ident", IDENTS)
def test_unit_defines_starts_and_registers_its_two_kernels(ident):
    kin, pt = _unit(ident)
    src = codegen.generate_points_collision_source(kin, pt, ident)
    defined = re.findall(r"^__global__ void __launch_bounds__\(SPEC_BLOCK, (\d+)\) (k_\w+)\(SpecArgs A\) \{$", src, re.M)
    assert sorted(n for _, n in defined) == ["k_pcoll_bg", "k_pcoll_bi"]
    assert {int(o) for o, _ in defined} == {codegen.POINTS_COLL_OCCUPANCY}
    assert src.count("__global__") == 2
    assert sorted(re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", src)) == ["k_pcoll_bg", "k_pcoll_bi"]
    assert codegen.points_collision_kernels(ident) == [f"spec_{ident}::k_pcoll_bi", f"spec_{ident}::k_pcoll_bg"]
    assert f"namespace spec_{ident} {{" in src
    # registration: the main unit's ident and hashes (what its SpecEntry carries), the argument struct's size, the launcher
    reg = re.findall(r"trk_spec_register_points_coll\(([^;]*)\);", src)
    assert len(reg) == 1 and "trk_spec_register(" not in src and "SpecEntry k" not in src
    args = [a.strip() for a in reg[0].split(",")]
    phash = codegen.points_hash(pt.point_link, pt.point_offset)
    assert args == [f'"{ident}"', f"0x{codegen.model_hash(kin):016x}ull", f"0x{phash:016x}ull", "(uint32_t)sizeof(SpecArgs)", "launch_pcoll"]
    main = codegen.generate_points_rollout_source(kin, pt, ident)
    entry = [f.strip() for f in re.search(r"static const SpecEntry kEntry = \{(.*)\};", main).group(1).split(",")]
    assert entry[9] == args[0] and entry[1] == args[1] and entry[12] == args[2]
    assert re.search(r"^static void launch_pcoll\(const SpecEntry\*, const SpecArgs& a, int base_identity, hipStream_t st\) \{$", src, re.M)
    # the boolean twin: k_coll's head and tail, the scene and pair tests, and nothing of the cost rollout's outputs
    for body in re.findall(r"^__global__.*?^\}$", src, re.M | re.S):
        for needle in ("spec_load_q_via<D>", "spec_load_q<D>", "spec_load_spheres_finish", "spec_via_partial_flags(", "A.coll_out[base + lane]"):
            assert body.count(needle) == 1, needle
        groups = [int(n) for n in re.findall(r"spec_collision_links<(\d+)>", body)]
        assert sum(groups) == len(pt.obj_cols) and max(groups) <= codegen.OBJ_GROUP
        assert body.count("spec_self_hit(") == len(pt.self_pairs)
        for absent in ("pf0", "pt0", "link_pos", "spec_flush_chunk", "store_wt", "row[", "gq", "cost"):
            assert absent not in body, absent
    # every pair is tested once, with its own margin, when the walk has produced both columns
    assert sorted(int(k) for k in re.findall(r"self_margin\)\[(\d+)\]", src)) == sorted(2 * list(range(len(pt.self_pairs))))


def test_the_main_units_keep_their_text():
    """tests/golden/spec_points_units_r10.json: sha1 of generate_points_rollout_source's output for the three models before the
    boolean units existed -- the new generator entry shares _PointsUnit and the emitters with it and must not move a character."""
    want = json.loads((ROOT / "tests" / "golden" / "spec_points_units_r10.json").read_text())
    assert sorted(want) == sorted(IDENTS)
    for ident in IDENTS:
        kin, pt = _unit(ident)
        assert hashlib.sha1(codegen.generate_points_rollout_source(kin, pt, ident).encode()).hexdigest() == want[ident], ident
        u = codegen._PointsUnit(kin, pt, ident)
        assert not any("pcoll" in k for k in u.kernels)


def test_generate_sources_lists_the_three_units(tmp_path):
    names = codegen.generate_sources(tmp_path)
    coll = [f"spec_{i}_coll.hip" for i in IDENTS]
    assert names[-3:] == coll and len(set(names)) == len(names)
    for ident in IDENTS:
        kin, pt = _unit(ident)
        assert (tmp_path / f"spec_{ident}_coll.hip").read_text() == codegen.generate_points_collision_source(kin, pt, ident)
        assert (tmp_path / f"spec_{ident}.hip").read_text() == codegen.generate_points_rollout_source(kin, pt, ident)


def test_header_exports_library_and_documentation_agree(trk):
    header = (ROOT / "include" / "trk.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(trk_[a-z0-9_]+)\s*\(", header, flags=re.M))
    doc = (ROOT / "INTEGRATION.md").read_text()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS and hasattr(trk, name) and f"`{name}`" in doc, name
        assert getattr(trk, name).argtypes is not None


def test_bad_arguments_are_refused_before_any_device_work(trk):
    ps = (C.c_char * 8192)()                # stand for TrkPointSet* / TrkCostModel*: zeroed blocks -- a point set of no model
    cm = (C.c_char * 8192)()
    buf = (C.c_float * 4096)()              # host memory standing for the device buffers, never read
    nan = float("nan")

    def err():
        return trk.trk_last_error().decode()

    def coll(p=ps, c=cm, fields=7, q=buf, batch=2, horizon=8, out=buf, ws=None):
        return trk.trk_rollout_points_collision(p, c, fields, q, batch, horizon, nan, out, ws, None)

    def via(p=ps, c=cm, fields=7, x=buf, n_traj=2, horizon=8, S=7, n=5, alpha=buf, beta=buf, qmin=None, qmax=None, out=buf, flags=None):
        return trk.trk_rollout_points_collision_via(p, c, fields, x, n_traj, horizon, S, n, alpha, beta, 0.0, qmin, qmax, out, flags, None)

    for fn, name in ((coll, NAMES[0]), (via, NAMES[1])):
        assert fn(p=None) == INVALID and "null point set" in err() and err().startswith(name + ":")
        assert fn(c=None) == INVALID and "null cost model" in err()
        for f in (0, 8, -1, 15):
            assert fn(fields=f) == INVALID and "bad fields" in err(), f
        # sound arguments get as far as the handles: the zeroed block is a point set of no model
        for f in range(1, 8):
            assert fn(fields=f) == INVALID and "belongs to no model" in err(), f
        assert fn(out=None) == INVALID and "in_collision" in err()
    assert coll(batch=-1) == INVALID and "bad batch/horizon" in err()
    assert via(n_traj=-1) == INVALID and "bad batch/horizon" in err()
    assert coll(q=None) == INVALID and "null q" in err()
    assert via(x=None) == INVALID and "null x" in err()
    for h in (0, -3):
        assert coll(horizon=h) == INVALID and "bad batch/horizon" in err(), h
    assert coll(horizon=1) == INVALID and "belongs to no model" in err()
    for h in (1, 0, -3):
        assert via(horizon=h) == INVALID and "bad batch/horizon" in err(), h
    for n in (0, -1):
        assert via(n=n) == INVALID and "n_interp" in err(), n
    assert via(alpha=None) == INVALID and via(beta=None) == INVALID and via(S=0) == INVALID
    # the flags buffer and both limits: all or none
    for kw in (dict(flags=buf), dict(qmin=buf), dict(qmax=buf), dict(flags=buf, qmin=buf), dict(flags=buf, qmax=buf), dict(qmin=buf, qmax=buf)):
        assert via(**kw) == INVALID and "given together" in err(), sorted(kw)
    assert via(flags=buf, qmin=buf, qmax=buf) == INVALID and "belongs to no model" in err()
    # an empty batch needs no buffers, but still a sound point set
    assert coll(batch=0, q=None, out=None) == INVALID and "belongs to no model" in err()


@pytest.fixture(scope="module")
def coll_isa(tmp_path_factory):
    d = tmp_path_factory.mktemp("pcoll_isa")
    meta = {}
    for ident in IDENTS:
        kin, pt = _unit(ident)
        src = d / f"spec_{ident}_coll.hip"
        src.write_text(codegen.generate_points_collision_source(kin, pt, ident))
        asm = isa._device_asm(src, d / f"spec_{ident}_coll.s")
        for n in isa._kernels(asm):
            blk = re.search(r"\.amdhsa_kernel\s+" + re.escape(n) + r"\n(.*?)\.end_amdhsa_kernel", asm, flags=re.S).group(1)
            meta[n] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(private_segment_fixed_size|next_free_vgpr|accum_offset)\s+(\d+)", blk)}
    return meta


def test_isa_no_scratch_and_the_stated_occupancy(coll_isa):
    assert len(coll_isa) == 6 and all("k_pcoll_b" in n for n in coll_isa), sorted(coll_isa)        # 3 units x 2 bases
    for n, m in sorted(coll_isa.items()):
        vgprs = m["next_free_vgpr"]
        print(f"{n}: private segment {m['private_segment_fixed_size']} B, {vgprs} VGPRs (incl. AGPRs) -> {512 // (-(-vgprs // 8) * 8)} wavefronts per SIMD")
        assert m["private_segment_fixed_size"] == 0, n
        # gfx950: 512 registers per lane and SIMD, allocated in blocks of 8
        assert 512 // (-(-vgprs // 8) * 8) >= codegen.POINTS_COLL_OCCUPANCY, (n, vgprs)


SELF_MARGIN = 0.15          # tests/test_gpu_points_collision.py runs the self-collision mask at this override margin too


@pytest.mark.parametrize("name, lo, hi", [("spheres", 0.015, 0.022), ("grasp", 0.038, 0.046), ("both", 0.038, 0.046)])
def test_self_margin_of_the_gpu_tests_gives_both_outcomes(oracle_lib, name, lo, hi):
    """The fp64 oracle alone, on the GPU tests' 4133 uniform configurations: self-collision hits 0 - 1 % of them at the override margins
    0.0 and 0.07 -- too few to see both outcomes at every batch size -- and 1.8 % (45 spheres: pairs of link origins) / 4.2 % (with the
    grasped box) at SELF_MARGIN; no sample is unstable there (the oracle's answer at SELF_MARGIN -+ 1e-5)."""
    import numpy as np
    import torch
    import torch_robotics_amd as tra
    cpu = dict(device=torch.device("cpu"), dtype=torch.float32)
    box = lambda: tra.GraspedObjectPandaBox(tensor_args=cpu)
    robot = {"spheres": lambda: tra.RobotPanda(link_sphere_model="panda", tensor_args=cpu),
             "grasp": lambda: tra.RobotPanda(grasped_object=box(), tensor_args=cpu),
             "both": lambda: tra.RobotPanda(link_sphere_model="panda", grasped_object=box(), tensor_args=cpu)}[name]()
    task = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=cpu), robot=robot, obstacle_cutoff_margin=0.03, tensor_args=cpu)
    pl, po = robot.collision_point_set()
    orc = oracle_lib.Oracle(robot.diff_panda._kin, task.build_cost_spec())
    q = np.random.default_rng(11).uniform(robot.q_min_np.astype(np.float64), robot.q_max_np.astype(np.float64), (4133, 7)).astype(np.float32)
    pos = orc.fk_points(pl, po, q.astype(np.float64), "f64")
    share = lambda m: float(orc.collision_fields(_abi.FIELD_SELF, pos, m, "f64").mean())
    print(name, "self-collision hit share at margins 0.0 / 0.07 / SELF_MARGIN:", share(0.0), share(0.07), share(SELF_MARGIN))
    assert share(0.0) == 0.0 and share(0.07) < 0.011
    assert lo < share(SELF_MARGIN) < hi
    a, b = (orc.collision_fields(_abi.FIELD_SELF, pos, SELF_MARGIN + d, "f64") for d in (-1e-5, 1e-5))
    assert int((a != b).sum()) <= 2
