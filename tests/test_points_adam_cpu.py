"""CPU-only checks of the planning loop of the attached-point models (trk_rollout_points_gp_adam_steps, generated kernels
k_padam_bi / k_padam_bg<FAST>): the generator writes a satellite unit that defines and starts exactly those kernels and announces its
launcher under the main unit's ident and hashes; the kernel body is k_traj_adam's loop around the walk of the points rollout without
any of the rollout's outputs; no earlier unit's text moves; the build lists the units after the via units and in front of the boolean units;
header, EXPORTS, library and INTEGRATION.md agree; bad arguments are refused before any device work (model, point set and cost model
are blocks of zeros, never read beyond their own headers); the twelve compiled instantiations use no scratch and fit the occupancy the
generator states; the task hands each plan out only where it holds; and, on the fp64 oracle alone, the inputs of
tests/test_gpu_points_adam.py exercise both sides of the object hinge."""
import ctypes as C
import hashlib
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import torch_robotics_amd as tra
from torch_robotics_amd import _abi, _lib, codegen
from torch_robotics_amd.kinematics import URDF_DIR
from torch_robotics_amd.kinmodel import KinModel
import test_isa_entry_chain_cpu as isa

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "torch_robotics_amd" / "csrc"
GOLDEN = ROOT / "tests" / "golden"
NAME = "trk_rollout_points_gp_adam_steps"
OK, INVALID, UNSUPPORTED = _abi.TRK_OK, _abi.TRK_ERR_INVALID_ARG, _abi.TRK_ERR_UNSUPPORTED
NAN, INF = float("nan"), float("inf")
IDENTS = list(codegen.SPEC_POINT_ROBOTS)
CPU = dict(device=torch.device("cpu"), dtype=torch.float32)


@pytest.fixture(scope="module")
def trk():
    if not _lib.LIB_PATH.exists():
        _lib.build()
    return _lib.lib()


def _unit(ident):
    urdf, fn = codegen.SPEC_POINT_ROBOTS[ident]
    kin = KinModel.from_urdf(str(URDF_DIR / urdf))
    return kin, fn(kin)


def _sha(text):
    return hashlib.sha1(text.encode()).hexdigest()


@pytest.mark.parametrize("ident", IDENTS)
def test_unit_defines_starts_and_registers_its_kernels(ident):
    kin, pt = _unit(ident)
    assert codegen.points_adam_ok(kin, pt) and codegen._PointsUnit(kin, pt, ident).traj_adam_ok
    src = codegen.generate_points_adam_source(kin, pt, ident)
    defined = re.findall(r"^template <bool FAST>[^\n]*\n__global__ void __launch_bounds__\(SPEC_BLOCK, (\d+)\) (k_\w+)\(TrajAdamArgs A\) \{$", src, re.M)
    assert sorted(n for _, n in defined) == ["k_padam_bg", "k_padam_bi"]
    assert {int(o) for o, _ in defined} == {codegen.POINTS_ADAM_OCCUPANCY}
    assert src.count("__global__") == 2
    started = re.findall(r"hipLaunchKernelGGL\(\((\w+)<(\w+)>\)", src)
    assert sorted(started) == sorted((k, f) for k in ("k_padam_bi", "k_padam_bg") for f in ("true", "false"))
    assert codegen.points_adam_kernels(ident) == [f"spec_{ident}::k_padam_{b}<{f}>" for b in ("bi", "bg") for f in ("true", "false")]
    assert f"namespace spec_{ident} {{" in src
    # one launcher, which chooses the instantiation as the rollout's launch_io does
    assert len(re.findall(r"^static void launch_\w+\(", src, re.M)) == 1
    assert re.search(r"^static void launch_padam\(const TrajAdamArgs& a, int base_identity, hipStream_t st\) \{$", src, re.M)
    assert "const bool fast = scene_is_fast(a.C) || a.w.w_obj == 0.0f;" in src
    # registration: once, under the main unit's ident and hashes (what its SpecEntry carries), with the argument struct's size
    reg = re.findall(r"trk_spec_register_points_adam\(([^;]*)\);", src)
    assert len(reg) == 1 and "trk_spec_register(" not in src and "SpecEntry k" not in src
    args = [a.strip() for a in reg[0].split(",")]
    phash = codegen.points_hash(pt.point_link, pt.point_offset)
    assert args == [f'"{ident}"', f"0x{codegen.model_hash(kin):016x}ull", f"0x{phash:016x}ull", "(uint32_t)sizeof(TrajAdamArgs)", "launch_padam"]
    main = codegen.generate_points_rollout_source(kin, pt, ident)
    entry = [f.strip() for f in re.search(r"static const SpecEntry kEntry = \{(.*)\};", main).group(1).split(",")]
    assert entry[9] == args[0] and entry[1] == args[1] and entry[12] == args[2]


@pytest.mark.parametrize("ident", IDENTS)
def test_kernel_body(ident):
    kin, pt = _unit(ident)
    src = codegen.generate_points_adam_source(kin, pt, ident)
    bodies = re.findall(r"^__global__.*?^\}$", src, re.M | re.S)
    assert len(bodies) == 2
    for body in bodies:
        assert body.count("#pragma nounroll") == 1 and "__syncthreads" not in body and "atomic" not in body
        for absent in ("spec_flush_chunk", "link_pos", "cost_sum", "A.gq", "row[", "return;"):
            assert absent not in body, absent
        assert body.count("trk_dpp_from_next") == 2 and body.count("trk_dpp_from_prev") == 2        # inside the loop over the joints
        # (q, qd, m, v): one load and one store each
        assert body.count("spec_load_q<") == 4 and body.count("spec_store_gq<") == 4
        for arr in ("A.q", "A.qd", "A.adam_m", "A.adam_v"):
            assert len(re.findall(r"spec_load_q<[^>]*>\(static_cast<const float\*>\(" + re.escape(arr) + r"\),", body)) == 1, arr
            assert len(re.findall(r"spec_store_gq<[^>]*>\(" + re.escape(arr) + r",", body)) == 1, arr
        # everything the iteration accumulates is declared inside the loop: it starts from zero every pass
        loop = body[body.index("#pragma nounroll"):]
        head = body[:body.index("#pragma nounroll")]
        for decl in ("float cost = 0.0f;", "float pf0 = 0.0f, pf1 = 0.0f, pf2 = 0.0f, pt0 = 0.0f, pt1 = 0.0f, pt2 = 0.0f;"):
            assert loop.count(decl) == 1 and decl not in head, decl
        lates = re.findall(r"^    float late(\d+) = 0\.0f;$", loop, re.M)
        assert sorted(int(d) for d in lates) == list(range(kin.n_dofs)) and "float late" not in head
        # the walk: every collision column scored once against the scene, every self pair once with its own margin
        groups = [int(n) for n in re.findall(r"spec_objects_cost<(\d+), NoTick, FAST>", body)]
        assert sum(groups) == len(pt.obj_cols) and max(groups) <= codegen.OBJ_GROUP
        assert [int(n) for n in re.findall(r"spec_ws_cost<(\d+)>", body)] == groups
        assert sorted(int(k) for k in re.findall(r"self_margin\)\[(\d+)\]", body)) == list(range(len(pt.self_pairs)))
        assert body.count("ee_cost_eval(") == 1
        # the loop's end: the prior, the update, then the stores after the loop
        assert loop.index("spec_objects_cost<") < loop.index("trk_dpp_from_next") < loop.index("spec_adam_component(") < loop.index("spec_store_gq<")
        assert "if (it == 0) cost0 = fmaf(0.5f, accg, cost);" in loop


def test_the_prior_is_the_arm_kernels_text():
    """one emitter: the lines between the gradient gc[D] and the Adam update are k_traj_adam's, character for character"""
    kin, pt = _unit(IDENTS[0])
    mine = codegen.generate_points_adam_source(kin, pt, IDENTS[0])
    panda = (CSRC / "generated" / "spec_panda.hip").read_text()

    def prior(text):
        a = text.index("    // the prior: e_t = (p_t + dt v_t - p_t+1")
        return text[a:text.index("    if (update) {", a)]
    assert prior(mine) == prior(panda[panda.index("k_traj_adam_bi("):]) and "trk_dpp_from_prev" in prior(mine)


def test_earlier_units_keep_their_text(tmp_path):
    """The committed sha1 goldens, read here: the main attached-point units (spec_points_units_r10.json), the Panda link unit's
    earlier kernels (spec_panda_kernels_r08.json), the shared structs (spec_common_structs_r08.json) -- and spec_units_r14.json, the
    sha1 of every other unit the build list held before this kernel family existed (the other link units, the _via, _vadam and _coll
    satellites), recorded from the generator as it stood then: the emitters this change shares with them must not move a character."""
    want = json.loads((GOLDEN / "spec_points_units_r10.json").read_text())
    assert sorted(want) == sorted(IDENTS)
    for ident in IDENTS:
        kin, pt = _unit(ident)
        assert _sha(codegen.generate_points_rollout_source(kin, pt, ident)) == want[ident], ident
        assert not any("padam" in k for k in codegen._PointsUnit(kin, pt, ident).kernels)
    kin, tmpl = codegen.template_for("panda")
    fresh = codegen.generate_link_kernel_source(kin, tmpl, "panda")
    assert fresh == (CSRC / "generated" / "spec_panda.hip").read_text()
    import test_arm_traj_cpu as arm
    got = {k: [_sha(b) for b in v] for k, v in arm._kernel_blocks(fresh).items()}
    want = json.loads((GOLDEN / "spec_panda_kernels_r08.json").read_text())
    assert {k: got[k] for k in want} == want
    hdr = (CSRC / "trk_spec_common.h").read_text()
    for name, sha in json.loads((GOLDEN / "spec_common_structs_r08.json").read_text()).items():
        m = re.search(r"^struct " + name + r" \{\n.*?^\};", hdr, flags=re.M | re.S)
        assert m and _sha(m.group(0)) == sha, name
    names = codegen.generate_sources(tmp_path)
    earlier = json.loads((GOLDEN / "spec_units_r14.json").read_text())
    assert sorted(earlier) == sorted(set(names) - {"spec_panda.hip"} - {f"spec_{i}{k}.hip" for i in IDENTS for k in ("", "_padam")})
    assert sum(n.endswith("_coll.hip") for n in earlier) == 3 and sum(n.endswith("_via.hip") for n in earlier) == 3
    assert sum(n.endswith("_vadam.hip") for n in earlier) == 3
    for name, sha in earlier.items():
        assert _sha((tmp_path / name).read_text()) == sha, name


def test_the_build_lists_the_units_where_stated(tmp_path):
    """generate_sources, which the Makefile and _lib.build() call, lists the units in link order -- after the _via units, in front of
    the _coll units -- and writes them into the directory itself, like every other unit."""
    srcs = codegen.generate_sources(tmp_path)
    padam = [f"spec_{i}_padam.hip" for i in IDENTS]
    coll = [f"spec_{i}_coll.hip" for i in IDENTS]
    assert srcs[-3:] == coll and srcs[-6:-3] == padam and len(set(srcs)) == len(srcs)
    assert [n for n in srcs if "padam" in n] == padam
    via = [n for n in srcs if n.endswith("_via.hip")]
    vadam = [n for n in srcs if n.endswith("_vadam.hip")]
    assert via and srcs.index(via[-1]) == len(srcs) - 7 and max(srcs.index(n) for n in vadam) < srcs.index(via[0])
    for ident in IDENTS:
        kin, pt = _unit(ident)
        assert (tmp_path / f"spec_{ident}_padam.hip").read_text() == codegen.generate_points_adam_source(kin, pt, ident)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(srcs) and not any(p.is_dir() for p in tmp_path.iterdir())
    # a file is rewritten only when its text changed
    f = tmp_path / srcs[-4]
    before = f.stat().st_mtime_ns
    codegen.generate_sources(tmp_path)
    assert f.stat().st_mtime_ns == before
    # the Makefile builds what generate_sources lists, _lib.build() generates the same, and git keeps the generated units out of history
    mk = (CSRC / "Makefile").read_text()
    assert mk.count("codegen.generate_sources(") == 2 and "$(GEN)" in mk
    assert re.search(r"^generated/%\.o: generated/%\.hip \$\(HDRS\)$", mk, re.M)
    import inspect
    assert "codegen.generate_sources(" in inspect.getsource(_lib.build)
    ignored = (ROOT / ".gitignore").read_text().split("\n")
    assert "torch_robotics_amd/csrc/generated/spec_*.hip" in ignored and "!torch_robotics_amd/csrc/generated/spec_panda.hip" in ignored


def test_units_above_eight_dof_get_none():
    kin, _ = codegen.template_for("dual_panda")
    pt = codegen.PointsTemplate(point_link=np.arange(kin.n_links, dtype=np.int32), point_offset=np.zeros((kin.n_links, 3), np.float32),
                                obj_cols=[1, 2])
    if codegen.points_layout_error(kin, pt.point_link, pt.obj_cols) is None:
        assert kin.n_dofs > 8 and not codegen.points_adam_ok(kin, pt)
        with pytest.raises(AssertionError):
            codegen.generate_points_adam_source(kin, pt, "x")
    kin7, pt7 = _unit(IDENTS[0])
    assert not codegen._PointsUnit(kin7, codegen.link_points_template(kin7, codegen.panda_template(kin7)), "x", link_mode=True).traj_adam_ok


def test_header_exports_library_and_documentation_agree(trk):
    header = (ROOT / "include" / "trk.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(trk_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert NAME in declared and NAME in _lib.EXPORTS and hasattr(trk, NAME) and getattr(trk, NAME).argtypes is not None
    assert f"`{NAME}`" in (ROOT / "INTEGRATION.md").read_text()
    assert re.search(r"#define TRK_ABI_VERSION 5\b", header) and _abi.TRK_ABI_VERSION == 5
    common = (CSRC / "trk_spec_common.h").read_text()
    assert "int trk_spec_register_points_adam(const char* ident, uint64_t model_hash, uint64_t points_hash, uint32_t sizeof_args," in common
    assert "sizeof_args != sizeof(TrajAdamArgs)" in (CSRC / "trk_capi.hip").read_text()


def test_registration_is_refused_on_another_struct_size(trk, capfd):
    """trk_spec_register_points_adam (C++ linkage, like its siblings: the Itanium name of the declaration in trk_spec_common.h) is a size
    check in front of the registry: a unit compiled against another TrajAdamArgs, a null ident or a null launcher is refused and said so"""
    reg = getattr(trk, "_Z29trk_spec_register_points_adamPKcmmjPFvRK12TrajAdamArgsiP12ihipStream_tE")
    reg.argtypes, reg.restype = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p], C.c_int
    fn = C.CFUNCTYPE(None)(lambda: None)                 # never called: nothing is registered under a refused size
    ptr = C.cast(fn, C.c_void_p)
    for size in (0, 8, 1 << 20):
        assert reg(b"no_such_unit", 1, 2, size, ptr) == INVALID, size
    assert reg(None, 1, 2, 0, ptr) == INVALID and reg(b"no_such_unit", 1, 2, 0, None) == INVALID
    assert "another TrajAdamArgs layout" in capfd.readouterr().err


def test_bad_arguments_are_refused_before_any_device_work(trk):
    model = (C.c_char * 8192)()             # stand for TrkModel* / TrkPointSet* / TrkCostModel*: zeroed blocks, never read beyond their headers
    ps = (C.c_char * 8192)()
    cm = (C.c_char * 8192)()
    buf = (C.c_float * 4096)()              # host memory standing for the device buffers, never read
    W, G, A = _abi.RolloutWeights, _abi.GpPrior, _abi.TrajAdam
    w0, g0, a0 = W(1.0, 1.0, 1.0, 0.0), G(0.08, 1.0, 1.0), A(1e-2, 3, 1, 1)

    def err():
        return trk.trk_last_error().decode()

    def steps(m=model, p=ps, c=cm, w=w0, g=g0, a=a0, batch=2, horizon=8, q=buf, qd=buf, am=buf, av=buf):
        ref = lambda s: C.byref(s) if s is not None else None
        return trk.trk_rollout_points_gp_adam_steps(m, p, c, ref(w), ref(g), ref(a), q, qd, am, av, batch, horizon, buf, None)

    assert steps(m=None) == INVALID and err().startswith(NAME + ":") and "null model" in err()
    assert steps(c=None) == INVALID and "null cost model" in err()
    for kw in (dict(w=None), dict(g=None), dict(a=None)):
        assert steps(**kw) == INVALID and "null weights / prior / TrkTrajAdam" in err(), sorted(kw)
    for kw in (dict(q=None), dict(qd=None), dict(am=None), dict(av=None)):
        assert steps(**kw) == INVALID and "null q / qd / adam_m / adam_v" in err(), sorted(kw)
    assert steps(batch=-1) == INVALID and "bad batch/horizon" in err()
    for h in (0, -1):
        assert steps(horizon=h) == INVALID and "bad batch/horizon" in err(), h
    for bad in (G(0.0, 1.0, 1.0), G(-0.1, 1.0, 1.0), G(NAN, 1.0, 1.0), G(INF, 1.0, 1.0), G(0.08, 0.0, 1.0), G(0.08, -1.0, 1.0),
                G(0.08, NAN, 1.0), G(0.08, INF, 1.0), G(0.08, 1.0, NAN), G(0.08, 1.0, INF)):
        assert steps(g=bad) == INVALID, (bad.dt, bad.sigma, bad.weight)
    for k in range(4):
        for v in (NAN, INF, -INF):
            vals = [1.0, 1.0, 1.0, 0.0]
            vals[k] = v
            assert steps(w=W(*vals)) == INVALID, vals
    for bad in (A(1e-2, 3, 1, -1), A(1e-2, 3, 0, 1), A(1e-2, 3, -4, 1), A(NAN, 3, 1, 1), A(INF, 3, 1, 1), A(1e-2, 16, 1, 1), A(1e-2, -1, 1, 1)):
        assert steps(a=bad) == INVALID, (bad.lr, bad.pin, bad.first_step, bad.n_steps)
    # a wavefront owns whole trajectories: the horizon is a power of two up to 64; the refusal names the route for the others -- and
    # comes before the point set is looked at
    for h in (3, 48, 65, 128):
        for p in (ps, None):
            assert steps(horizon=h, p=p) == UNSUPPORTED, h
            assert "power of two" in err() and "64" in err() and "trk_rollout_points_cost_grad" in err() and "trk_gp_prior" in err(), err()
    # sound arguments get as far as the point set: none, or the zeroed block -- a point set of no model
    for h in (1, 2, 8, 64):
        assert steps(horizon=h, p=None) == INVALID and "null point set" in err(), h
        assert steps(horizon=h) == INVALID and "belongs to no model" in err(), h
    # an empty batch needs no buffers, but still a sound point set
    assert steps(batch=0, q=None, qd=None, am=None, av=None) == INVALID and "belongs to no model" in err()


@pytest.fixture(scope="module")
def padam_isa(tmp_path_factory):
    d = tmp_path_factory.mktemp("padam_isa")
    meta = {}
    for ident in IDENTS:
        kin, pt = _unit(ident)
        src = d / f"spec_{ident}_padam.hip"
        src.write_text(codegen.generate_points_adam_source(kin, pt, ident))
        asm = isa._device_asm(src, d / f"spec_{ident}_padam.s")
        for n, body in isa._kernels(asm).items():
            blk = re.search(r"\.amdhsa_kernel\s+" + re.escape(n) + r"\n(.*?)\.end_amdhsa_kernel", asm, flags=re.S).group(1)
            meta[n] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(private_segment_fixed_size|next_free_vgpr|accum_offset)\s+(\d+)", blk)}
            meta[n]["barriers"] = sum("s_barrier" in l for l in body)
    return meta


def test_isa_no_scratch_and_the_stated_occupancy(padam_isa):
    """Scratch 0 is the condition.  The occupancy is what the compiler reports for these kernels (POINTS_ADAM_OCCUPANCY = 1: the walk's
    registers + 5 D of state need more than the 256 of two wavefronts per SIMD -- with that bound stated every instantiation but two
    spills 44 - 276 bytes per lane; within 512 none does)."""
    assert len(padam_isa) == 12 and all("k_padam_b" in n for n in padam_isa), sorted(padam_isa)          # 3 units x 2 bases x FAST
    for n, m in sorted(padam_isa.items()):
        vgprs = m["next_free_vgpr"]
        print(f"{n}: private segment {m['private_segment_fixed_size']} B, {vgprs} VGPRs (incl. AGPRs) -> {512 // (-(-vgprs // 8) * 8)} wavefronts per SIMD, "
              f"{m['barriers']} barriers")
        assert m["private_segment_fixed_size"] == 0, n
        # gfx950: 512 registers per lane and SIMD, allocated in blocks of 8
        assert 512 // (-(-vgprs // 8) * 8) >= codegen.POINTS_ADAM_OCCUPANCY, (n, vgprs)
        assert m["barriers"] == 0, n


def _robot(name):
    box = lambda: tra.GraspedObjectPandaBox(tensor_args=CPU)
    return {"spheres": lambda: tra.RobotPanda(link_sphere_model="panda", tensor_args=CPU),
            "grasp": lambda: tra.RobotPanda(grasped_object=box(), tensor_args=CPU),
            "both": lambda: tra.RobotPanda(link_sphere_model="panda", grasped_object=box(), tensor_args=CPU)}[name]()


def test_the_task_hands_each_plan_out_only_where_it_holds():
    q7 = torch.zeros(2, 8, 7)
    links = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=CPU), robot=tra.RobotPanda(tensor_args=CPU), tensor_args=CPU)
    with pytest.raises(NotImplementedError, match="rollout_adam_plan"):
        links.points_adam_plan(q7, q7.clone(), 0.1, 1.0)
    mass = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=CPU), robot=tra.RobotPointMass3D(tensor_args=CPU), tensor_args=CPU)
    q3 = torch.zeros(2, 8, 3)
    with pytest.raises(NotImplementedError, match="rollout_adam_plan"):
        mass.points_adam_plan(q3, q3.clone(), 0.1, 1.0)
    grasp = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=CPU), robot=_robot("grasp"), tensor_args=CPU)
    with pytest.raises(NotImplementedError, match="link-column.*points_adam_plan"):
        grasp.rollout_adam_plan(q7, q7.clone(), 0.1, 1.0)
    for H in (3, 48, 65, 128):
        t = torch.zeros(2, H, 7)
        with pytest.raises(NotImplementedError, match="power of two"):
            grasp.points_adam_plan(t, t.clone(), 0.1, 1.0)


@pytest.mark.parametrize("name", ["spheres", "grasp", "both"])
def test_the_gpu_tests_inputs_reach_both_sides_of_the_object_hinge(oracle_lib, name):
    """The fp64 oracle alone, on the union of the seven shapes' walks (seeds 1000 B + H) of tests/test_gpu_points_adam.py with
    obstacle_cutoff_margin = 0.05 and clamp_sdf = True: the object hinge is active on at least 20 % and inactive on at least 10 % of
    the samples for every model on EnvSpheres3D and on EnvTableShelf (measured: active 0.77 / 0.86 / 0.79 and 0.23 / 0.27 / 0.25).
    The workspace hinge is active on about a fifth of the samples on the spheres scene and about none on the shelf, the self pairs on
    0 - 1.2 %: their gradient is covered by the clamp_sdf = False cases, where no term is ever zero."""
    from test_gpu_arm_traj import SHAPES, dof_limits, walks
    robot = _robot(name)
    kin = robot.diff_panda._kin
    kin.lower_dof, kin.upper_dof = dof_limits(kin)
    q = np.concatenate([walks(kin, B, H, 1000 * B + H)[0].reshape(-1, kin.n_dofs) for B, H in SHAPES]).astype(np.float64)
    assert [tuple(s) for s in SHAPES] == [(1, 64), (3, 64), (5, 64), (9, 32), (8, 8), (7, 2), (130, 1)] and len(q) == 1072
    pl, po = robot.collision_point_set()
    for env in (tra.EnvSpheres3D, tra.EnvTableShelf):
        task = tra.PlanningTask(env=env(tensor_args=CPU), robot=robot, obstacle_cutoff_margin=0.05, clamp_sdf=True, tensor_args=CPU)
        orc = oracle_lib.Oracle(kin, task.build_cost_spec())
        share = {k: float((orc.rollout_points(pl, po, q, w, "f64")[1] > 0.0).mean())
                 for k, w in (("self", (1, 0, 0, 0)), ("obj", (0, 1, 0, 0)), ("ws", (0, 0, 1, 0)))}
        print(f"{name} on {env.__name__}: active share of the samples: {share}")
        assert share["obj"] >= 0.20 and 1.0 - share["obj"] >= 0.10, (name, env.__name__, share)
