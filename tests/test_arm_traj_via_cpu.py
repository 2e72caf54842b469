"""CPU-only checks of the arm's planning loop with the via-point term (trk_rollout_gp_via_adam_steps, generated kernels
k_traj_via_adam_bi / k_traj_via_adam_bg<BOX>): header, EXPORTS, library and documents agree and the ctypes struct has the header's
layout; bad arguments are refused before any device work (model and cost model are blocks of zeros that are never dereferenced beyond
their headers); the generator writes a unit of its own for the small arms only, generate_sources lists it in front of the via-point cost
units, and the Panda's main and via-point cost units keep their text; the kernel body has one run-time loop over the via points
inside the iteration loop, no barrier, one load and one store of each state array and the interpolation rounded operation by
operation; the four compiled Panda instantiations use no scratch, fit the occupancy the generator states, have no barrier and no
atomics and exchange by DPP; the task hands the plan out only where it holds."""
import ctypes as C
import hashlib
import re
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

import torch_robotics_amd as tra
from torch_robotics_amd import _abi, _lib, codegen
import test_isa_entry_chain_cpu as isa

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "torch_robotics_amd" / "csrc"
CPU = dict(device=torch.device("cpu"), dtype=torch.float32)
NAME = "trk_rollout_gp_via_adam_steps"
OK, INVALID, UNSUPPORTED = _abi.TRK_OK, _abi.TRK_ERR_INVALID_ARG, _abi.TRK_ERR_UNSUPPORTED
NAN, INF = float("nan"), float("inf")
SMALL_ARMS = ["panda", "iiwa7", "ur10"]
# sha1 of spec_panda_via.hip as the generator wrote it before this kernel family existed
PANDA_VIA_UNIT_SHA1 = "375d36d60ee865a692f3f258554fe7fb98fd1c4f"


@pytest.fixture(scope="module")
def trk():
    if not _lib.LIB_PATH.exists():
        _lib.build()
    return _lib.lib()


def test_header_exports_library_and_documentation_agree(trk):
    header = (ROOT / "include" / "trk.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(trk_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert NAME in declared and NAME in _lib.EXPORTS and hasattr(trk, NAME)
    assert getattr(trk, NAME).argtypes is not None and len(getattr(trk, NAME).argtypes) == 14
    assert f"`{NAME}`" in (ROOT / "INTEGRATION.md").read_text()
    assert re.search(r"TRK_DISPATCH_GENERATED_VIA_ADAM = (\d+)", header).group(1) == "5"
    from torch_robotics_amd import ops
    assert 5 in ops.DISPATCH_NAMES and len(ops.DISPATCH_NAMES) == 6


def test_struct_layout_and_dispatch_constant_match_header():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "trk.h"\nint main(){printf("%zu %zu %zu %zu %zu %d\\n",sizeof(TrkTrajVia),' \
          'offsetof(TrkTrajVia,w_via),offsetof(TrkTrajVia,n_interp),offsetof(TrkTrajVia,alpha),offsetof(TrkTrajVia,beta),' \
          '(int)TRK_DISPATCH_GENERATED_VIA_ADAM);}'
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")], check=True)
        out = [int(v) for v in subprocess.run([str(Path(d) / "s")], capture_output=True, text=True, check=True).stdout.split()]
    T = _abi.TrajVia
    assert out == [C.sizeof(T), T.w_via.offset, T.n_interp.offset, T.alpha.offset, T.beta.offset, 5]


def test_bad_arguments_are_refused_before_any_device_work(trk):
    model = (C.c_char * 8192)()             # stand for TrkModel* / TrkCostModel*: zeroed headers (0 links, 0 DOF), nothing behind them is read
    cm = (C.c_char * 8192)()
    buf = (C.c_float * 4096)()              # host memory standing for the device buffers, never read
    p = C.addressof(buf)
    W, G, V, A = _abi.RolloutWeights, _abi.GpPrior, _abi.TrajVia, _abi.TrajAdam
    w0, g0, v0, a0 = W(1.0, 1.0, 1.0, 0.0), G(0.08, 1.0, 1.0), V(0.2, 5, p, p), A(1e-2, 3, 1, 1)

    def steps(m=model, c=cm, w=w0, g=g0, v=v0, a=a0, batch=2, horizon=8, q=buf, qd=buf, am=buf, av=buf):
        ref = lambda s: C.byref(s) if s is not None else None
        return trk.trk_rollout_gp_via_adam_steps(m, c, ref(w), ref(g), ref(v), ref(a), q, qd, am, av, batch, horizon, buf, None)

    def err():
        return trk.trk_last_error().decode()

    for kw in ("m", "c", "w", "g", "v", "a", "q", "qd", "am", "av"):
        assert steps(**{kw: None}) == INVALID, kw
        assert err().startswith(NAME + ":"), err()
    assert steps(v=V(0.2, 5, None, p)) == INVALID and "alpha" in err()
    assert steps(v=V(0.2, 5, p, None)) == INVALID and "beta" in err()
    for n in (0, -1):
        assert steps(v=V(0.2, n, p, p)) == INVALID and "n_interp" in err(), n
    for wv in (NAN, INF, -INF):
        assert steps(v=V(wv, 5, p, p)) == INVALID and "w_via" in err(), wv
    assert steps(batch=-1) == INVALID
    for h in (0, -1):
        assert steps(horizon=h) == INVALID, h
    # everything trk_rollout_gp_adam_steps checks
    for bad in (G(0.0, 1.0, 1.0), G(NAN, 1.0, 1.0), G(0.08, 0.0, 1.0), G(0.08, INF, 1.0), G(0.08, 1.0, NAN)):
        assert steps(g=bad) == INVALID, (bad.dt, bad.sigma, bad.weight)
    for k in range(4):
        vals = [1.0, 1.0, 1.0, 0.0]
        vals[k] = NAN
        assert steps(w=W(*vals)) == INVALID, vals
    for bad in (A(1e-2, 3, 1, -1), A(1e-2, 3, 0, 1), A(NAN, 3, 1, 1), A(1e-2, 16, 1, 1), A(1e-2, -1, 1, 1)):
        assert steps(a=bad) == INVALID, (bad.lr, bad.pin, bad.first_step, bad.n_steps)
    # a wavefront owns whole trajectories: the horizon is a power of two up to 64, and the message says so
    for h in (3, 48, 65, 128):
        assert steps(horizon=h) == UNSUPPORTED, h
        assert "power of two" in err() and "64" in err(), err()
    assert steps(batch=0, horizon=64) == OK and steps(batch=0, horizon=64, q=None, qd=None, am=None, av=None) == OK
    # sound arguments get past the validation: the zeroed model has no joints, so there is nothing to launch
    assert steps(horizon=1) == OK and steps(v=V(0.0, 1, p, p), horizon=64) == OK


def _vadam_text(ident):
    kin, tmpl = codegen.template_for(ident)
    return kin, tmpl, codegen.generate_via_adam_source(kin, tmpl, ident)


def test_generate_sources_lists_the_units_of_the_small_arms_in_front_of_the_via_units(tmp_path):
    names = codegen.generate_sources(tmp_path)
    vadam = [n for n in names if n.endswith("_vadam.hip")]
    assert vadam == [f"spec_{i}_vadam.hip" for i in SMALL_ARMS]
    for ident in ("dual_panda", "ur10_allegro"):
        assert f"spec_{ident}_vadam.hip" not in names and not (tmp_path / f"spec_{ident}_vadam.hip").exists(), ident
    assert len(set(names)) == len(names)
    via = [n for n in names if n.endswith("_via.hip")]
    first_main = [f"spec_{i}.hip" for i in list(codegen.SPEC_ROBOTS) + list(codegen.SPEC_POINT_ROBOTS)]
    # after the main units, contiguous, in front of the first via unit; the via units contiguous, then the attached-point units'
    # planning loops, the three _coll units last
    padam = [f"spec_{i}_padam.hip" for i in codegen.SPEC_POINT_ROBOTS]
    assert names == first_main + vadam + via + padam + [f"spec_{i}_coll.hip" for i in codegen.SPEC_POINT_ROBOTS]
    for ident in codegen.SPEC_ROBOTS:
        kin, tmpl = codegen.template_for(ident)
        assert codegen.via_adam_ok(kin, tmpl, ident) == (f"spec_{ident}_vadam.hip" in vadam), ident
        if codegen.via_adam_ok(kin, tmpl, ident):
            assert "k_traj_adam_bi" in (tmp_path / f"spec_{ident}.hip").read_text() and kin.n_dofs <= 8      # the units that carry k_traj_adam
            assert (tmp_path / f"spec_{ident}_vadam.hip").read_text() == codegen.generate_via_adam_source(kin, tmpl, ident)
    # the headline unit and its via-point cost unit keep their text, byte for byte
    assert (tmp_path / "spec_panda.hip").read_text() == (CSRC / "generated" / "spec_panda.hip").read_text()
    assert hashlib.sha1((tmp_path / "spec_panda_via.hip").read_bytes()).hexdigest() == PANDA_VIA_UNIT_SHA1
    assert (tmp_path / "spec_panda_via.hip").read_text().count("__global__") == 2


@pytest.mark.parametrize("ident", SMALL_ARMS)
def test_unit_defines_starts_and_registers_its_kernels(ident):
    kin, tmpl, src = _vadam_text(ident)
    defined = re.findall(r"^__global__ void __launch_bounds__\(SPEC_BLOCK\) (k_\w+)\(TrajViaAdamArgs A\) \{", src, re.M)
    assert sorted(defined) == ["k_traj_via_adam_bg", "k_traj_via_adam_bi"] and src.count("__global__") == 2       # the block size alone
    assert sorted(set(re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", src))) == ["k_traj_via_adam_bg", "k_traj_via_adam_bi"]
    assert codegen.via_adam_kernels(ident) == [f"spec_{ident}::k_traj_via_adam_{b}<{v}>" for b in ("bi", "bg") for v in ("false", "true")]
    assert f"namespace spec_{ident} {{" in src and f"constexpr int L = {kin.n_links}, D = {kin.n_dofs}," in src
    assert src.split("\n")[1] == "#pragma clang fp reassociate(on) contract(fast) reciprocal(on)"                # the FP line of the via unit
    reg = re.findall(r"trk_spec_register_via_adam\(([^;]*)\);", src)
    assert len(reg) == 1 and "trk_spec_register(" not in src and "SpecEntry k" not in src
    assert [a.strip() for a in reg[0].split(",")] == [f'"{ident}"', f"0x{codegen.model_hash(kin):016x}ull",
                                                      f"0x{codegen.template_identity(tmpl):016x}ull",
                                                      "(uint32_t)sizeof(TrajViaAdamArgs)", "launch_via_adam"]
    for body in re.findall(r"^__global__.*?^\}$", src, re.M | re.S):
        assert "__syncthreads" not in body and "s_barrier" not in body and "atomic" not in body.lower()
        # one run-time loop over the via points (the way point is its pass -1) inside the run-time iteration loop
        assert body.count("#pragma nounroll") == 2
        it, via = body.index("for (int it = 0; it < A.n_steps; ++it) {"), body.index("for (int a = -1; a < A.n_via; ++a) {")
        assert it < via and body.count("for (int a = ") == 1 and body.count("trk_sincos") == body[via:].count("trk_sincos") > 0   # the body once
        assert "link_pos" not in body and "PosFlusher" not in body and "NoFlush flush" in body            # no position stores
        # q, qd, m, v: one load and one store each
        assert body.count("spec_load_q<D>") == 2 and body.count("spec_load_q<2 * D>") == 2
        assert body.count("spec_store_gq<D>") == 2 and body.count("spec_store_gq<2 * D>") == 2
        for arr in ("A.q)", "A.qd)", "A.adam_m)", "A.adam_v)"):
            assert body.count("static_cast<const float*>(" + arr) == 1, arr
        for arr in ("A.q,", "A.qd,", "A.adam_m,", "A.adam_v,"):
            assert body.count("(" + arr) == 1, arr
        # the way point by a select, the via points with each product and the sum rounded once
        assert "q[d] = way ? x[d] : __fadd_rn(__fmul_rn(x[d], fa), __fmul_rn(xn[d], fb));" in body
        assert body.count("trk_dpp_from_next") == 2 and body.count("trk_dpp_from_prev") == 3               # each inside a loop over the joints
        assert "spec_adam_component" in body


@pytest.fixture(scope="module")
def panda_isa(tmp_path_factory):
    d = tmp_path_factory.mktemp("vadam_isa")
    src = d / "spec_panda_vadam.hip"
    src.write_text(_vadam_text("panda")[2])
    asm = isa._device_asm(src, d / "spec_panda_vadam.s")
    kernels = isa._kernels(asm)
    meta = {}
    for n in kernels:
        blk = re.search(r"\.amdhsa_kernel\s+" + re.escape(n) + r"\n(.*?)\.end_amdhsa_kernel", asm, flags=re.S).group(1)
        meta[n] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(private_segment_fixed_size|next_free_vgpr|accum_offset|group_segment_fixed_size)\s+(\d+)", blk)}
    return kernels, meta


def test_isa_of_the_four_panda_instantiations(panda_isa):
    kernels, meta = panda_isa
    assert len(kernels) == 4 and all("k_traj_via_adam_b" in n for n in kernels), sorted(kernels)             # bi / bg x BOX
    for n, m in sorted(meta.items()):
        vgprs = m["next_free_vgpr"]
        print(f"{n}: private segment {m['private_segment_fixed_size']} B, {vgprs} VGPRs (incl. AGPRs), LDS {m['group_segment_fixed_size']} B "
              f"-> {512 // (-(-vgprs // 8) * 8)} wavefronts per SIMD")
        assert m["private_segment_fixed_size"] == 0, n
        # gfx950: 512 registers per lane and SIMD, allocated in blocks of 8
        assert 512 // (-(-vgprs // 8) * 8) >= codegen.TRAJ_VIA_ADAM_OCCUPANCY, (n, vgprs)
        body = kernels[n]
        assert all("s_barrier" not in l for l in body), n
        assert all("s_swappc_b64" not in l for l in body), n
        assert all("scratch_" not in l.split(";")[0] for l in body), n
        assert not any(re.match(r"^\s*(global_atomic|flat_atomic|buffer_atomic|ds_add|ds_cmpst)", l) for l in body), n
        # per joint: q and qd from the next lane; the via share and the prior's two factors to the next lane
        shl, shr = [l for l in body if "wave_shl:1" in l], [l for l in body if "wave_shr:1" in l]
        print(f"{n}: {len(shl)} DPP operands from the next lane, {len(shr)} to the next lane")
        assert len(shl) >= 7 and len(shr) >= 7, (n, len(shl), len(shr))              # at least one per joint each way


def test_the_task_hands_the_plan_out_only_where_it_holds():
    """with the via keywords the refusals are the plain plan's"""
    q = torch.zeros(2, 8, 2)
    planar = tra.PlanningTask(env=tra.EnvNarrowPassageDense2D(tensor_args=CPU), robot=tra.RobotPointMass(tensor_args=CPU), tensor_args=CPU)
    with pytest.raises(NotImplementedError, match="kinematic tree"):
        planar.rollout_adam_plan(q, q.clone(), 0.1, 1.0, w_via=0.2, num_interpolation=5)
    grasp = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=CPU),
                             robot=tra.RobotPanda(grasped_object=tra.GraspedObjectPandaBox(tensor_args=CPU), tensor_args=CPU), tensor_args=CPU)
    q7 = torch.zeros(2, 8, 7)
    with pytest.raises(NotImplementedError, match="link-column"):
        grasp.rollout_adam_plan(q7, q7.clone(), 0.1, 1.0, w_via=0.2, num_interpolation=5)
    import inspect
    from torch_robotics_amd import ops
    sig = inspect.signature(ops.ArmAdamPlan.__init__).parameters
    assert sig["w_via"].default == 0.0 and sig["num_interpolation"].default == 0
    with pytest.raises(ValueError, match="same GPU|GPU"):
        ops.ArmAdamPlan(None, None, (1, 1, 1, 0), q7, q7.clone(), 0.1, 1.0, w_via=0.2, num_interpolation=5)


from test_satellite_units_cpu import rec          # noqa: E402,F401  (the recorder in place of compiler and dlopen)


def test_run_time_units_get_their_kernels_on_the_first_request(rec):          # noqa: F811
    """jit.specialize only notes that a qualifying run-time unit may get a spec_<ident>_vadam unit (told by the requests it makes:
    tests/test_satellite_units_cpu.py has every other case); ArmAdamPlan asks for it when it binds the term.  A robot served by the
    bundled units has nothing to compile."""
    import inspect
    from test_satellite_units_cpu import first_request_of_the_iiwa7_unit
    from torch_robotics_amd import jit, ops
    first_request_of_the_iiwa7_unit(rec)
    bind = inspect.getsource(ops.ArmAdamPlan._bind)
    assert bind.index("if via:") < bind.index('jit.load_satellite_units(self.model.kin, "vadam")') < bind.index("else:")
    kin, _ = codegen.template_for("panda")
    assert jit.load_satellite_units(kin, "vadam") == [] and len(rec.requests) == 3
