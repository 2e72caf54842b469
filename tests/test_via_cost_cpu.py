"""CPU-only checks of the fused via-point cost (trk_rollout_via_cost_grad, generated kernels k_via_cost_bi / k_via_cost_bg<BOX>): header,
EXPORTS, library and INTEGRATION.md agree; bad arguments of every kind are refused before any device work (model and cost model are
blocks of zeros that are never dereferenced beyond their headers); the generator writes a unit of its own for the small arms only,
generate_sources lists it in front of the attached-point units' satellite units, and the main Panda unit keeps its text; the kernel body
has no barrier, a run-time loop and one DPP exchange per joint in each direction; the compiled Panda unit uses no scratch, fits the
occupancy the generator states and has no s_barrier; the task method takes its two-step route where the kernel does not serve."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import torch_robotics_amd as tra
from torch_robotics_amd import _abi, _lib, codegen
import test_isa_entry_chain_cpu as isa

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "torch_robotics_amd" / "csrc"
CPU = dict(device=torch.device("cpu"), dtype=torch.float32)
NAME = "trk_rollout_via_cost_grad"
OK, INVALID, UNSUPPORTED = _abi.TRK_OK, _abi.TRK_ERR_INVALID_ARG, _abi.TRK_ERR_UNSUPPORTED
NAN, INF = float("nan"), float("inf")
SMALL_ARMS = ["panda", "iiwa7", "ur10"]


@pytest.fixture(scope="module")
def trk():
    if not _lib.LIB_PATH.exists():
        _lib.build()
    return _lib.lib()


def test_header_exports_library_and_documentation_agree(trk):
    header = (ROOT / "include" / "trk.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(trk_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert NAME in declared and NAME in _lib.EXPORTS and hasattr(trk, NAME)
    assert getattr(trk, NAME).argtypes is not None and len(getattr(trk, NAME).argtypes) == 13
    assert f"`{NAME}`" in (ROOT / "INTEGRATION.md").read_text()
    assert re.search(r"#define TRK_VIA_COST_MAX_HORIZON (\d+)", header).group(1) == str(_abi.TRK_VIA_COST_MAX_HORIZON) == "64"


def test_bad_arguments_are_refused_before_any_device_work(trk):
    model = (C.c_char * 8192)()             # stand for TrkModel* / TrkCostModel*: zeroed headers (0 links, 0 DOF), nothing behind them is read
    cm = (C.c_char * 8192)()
    buf = (C.c_float * 4096)()              # host memory standing for the device buffers, never read
    W = _abi.RolloutWeights
    w0 = W(1.0, 1.0, 1.0, 0.0)

    def via(m=model, c=cm, w=w0, x=buf, T=2, H=8, n=5, alpha=buf, beta=buf, seed=None, cost=None, gq=buf):
        return trk.trk_rollout_via_cost_grad(m, c, C.byref(w) if w is not None else None, x, T, H, n, alpha, beta, seed, cost, gq, None)

    def err():
        return trk.trk_last_error().decode()

    assert via(m=None) == INVALID and err().startswith(NAME + ":") and "null model" in err()
    assert via(c=None) == INVALID and "null cost model" in err()
    assert via(w=None) == INVALID and "null weights" in err()
    assert via(x=None) == INVALID and via(gq=None) == INVALID and "null x / gq" in err()
    assert via(alpha=None) == INVALID and via(beta=None) == INVALID and "alpha / beta" in err()
    assert via(T=-1) == INVALID
    for h in (0, 1, -1):
        assert via(H=h) == INVALID, h
    for n in (0, -1):
        assert via(n=n) == INVALID and "n_interp" in err(), n
    for k in range(4):
        for v in (NAN, INF, -INF):
            vals = [1.0, 1.0, 1.0, 0.0]
            vals[k] = v
            assert via(w=W(*vals)) == INVALID and "finite" in err(), vals
    # a wavefront owns whole trajectories: the horizon is at most 64, and the message says so
    for h in (65, 128):
        assert via(H=h) == UNSUPPORTED, h
        assert "64" in err() and "horizon" in err(), err()
    # the nullable buffers are nullable, an empty batch needs no launch (and no x / gq)
    assert via(T=0, H=64) == OK and via(T=0, H=64, x=None, gq=None, seed=buf, cost=buf) == OK
    # sound arguments get past the validation: the zeroed model has no joints, so there is nothing to launch
    assert via(H=2, n=1) == OK and via(H=64, seed=buf, cost=buf) == OK


def _via_text(ident):
    kin, tmpl = codegen.template_for(ident)
    return kin, tmpl, codegen.generate_via_cost_source(kin, tmpl, ident)


def test_generate_sources_lists_the_via_units_of_the_small_arms(tmp_path):
    names = codegen.generate_sources(tmp_path)
    via = [n for n in names if n.endswith("_via.hip")]
    for ident in SMALL_ARMS:
        assert f"spec_{ident}_via.hip" in via, ident
    for ident in ("dual_panda", "ur10_allegro"):
        assert f"spec_{ident}_via.hip" not in names and not (tmp_path / f"spec_{ident}_via.hip").exists(), ident
    assert len(set(names)) == len(names)
    # after every main unit, in front of the attached-point units' planning loops and boolean kernels (which stay the last three names)
    first, last = names.index(via[0]), names.index(via[-1])
    assert last - first == len(via) - 1 and names[-3:] == [f"spec_{i}_coll.hip" for i in codegen.SPEC_POINT_ROBOTS]
    assert names[last + 1:-3] and all(n.endswith("_padam.hip") for n in names[last + 1:-3])
    assert all(not n.endswith(("_via.hip", "_padam.hip", "_coll.hip")) for n in names[:first])
    for n in via:
        ident = n[len("spec_"):-len("_via.hip")]
        kin, tmpl, text = _via_text(ident)
        assert (tmp_path / n).read_text() == text, ident
        assert codegen.via_cost_ok(kin, tmpl, ident) and kin.n_dofs <= 8
    for ident in codegen.SPEC_ROBOTS:
        kin, tmpl = codegen.template_for(ident)
        assert codegen.via_cost_ok(kin, tmpl, ident) == (f"spec_{ident}_via.hip" in via), ident
    # the headline unit keeps its committed text, byte for byte
    assert (tmp_path / "spec_panda.hip").read_text() == (CSRC / "generated" / "spec_panda.hip").read_text()


@pytest.mark.parametrize("ident", SMALL_ARMS)
def test_unit_defines_starts_and_registers_its_kernels(ident):
    kin, tmpl, src = _via_text(ident)
    D = kin.n_dofs
    defined = re.findall(r"^__global__ void __launch_bounds__\(SPEC_BLOCK\) (k_\w+)\(ViaCostArgs A\) \{", src, re.M)
    assert sorted(defined) == ["k_via_cost_bg", "k_via_cost_bi"] and src.count("__global__") == 2
    assert sorted(set(re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", src))) == ["k_via_cost_bg", "k_via_cost_bi"]
    assert codegen.via_cost_kernels(ident) == [f"spec_{ident}::k_via_cost_{b}<{v}>" for b in ("bi", "bg") for v in ("false", "true")]
    assert f"namespace spec_{ident} {{" in src and f"constexpr int L = {kin.n_links}, D = {D}," in src
    reg = re.findall(r"trk_spec_register_via_cost\(([^;]*)\);", src)
    assert len(reg) == 1 and "trk_spec_register(" not in src and "SpecEntry k" not in src
    args = [a.strip() for a in reg[0].split(",")]
    assert args == [f'"{ident}"', f"0x{codegen.model_hash(kin):016x}ull", f"0x{codegen.template_identity(tmpl):016x}ull",
                    "(uint32_t)sizeof(ViaCostArgs)", "launch_via_cost"]
    # the identity tells two templates of one robot apart
    other = codegen.CollisionTemplate(obj_links=list(tmpl.obj_links)[:-1], self_pairs=list(tmpl.self_pairs), ee_link=tmpl.ee_link)
    assert codegen.template_identity(other) != codegen.template_identity(tmpl)
    for body in re.findall(r"^__global__.*?^\}$", src, re.M | re.S):
        assert "__syncthreads" not in body and "s_barrier" not in body and "atomic" not in body.lower()
        assert body.count("#pragma nounroll") == 1 and "for (int a = 0; a < A.n; ++a)" in body
        assert body.count("trk_dpp_from_next") == 1 and body.count("trk_dpp_from_prev") == 1         # each inside a loop over the D joints
        for needle, loop in (("trk_dpp_from_next", "xn[d] ="), ("trk_dpp_from_prev", "gv[d] =")):
            line = next(l for l in body.split("\n") if needle in l)
            assert loop in line
        assert "link_pos" not in body and "PosFlusher" not in body and "NoFlush flush" in body            # no position stores
        assert body.count("spec_load_q<D>") == 1 and body.count("spec_store_gq<D>") == 1                  # x read once, gq written once
        assert "__fadd_rn(__fmul_rn(x[d], fa), __fmul_rn(xn[d], fb))" in body                            # each product and the sum rounded once
        assert body.count("store_wt_f1(A.cost + seg + a, cost)") == 1


@pytest.fixture(scope="module")
def via_isa(tmp_path_factory):
    d = tmp_path_factory.mktemp("via_isa")
    src = d / "spec_panda_via.hip"
    src.write_text(_via_text("panda")[2])
    asm = isa._device_asm(src, d / "spec_panda_via.s")
    kernels = isa._kernels(asm)
    meta = {}
    for n in kernels:
        blk = re.search(r"\.amdhsa_kernel\s+" + re.escape(n) + r"\n(.*?)\.end_amdhsa_kernel", asm, flags=re.S).group(1)
        meta[n] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(private_segment_fixed_size|next_free_vgpr|accum_offset)\s+(\d+)", blk)}
    return kernels, meta


def test_isa_no_scratch_the_stated_occupancy_and_no_barrier(via_isa):
    kernels, meta = via_isa
    assert len(kernels) == 4 and all("k_via_cost_b" in n for n in kernels), sorted(kernels)             # bi / bg x BOX
    for n, m in sorted(meta.items()):
        vgprs = m["next_free_vgpr"]
        print(f"{n}: private segment {m['private_segment_fixed_size']} B, {vgprs} VGPRs (incl. AGPRs) -> {512 // (-(-vgprs // 8) * 8)} wavefronts per SIMD")
        assert m["private_segment_fixed_size"] == 0, n
        # gfx950: 512 registers per lane and SIMD, allocated in blocks of 8
        assert 512 // (-(-vgprs // 8) * 8) >= codegen.VIA_COST_OCCUPANCY, (n, vgprs)
        body = kernels[n]
        assert all("s_barrier" not in l for l in body), n
        assert all("s_swappc_b64" not in l for l in body), n
        dpps = [l for l in body if "dpp" in l or "wave_sh" in l]
        assert len(dpps) >= 2 * 7, (n, len(dpps))                       # x from the next lane, the gradient's share to the next, per joint
        assert not any(re.match(r"^\s*(global_atomic|flat_atomic|buffer_atomic|ds_add|ds_cmpst)", l) for l in body), n


def test_the_task_method_takes_the_two_step_route_where_the_kernel_does_not_serve():
    """A grasped-box Panda (attached points) and the 2-D point mass have no via-point cost kernel: the method does not refuse them.  On
    host tensors the call is a round trip through the GPU; without one it runs up to the first device operation, which says so."""
    grasp = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=CPU),
                             robot=tra.RobotPanda(grasped_object=tra.GraspedObjectPandaBox(tensor_args=CPU), tensor_args=CPU), tensor_args=CPU)
    planar = tra.PlanningTask(env=tra.EnvNarrowPassageDense2D(tensor_args=CPU), robot=tra.RobotPointMass(tensor_args=CPU), tensor_args=CPU)
    for task, q, n in ((grasp, torch.zeros(2, 8, 7), 5), (grasp, torch.zeros(2, 8, 14), 5), (grasp, torch.zeros(2, 70, 7), 2),
                       (planar, torch.zeros(2, 8, 2), 3)):
        q.requires_grad_(True)
        if torch.cuda.is_available():
            cost = task.compute_collision_cost_via(q, num_interpolation=n)
            assert tuple(cost.shape) == (2, (q.shape[1] - 1) * n) and cost.requires_grad
        else:
            with pytest.raises((_lib.TrkError, RuntimeError), match="no CPU path|no HIP device"):
                task.compute_collision_cost_via(q, num_interpolation=n)
    with pytest.raises(ValueError, match="two way points"):
        grasp.compute_collision_cost_via(torch.zeros(2, 1, 7))
    with pytest.raises(TypeError, match="unexpected keyword"):
        grasp.compute_collision_cost_via(torch.zeros(2, 8, 7), w_gp=1.0)
    with pytest.raises(ValueError, match="trajectories, horizon, state"):
        grasp.compute_collision_cost_via(torch.zeros(8, 7))
