"""CPU-only checks of the arm's planning loop (trk_rollout_gp_adam_steps, generated kernel k_traj_adam): header, EXPORTS, library and
INTEGRATION.md agree, the ctypes struct has the header's layout, bad arguments are refused before any device work (model and cost
model are blocks of zeros that are never dereferenced beyond their headers), the generator emits the kernel for the small arms only
and leaves every earlier kernel's text alone, the compiled instantiations of the committed Panda unit use no scratch, fit the
occupancy the generator states and exchange nothing through LDS inside the loop, and the task hands the plan out only where it holds."""
import ctypes as C
import hashlib
import json
import re
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

import torch_robotics_amd as tra
from torch_robotics_amd import _abi, _lib, codegen, jit
import test_isa_entry_chain_cpu as isa

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "torch_robotics_amd" / "csrc"
CPU = dict(device=torch.device("cpu"), dtype=torch.float32)
NAME = "trk_rollout_gp_adam_steps"
OK, INVALID, UNSUPPORTED = _abi.TRK_OK, _abi.TRK_ERR_INVALID_ARG, _abi.TRK_ERR_UNSUPPORTED
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def trk():
    if not _lib.LIB_PATH.exists():
        _lib.build()
    return _lib.lib()


def test_header_exports_library_and_documentation_agree(trk):
    header = (ROOT / "include" / "trk.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(trk_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert NAME in declared and NAME in _lib.EXPORTS and hasattr(trk, NAME)
    assert NAME in (ROOT / "INTEGRATION.md").read_text()


def test_struct_layout_matches_header():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "trk.h"\nint main(){printf("%zu %zu %zu %zu %zu %d\\n",sizeof(TrkTrajAdam),' \
          'offsetof(TrkTrajAdam,lr),offsetof(TrkTrajAdam,pin),offsetof(TrkTrajAdam,first_step),offsetof(TrkTrajAdam,n_steps),' \
          'TRK_TRAJ_ADAM_MAX_HORIZON);}'
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")], check=True)
        out = [int(v) for v in subprocess.run([str(Path(d) / "s")], capture_output=True, text=True, check=True).stdout.split()]
    T = _abi.TrajAdam
    assert out == [C.sizeof(T), T.lr.offset, T.pin.offset, T.first_step.offset, T.n_steps.offset, _abi.TRK_TRAJ_ADAM_MAX_HORIZON]


def test_bad_arguments_are_refused_before_any_device_work(trk):
    model = (C.c_char * 8192)()             # stand for TrkModel* / TrkCostModel*: zeroed headers (0 links, 0 DOF), nothing behind them is read
    cm = (C.c_char * 8192)()
    buf = (C.c_float * 4096)()              # host memory standing for the device buffers, never read
    W, G, A = _abi.RolloutWeights, _abi.GpPrior, _abi.TrajAdam
    w0, g0, a0 = W(1.0, 1.0, 1.0, 0.0), G(0.08, 1.0, 1.0), A(1e-2, 3, 1, 1)

    def steps(m=model, c=cm, w=w0, g=g0, a=a0, batch=2, horizon=8, q=buf):
        ref = lambda s: C.byref(s) if s is not None else None
        return trk.trk_rollout_gp_adam_steps(m, c, ref(w), ref(g), ref(a), q, buf, buf, buf, batch, horizon, buf, None)

    assert steps(m=None) == INVALID and steps(c=None) == INVALID and steps(w=None) == INVALID and steps(g=None) == INVALID
    assert steps(a=None) == INVALID and steps(q=None) == INVALID
    assert NAME.encode() in trk.trk_last_error()
    assert steps(batch=-1) == INVALID
    for h in (0, -1):
        assert steps(horizon=h) == INVALID, h
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
    # a wavefront owns whole trajectories: the horizon is a power of two up to 64, and the message says so
    for h in (3, 48, 65, 128):
        assert steps(horizon=h) == UNSUPPORTED, h
        msg = trk.trk_last_error()
        assert b"power of two" in msg and b"64" in msg, msg
    assert steps(batch=0, horizon=64) == OK


def _unit_text(ident):
    kin, tmpl = codegen.template_for(ident)
    return codegen.generate_link_kernel_source(kin, tmpl, ident)


def _kernel_blocks(text):
    """{kernel name: text from its `__global__` line (and a template line in front of it) to its closing brace in column 0}; a name that
    occurs twice (bi / bg share none) keeps every block"""
    lines, out, i = text.split("\n"), {}, 0
    while i < len(lines):
        if lines[i].startswith("__global__"):
            m = re.search(r"\b(k_[A-Za-z0-9_]+)\(", lines[i])
            start = i - 1 if i > 0 and lines[i - 1].startswith("template") else i
            end = next(j for j in range(i, len(lines)) if lines[j] == "}")
            out.setdefault(m.group(1), []).append("\n".join(lines[start:end + 1]))
            i = end
        i += 1
    return out


def test_generator_emits_the_kernel_for_small_arms_only():
    for ident, want in (("panda", True), ("iiwa7", True), ("dual_panda", False), ("ur10_allegro", False)):
        text = _unit_text(ident)
        assert ("k_traj_adam_bi" in text) == want and ("k_traj_adam_bg" in text) == want and ("launch_traj_adam" in text) == want, ident
    text = _unit_text("panda")
    body = _kernel_blocks(text)["k_traj_adam_bi"][0]
    assert "link_pos" not in body and "PosFlusher" not in body and "NoFlush flush" in body            # no position stores
    assert "__syncthreads" not in body and "#pragma nounroll" in body
    assert body.count("trk_dpp_from_next") == 2 and body.count("trk_dpp_from_prev") == 2               # inside the loop over the joints


def test_every_earlier_kernel_of_the_panda_unit_keeps_its_text():
    """tests/golden/spec_panda_kernels_r08.json: sha1 of each kernel's text in the Panda unit as committed before this kernel family
    existed -- the freshly generated unit, and the committed one, must contain exactly those texts next to the new ones"""
    want = json.loads((ROOT / "tests" / "golden" / "spec_panda_kernels_r08.json").read_text())
    fresh = _unit_text("panda")
    committed = (CSRC / "generated" / "spec_panda.hip").read_text()
    assert fresh == committed, "csrc/generated/spec_panda.hip is not what the generator writes"
    got = {k: [hashlib.sha1(b.encode()).hexdigest() for b in v] for k, v in _kernel_blocks(fresh).items()}
    new = sorted(set(got) - set(want))
    assert new == ["k_traj_adam_bg", "k_traj_adam_bi"], new
    assert {k: got[k] for k in want} == want
    # SpecArgs / IkArgs / IkGnArgs and the layout stamp: the shared header still holds their committed text
    hdr = (CSRC / "trk_spec_common.h").read_text()
    for name, sha in json.loads((ROOT / "tests" / "golden" / "spec_common_structs_r08.json").read_text()).items():
        m = re.search(r"^struct " + name + r" \{\n.*?^\};", hdr, flags=re.M | re.S)
        assert m and hashlib.sha1(m.group(0).encode()).hexdigest() == sha, name


def test_jit_cache_key_follows_the_generator():
    """a cached run-time unit is reused only under the same stamp, and the stamp hashes the generator's own source and the shared
    headers: a unit whose text this change extends cannot be served from an older cache"""
    import inspect
    src = inspect.getsource(jit._generator_stamp)
    assert "codegen.__file__" in src and "trk_spec_common.h" in src and "trk.h" in src
    stamp = jit._generator_stamp()
    assert stamp == jit._generator_stamp() and len(stamp) == 12


@pytest.fixture(scope="module")
def panda_isa(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa")
    asm = isa._device_asm(CSRC / "generated" / "spec_panda.hip", d / "spec_panda.s")
    kernels = {n: b for n, b in isa._kernels(asm).items() if "k_traj_adam" in n}
    meta = {}
    for n in kernels:
        blk = re.search(r"\.amdhsa_kernel\s+" + re.escape(n) + r"\n(.*?)\.end_amdhsa_kernel", asm, flags=re.S).group(1)
        meta[n] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(private_segment_fixed_size|next_free_vgpr|accum_offset)\s+(\d+)", blk)}
    return kernels, meta


def test_isa_no_scratch_and_the_stated_occupancy(panda_isa):
    kernels, meta = panda_isa
    assert len(kernels) == 4, sorted(kernels)             # bi / bg x BOX
    for n, m in sorted(meta.items()):
        vgprs = m["next_free_vgpr"]
        print(f"{n}: private segment {m['private_segment_fixed_size']} B, {vgprs} VGPRs (incl. AGPRs) -> {512 // (-(-vgprs // 8) * 8)} wavefronts per SIMD")
        assert m["private_segment_fixed_size"] == 0, n
        # gfx950: 512 registers per lane and SIMD, allocated in blocks of 8
        assert 512 // (-(-vgprs // 8) * 8) >= codegen.TRAJ_ADAM_OCCUPANCY, (n, vgprs)


def test_isa_nothing_crosses_a_wavefront_inside_the_loop(panda_isa):
    """The iteration loop: among the backward branches (conditional or not) whose span holds all of the prior's DPP operands, the one
    with the smallest span names the loop's header; the loop runs from there to the last backward branch to that header.  (Blocks of
    the entry that the compiler lays out behind the loop -- the scene tables' copy into LDS among them -- jump back to the entry and are
    not part of it.)  Inside: no LDS write, swizzle, permute or atomic; no barrier anywhere in the kernel.  LDS reads are the gathers
    from the wavefront's own copy of the scene tables.
    One exemption, counted and shown: the general-scene instantiation at the identity base carries k_rollout's scene text, which scores
    the collision link at a constant position once per wavefront, cooperatively (spec_object_cost_uniform_point: the wavefront's
    minimum by ds_bpermute_b32).  That belongs to the objective and stays within the wavefront; it exchanges nothing between time steps."""
    kernels, _ = panda_isa
    for n, body in sorted(kernels.items()):
        labels = {l.split(":")[0]: i for i, l in enumerate(body) if re.match(r"^\.LBB\d+_\d+:", l)}
        back = [(labels[m.group(1)], i) for i, l in enumerate(body)
                for m in [re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)] if m and m.group(1) in labels and labels[m.group(1)] < i]
        is_dpp = lambda l: "dpp" in l or "wave_sh" in l
        dpps = [i for i, l in enumerate(body) if is_dpp(l)]
        assert len(dpps) >= 4 * 7, (n, len(dpps))                        # two values from the next lane, two to the next, per joint
        around = [(a, b) for a, b in back if a <= dpps[0] and dpps[-1] <= b]
        assert around, n
        lo = min(around, key=lambda ab: ab[1] - ab[0])[0]
        hi = max(b for a, b in back if a == lo)
        loop = body[lo:hi + 1]
        exch = [l.strip() for l in loop if re.match(r"^\s*(ds_write|ds_swizzle|ds_permute|ds_bpermute|ds_add|ds_max|ds_min|ds_cmpst|ds_wrxchg|s_barrier)", l)]
        reads = sum(bool(re.match(r"^\s*ds_read", l)) for l in loop)
        print(f"{n}: loop of {len(loop)} lines, {len(dpps)} DPP operands, {reads} LDS reads (scene tables), {len(exch)} LDS writes / permutes: {sorted(set(e.split()[0] for e in exch))}")
        if "k_traj_adam_biILb1E" in n:
            exch = [l for l in exch if not l.startswith("ds_bpermute_b32")]
        assert exch == [], (n, exch[:4])
        assert all("s_barrier" not in l for l in body), n


def test_the_task_hands_the_plan_out_only_where_it_holds():
    q = torch.zeros(2, 8, 3)
    task = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=CPU), robot=tra.RobotPointMass3D(tensor_args=CPU), tensor_args=CPU)
    with pytest.raises(NotImplementedError, match="kinematic tree"):
        task.rollout_adam_plan(q, q.clone(), 0.1, 1.0)
    with pytest.raises(NotImplementedError, match="2-D point mass"):
        task.trajectory_optimizer(q, q.clone(), 0.1, 1.0)
    grasp = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=CPU),
                             robot=tra.RobotPanda(grasped_object=tra.GraspedObjectPandaBox(tensor_args=CPU), tensor_args=CPU), tensor_args=CPU)
    q7 = torch.zeros(2, 8, 7)
    with pytest.raises(NotImplementedError, match="link-column"):
        grasp.rollout_adam_plan(q7, q7.clone(), 0.1, 1.0)
