"""The generated kernels' entry must be one memory round trip (CPU only: hipcc cross-compiles to assembly).

Two things used to serialise the front of every wavefront of a fused rollout.  The work-item / work-group IDs (and atan2f in the IK
kernel) were out-of-line device-library calls -- a unit built with -mno-amdgpu-ieee cannot inline them -- and each callee starts
with a full `s_waitcnt vmcnt(0) ...`, which drained the scene table load issued in front of it.  And spec_load_q wrote each
16-byte q chunk to LDS before the next chunk's load, a vmcnt(0) apiece.  Checked here, on the committed headline unit and on a
unit generated now with another D (UR10 + Allegro, D = 22, ring-staged positions):
  - no kernel contains an out-of-line call (`s_swappc_b64`);
  - in every k_rollout_* / k_rollout_gpt_* instantiation, every vector-memory load in front of the first LDS read (the q
    transpose) is issued before the first vmcnt wait.
"""
import re
import subprocess
from pathlib import Path

import pytest

from torch_robotics_amd import codegen

CSRC = Path(__file__).resolve().parent.parent / "torch_robotics_amd" / "csrc"

VMEM_LOAD = re.compile(r"^\s*(global|buffer|flat)_load")
VMCNT_WAIT = re.compile(r"^\s*s_waitcnt\b.*\bvmcnt\(")
DS_READ = re.compile(r"^\s*ds_read")


def _device_asm(src: Path, out: Path) -> str:
    """`src` compiled the way csrc/Makefile compiles a generated unit, device half only, to assembly."""
    mk = (CSRC / "Makefile").read_text()
    hipcc = re.search(r"^HIPCC \?= (.*)$", mk, re.M).group(1).strip()
    cxx = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    gen = re.search(r"^GENFLAGS \?= (.*)$", mk, re.M).group(1).split()
    rule = re.search(r"^generated/%\.o:.*\n\t(.*)$", mk, re.M).group(1).split()
    rule_dev = [f for i, f in enumerate(rule) if f == "-Xarch_device" or (i > 0 and rule[i - 1] == "-Xarch_device")]
    subprocess.run([hipcc, *cxx, f"-I{CSRC}", *rule_dev, *gen, "--cuda-device-only", "-S", str(src), "-o", str(out)],
                   cwd=CSRC, check=True, capture_output=True)
    return out.read_text()


def _kernels(asm: str):
    """{mangled name: body lines} of every kernel (an .amdhsa_kernel descriptor names it)"""
    lines = asm.split("\n")
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    out = {}
    for name in names:
        start = lines.index(name + ":") if name + ":" in lines else next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if re.match(r"^\s*\.Lfunc_end\d+:", lines[i]))
        out[name] = lines[start:end]
    return out


def _late_loads(body):
    """vector-memory loads in front of the first LDS read that come after a vmcnt wait"""
    waited, late = False, []
    for line in body:
        if DS_READ.match(line):
            return late
        if VMCNT_WAIT.match(line):
            waited = True
        elif VMEM_LOAD.match(line) and waited:
            late.append(line.strip())
    raise AssertionError("no LDS read (the q transpose) in the kernel")


def _unit(tmp_path, ident):
    if ident == "panda":
        return CSRC / "generated" / "spec_panda.hip"
    kin, tmpl = codegen.template_for(ident)
    src = tmp_path / f"spec_{ident}.hip"
    src.write_text(codegen.generate_link_kernel_source(kin, tmpl, ident))
    return src


@pytest.mark.parametrize("ident", ["panda", "ur10_allegro"])
def test_generated_kernels_have_a_one_round_trip_entry(tmp_path, ident):
    if ident != "panda":
        assert codegen.template_for(ident)[0].n_dofs == 22
    kernels = _kernels(_device_asm(_unit(tmp_path, ident), tmp_path / f"spec_{ident}.s"))
    assert kernels, "no kernels found in the assembly"
    calls = {n: sum("s_swappc_b64" in l for l in b) for n, b in kernels.items()}
    assert {n: c for n, c in calls.items() if c} == {}, "out-of-line calls in generated kernels"
    rollouts = [n for n in kernels if re.search(r"k_rollout_(bi|bg|gpt_bi|gpt_bg)I", n)]
    assert any("k_rollout_bi" in n for n in rollouts), "no k_rollout instantiation found"
    late = {n: _late_loads(kernels[n]) for n in rollouts}
    assert {n: v for n, v in late.items() if v} == {}, "loads in front of the q transpose issued after a vmcnt wait"
