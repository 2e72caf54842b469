"""The headline fused rollout must not drain its position stores at the sphere gather (CPU only: hipcc cross-compiles to assembly).

On gfx950 loads and stores share `vmcnt`, so an `s_waitcnt vmcnt(..)` after the tick slots have issued their write-through position
chunks stops the wavefront until memory has acknowledged every chunk in flight.  The winning-centre gather of the paired sphere
ranking reads LDS; when it shared registers or a join block with the global fall-back, the waitcnt pass put the fall-back's `vmcnt`
waits on the LDS path too.  The rule checked here: after the first store a tick slot issues (the inline-asm position-chunk store),
every `vmcnt` wait in the kernel sits in a basic block that has itself issued a vector-memory load before it -- it waits for its own
gather (the > 16-sphere path), never for stores inherited from elsewhere.
"""
import re
import subprocess
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "torch_robotics_amd" / "csrc"
HEADLINE = "_ZN10spec_panda12k_rollout_biIfLb0ELb0EEEv8SpecArgs"        # k_rollout_bi<float, false, false>

BLOCK = re.compile(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)")
VMEM_LOAD = re.compile(r"^\s*(global|buffer|flat|scratch)_load")
VMCNT_WAIT = re.compile(r"^\s*s_waitcnt\b.*\bvmcnt\(")


def _device_asm(tmp_path):
    """spec_panda.hip compiled the way csrc/Makefile compiles a generated unit, device half only, to assembly."""
    mk = (CSRC / "Makefile").read_text()
    hipcc = re.search(r"^HIPCC \?= (.*)$", mk, re.M).group(1).strip()
    cxx = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    gen = re.search(r"^GENFLAGS \?= (.*)$", mk, re.M).group(1).split()
    rule = re.search(r"^generated/%\.o:.*\n\t(.*)$", mk, re.M).group(1).split()
    rule_dev = [f for i, f in enumerate(rule) if f == "-Xarch_device" or (i > 0 and rule[i - 1] == "-Xarch_device")]
    out = tmp_path / "spec_panda.s"
    subprocess.run([hipcc, *cxx, *rule_dev, *gen, "--cuda-device-only", "-S", "generated/spec_panda.hip", "-o", str(out)],
                   cwd=CSRC, check=True, capture_output=True)
    return out.read_text()


def _kernel(asm, name):
    lines = asm.split("\n")
    start = lines.index(next(l for l in lines if l.startswith(name + ":")))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    return lines[start:end + 1]


def _first_tick_store(body):
    in_asm = False
    for i, line in enumerate(body):
        if ";;#ASMSTART" in line:
            in_asm = True
        elif ";;#ASMEND" in line:
            in_asm = False
        elif in_asm and re.match(r"^\s*global_store_dwordx4\b", line):
            return i
    return None


def _inherited_vmcnt_waits(body, first):
    bad, loaded = [], False
    for i, line in enumerate(body):
        if BLOCK.match(line):
            loaded = False
        if VMEM_LOAD.match(line):
            loaded = True
        if i > first and VMCNT_WAIT.match(line) and not loaded:
            bad.append(line.strip())
    return bad


def test_headline_kernel_does_not_drain_its_position_stores(tmp_path):
    body = _kernel(_device_asm(tmp_path), HEADLINE)
    first = _first_tick_store(body)
    assert first is not None, "no inline-asm position-chunk store found in the headline kernel"
    assert sum(bool(re.match(r"^\s*ds_read_b96\b", l)) for l in body[first:]) >= 5, "the LDS gather of the winning centres is gone"
    bad = _inherited_vmcnt_waits(body, first)
    assert bad == [], f"vmcnt waits after the first tick store that no load of their own block needs: {bad}"
