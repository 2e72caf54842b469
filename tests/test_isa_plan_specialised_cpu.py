"""The plan-specialised rollout kernel is less code than the generic one (CPU only: hipcc cross-compiles to assembly).

k_rollout_fx compiles in what a bound plan fixes -- the objective terms, the outputs, the scene's sphere-pair count -- and reads the
constant collision point from a record.  Checked on the committed headline unit, c2 instantiation (obstacle + EE cost, positions,
per-wavefront sums, 5 sphere pairs) against k_rollout_bi<float, false, false>, and nothing else:
  - fewer basic blocks and fewer VALU instructions;
  - no stamp code (no shader-clock read);
  - no more VGPRs, and no scratch.
"""
import re

import pytest

from test_isa_entry_chain_cpu import CSRC, _device_asm, _kernels

GENERIC = "_ZN10spec_panda12k_rollout_biIfLb0ELb0EEEv8SpecArgs"
FX_C2 = re.compile(r"^_ZN10spec_panda\d+k_rollout_fx39_biIfLi5EEEv8SpecArgs$")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return _device_asm(CSRC / "generated" / "spec_panda.hip", tmp_path_factory.mktemp("isa") / "spec_panda.s")


def _counts(asm, name):
    body = _kernels(asm)[name]
    desc = asm[asm.index(f".amdhsa_kernel {name}"):]
    desc = desc[:desc.index(".end_amdhsa_kernel")]
    return dict(blocks=sum(bool(re.match(r"^\.LBB\d+_\d+:", l)) for l in body),
                valu=sum(bool(re.match(r"^\s*v_", l)) for l in body),
                clock_reads=sum(bool(re.match(r"^\s*s_mem(real)?time", l)) for l in body),
                vgprs=int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", desc).group(1)),
                scratch=int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1)))


def test_c2_instantiation_is_less_code_than_the_generic_kernel(asm):
    names = list(_kernels(asm))
    fx = [n for n in names if FX_C2.match(n)]
    assert GENERIC in names and len(fx) == 1, names
    g, f = _counts(asm, GENERIC), _counts(asm, fx[0])
    print("generic", g, "plan-specialised", f)
    assert g["clock_reads"] > 0 and f["clock_reads"] == 0
    assert f["blocks"] < g["blocks"]
    assert f["valu"] < g["valu"]
    assert f["vgprs"] <= g["vgprs"]
    assert f["scratch"] == 0 and g["scratch"] == 0
