"""The fused joint-limit flag must keep its zero canonicalisation (CPU only: hipcc cross-compiles to assembly).

spec_load_q_via tests "v outside [lo, hi] or NaN" as "the bits of med3(v, lo, hi) differ from v's".  -0.0 against a +0.0 limit
(or +0.0 against a -0.0 one) is inside for the reference's `>=` / `<=` but gives differing bits, so v, lo and hi first go through
`x + 0.0f`, which turns -0.0 into +0.0 and leaves every other value alone.  A compiler allowed to ignore the sign of zero (nsz)
would fold those additions away and bring the wrong flag back without any test on ordinary inputs noticing.  Checked on the
committed headline unit: each via-point kernel (k_coll_*) keeps at least one `v_add_f32 ..., 0` per way-point value it tests
(two way points of D = 7 joints).
"""
import re

from test_isa_entry_chain_cpu import CSRC, _device_asm, _kernels

ADD_ZERO = re.compile(r"^\s*v_add_f32(_e32|_e64)?\s+v\d+,\s*(0,\s*[sv]\d+|[sv]\d+,\s*0)\s*$")


def test_limit_flag_keeps_its_zero_canonicalisation(tmp_path):
    kernels = _kernels(_device_asm(CSRC / "generated" / "spec_panda.hip", tmp_path / "spec_panda.s"))
    coll = {n: b for n, b in kernels.items() if re.search(r"k_coll_b[ig]", n)}
    assert coll, "no via-point (k_coll_*) kernel found in the assembly"
    adds = {n: sum(bool(ADD_ZERO.match(l)) for l in b) for n, b in coll.items()}
    assert all(c >= 2 * 7 for c in adds.values()), f"x + 0.0f folded away in the limit test: {adds}"
