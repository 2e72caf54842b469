"""The host contract of the device sin/cos (trk_device.h: trk_sincos), CPU only.  A stand-alone program that includes the header and
calls the host side of trk_sincos is compiled with the Makefile's compiler driver and held against fp64 libm over every fp32 in
[2, 8), every 61st fp32 in [0, 1e5] and the probe list of fk_helpers.probe_angles: both functions within 3 * 2^-24 = 1.79e-7 (three
half-ulps of a result near 1), odd / even symmetry bit for bit.  The probe list's bit patterns are recorded in
tests/golden/sincos_host_bits.npz, which test_gpu_fk_edges.py holds the kernels to; this file regenerates them, so the record cannot
drift from the header.

Exhaustive maxima over every fp32 in [0, 1e5) (a one-off run of the same program): sin 1.560e-7 at 0x1.920decp+0, cos 1.304e-7 at
0x1.794a58p+12.  Beyond 1e5 the two-term reduction runs out: 3.4e-7 below 1e6, 1.0e-4 below 1e7."""
import subprocess

import numpy as np
import pytest

import fk_helpers as fh


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sincos_host")
    return fh.build_sincos_program(tmp), tmp


def test_host_sincos_within_three_half_ulps_and_symmetric(program):
    exe, _ = program
    res = subprocess.run([str(exe), "sweep"], check=True, capture_output=True, text=True)
    rep = fh.parse_report(res.stdout)
    print(res.stdout)
    assert set(rep) == {"dense_2_8", "stride61_0_1e5"}
    assert rep["dense_2_8"]["n"] == 2 ** 24 and rep["stride61_0_1e5"]["n"] == int(np.float32(1e5).view(np.uint32)) // 61 + 1
    for name, r in rep.items():
        assert r["max_sin"] <= fh.SINCOS_BOUND and r["max_cos"] <= fh.SINCOS_BOUND, (name, r)
        assert r["asym"] == 0, (name, r)
    # the sweep is not vacuous: each set comes within a few per cent of the exhaustive maxima
    assert rep["dense_2_8"]["max_sin"] > 1.4e-7 and rep["stride61_0_1e5"]["max_cos"] > 1.0e-7, rep


def test_probe_list_matches_the_recorded_bits(program):
    exe, tmp = program
    x = fh.probe_angles()
    g = np.load(fh.GOLDEN_SINCOS)
    assert 1800 <= len(x) <= 3200 and len(np.unique(fh.bits(x))) == len(x)
    assert (np.sort(np.abs(x)) == np.sort(np.abs(-x))).all() and set(fh.bits(-x).tolist()) == set(fh.bits(x).tolist())    # both signs
    for h in fh.SINCOS_WORST:
        assert np.float32(float.fromhex(h)) in x
    assert np.array_equal(g["x"], fh.bits(x)), "probe_angles() and the recorded list differ: PYTHONPATH=. python tests/fk_helpers.py"
    sb, cb, rep = fh.run_sincos_probe(exe, x, tmp)
    print(rep)
    assert np.array_equal(sb, g["sin"]) and np.array_equal(cb, g["cos"]), "trk_sincos changed: PYTHONPATH=. python tests/fk_helpers.py"
    assert rep["max_sin"] <= fh.SINCOS_BOUND and rep["max_cos"] <= fh.SINCOS_BOUND and rep["asym"] == 0, rep
    # the recorded bits through the numpy-side checks the GPU test applies to the kernels' output
    s, c = sb.view(np.float32), cb.view(np.float32)
    assert len(fh.sincos_error_faults(x, s, c)) == 0
    assert len(fh.sincos_bit_faults(s, c, g["sin"], g["cos"])) == 0
    # sin(-x) == -sin(x), cos(-x) == cos(x) across the list, by bit pattern
    at = {int(b): k for k, b in enumerate(fh.bits(x))}
    mirror = np.array([at[int(b)] for b in fh.bits(-x)])
    assert (fh.bits_nz(s[mirror]) == fh.bits_nz(-s)).all() and (fh.bits_nz(c[mirror]) == fh.bits_nz(c)).all()


def test_header_comment_states_the_measured_contract():
    text = (fh.CSRC / "trk_device.h").read_text()
    assert "1.560e-7 (sin) / 1.304e-7 (cos) for |x| <= 1e5" in text and "tests/test_device_math_cpu.py" in text
