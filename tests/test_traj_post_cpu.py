"""CPU-only checks of trajectory post-processing (trk_traj_spline_resample, trk_traj_waypoint_variance): header, ctypes mirror,
EXPORTS, library and INTEGRATION.md agree; every refusal of include/trk.h comes before any device work (the buffers are host memory
that is never read); the fp64 restatement of traj_post_helpers agrees with the reference's own results in tests/golden/traj_post.npz;
the sequential fp32 restatement stays within a quarter of the tolerances the GPU tests allow; the Python wrappers keep the
reference's assertion and IndexError; the kernels compile for gfx950 without scratch and within the LDS DESIGN.md states."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

import torch_robotics_amd as tra
import traj_post_helpers as tp
from torch_robotics_amd import _abi, _lib

ROOT = Path(__file__).resolve().parent.parent
NEW = ("trk_traj_spline_resample", "trk_traj_waypoint_variance", "trk_traj_waypoint_variance_workspace_bytes")
OK, INVALID, UNSUPPORTED = _abi.TRK_OK, _abi.TRK_ERR_INVALID_ARG, _abi.TRK_ERR_UNSUPPORTED
NAN, INF = float("nan"), float("inf")
BUF = (C.c_double * 4096)()
MODE_NAMES = {0: "zero", 1: "average", 2: "spline"}


@pytest.fixture(scope="module")
def trk():
    if not _lib.LIB_PATH.exists():
        _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    with np.load(ROOT / "tests" / "golden" / "traj_post.npz") as z:
        return {k: z[k] for k in z.files}


def err(trk):
    return trk.trk_last_error().decode()


def spline(trk, y=BUF, n=2, N=8, D=3, S=16, mode=1, dt=0.02, pos=BUF, vel=BUF):
    return trk.trk_traj_spline_resample(y, n, N, D, S, mode, dt, pos, vel, None)


def variance(trk, x=BUF, P=2, K=3, H=4, Sd=6, c0=0, dim=3, out=BUF, work=BUF, nbytes=C.sizeof(BUF)):
    return trk.trk_traj_waypoint_variance(x, P, K, H, Sd, c0, dim, out, work, nbytes, None)


def test_header_mirror_exports_library_and_documents_agree(trk):
    header = (ROOT / "include" / "trk.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(trk_[a-z0-9_]+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(trk, name), name
    for name in NEW[:2]:
        assert name in (ROOT / "INTEGRATION.md").read_text(), name
    for macro, value in (("TRK_SPLINE_MAX_POINTS", 256), ("TRK_SPLINE_MAX_OUT", 1024), ("TRK_SPLINE_MAX_DIM", 32),
                         ("TRK_WAYPOINT_VAR_MAX_PARTICLES", 4096), ("TRK_WAYPOINT_VAR_MAX_DIM", 32)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", header) and getattr(_abi, macro) == value, macro
    assert re.search(r"#define\s+TRK_ABI_VERSION\s+5\b", header) and _abi.TRK_ABI_VERSION == 5      # additive: the version stays
    assert hasattr(tra.ops, "traj_spline_resample") and hasattr(tra.ops, "traj_waypoint_variance")
    assert callable(tra.smoothen_trajectory) and callable(tra.compute_variance_waypoints)


def test_the_spline_refuses_invalid_arguments_before_any_device_work(trk):
    who = "trk_traj_spline_resample:"
    for name in ("y", "pos"):
        assert spline(trk, **{name: None}) == INVALID and err(trk).startswith(who) and "null y / pos" in err(trk), name
        assert spline(trk, n=0, **{name: None}) == OK, name                # nothing to point at
    for kw in (dict(n=-1), dict(N=1), dict(N=0), dict(N=-4), dict(S=1), dict(S=0), dict(S=-2), dict(D=0), dict(D=-1)):
        for n in ((kw["n"],) if "n" in kw else (2, 0)):
            assert spline(trk, **{**kw, "n": n}) == INVALID and "n_traj >= 0, n_points >= 2, n_out >= 2 and dim >= 1" in err(trk), kw
    assert spline(trk, n=0x3fffffff // 16 + 1, S=16) == INVALID and "above 0x3fffffff" in err(trk)
    assert spline(trk, n=0x3fffffff // 8 + 1, N=8, S=4) == INVALID and "above 0x3fffffff" in err(trk)
    for mode in (-1, 3, 7):
        assert spline(trk, mode=mode) == INVALID and "vel_mode must be 0 (zero), 1 (average) or 2 (spline)" in err(trk), mode
        assert spline(trk, mode=mode, n=0) == INVALID, mode
    for bad in (NAN, INF, -INF, 0.0, -0.02):
        assert spline(trk, mode=1, dt=bad) == INVALID and "vel_mode 1 needs dt finite and > 0" in err(trk), bad
        assert spline(trk, mode=1, dt=bad, n=0) == INVALID, bad
        assert spline(trk, mode=0, dt=bad, n=0) == OK and spline(trk, mode=2, dt=bad, n=0) == OK, bad      # dt is not used there
    for mode in (1, 2):
        assert spline(trk, mode=mode, vel=None) == INVALID and "vel_mode 1 and 2 need vel" in err(trk), mode
        assert spline(trk, mode=mode, vel=None, n=0) == INVALID, mode
    assert spline(trk, mode=0, vel=None, n=0) == OK
    # an argument error speaks before the limits, and with an empty batch too
    assert spline(trk, N=257, mode=5) == INVALID
    assert spline(trk, D=33, n=0, mode=2, vel=None) == INVALID


def test_the_spline_names_the_limit_it_refuses(trk):
    for n in (2, 0):
        assert spline(trk, N=257, n=n) == UNSUPPORTED and "TRK_SPLINE_MAX_POINTS (256)" in err(trk)
        assert spline(trk, S=1025, n=n) == UNSUPPORTED and "TRK_SPLINE_MAX_OUT (1024)" in err(trk)
        assert spline(trk, D=33, n=n) == UNSUPPORTED and "TRK_SPLINE_MAX_DIM (32)" in err(trk)
    for N, S, D in ((2, 2, 1), (256, 1024, 32), (64, 256, 7)):
        for mode in (0, 1, 2):
            assert spline(trk, N=N, S=S, D=D, mode=mode, n=0) == OK


def test_the_variance_refuses_invalid_arguments_before_any_device_work(trk):
    who = "trk_traj_waypoint_variance:"
    for kw in (dict(P=-1), dict(K=0), dict(K=-2), dict(H=0), dict(H=-1)):
        assert variance(trk, **kw) == INVALID and err(trk).startswith(who) and "n_problems >= 0, n_particles >= 1 and horizon >= 1" in err(trk), kw
    assert variance(trk, P=0, K=0) == INVALID and variance(trk, P=0, H=0) == INVALID                    # with an empty batch too
    assert variance(trk, P=0x3fffffff // 12 + 1) == INVALID and "n_problems * n_particles * horizon above 0x3fffffff" in err(trk)
    assert variance(trk, P=0x40000000, K=1, H=1) == INVALID and "above 0x3fffffff" in err(trk)
    assert variance(trk, P=1 << 20, K=4096, H=1) == INVALID and "above 0x3fffffff" in err(trk)
    for kw in (dict(dim=0), dict(dim=-1), dict(c0=-1), dict(c0=4, dim=3), dict(c0=0, dim=7), dict(Sd=0)):
        for P in (2, 0):
            assert variance(trk, P=P, **kw) == INVALID and "dim >= 1, c0 >= 0 and c0 + dim <= state_dim" in err(trk), kw
    for name in ("x", "out"):
        assert variance(trk, **{name: None}) == INVALID and "null x / out" in err(trk), name
        assert variance(trk, P=0, **{name: None}) == OK, name
    need = trk.trk_traj_waypoint_variance_workspace_bytes(2, 3, 4)
    assert need == 2 * 1 * 4 * 16
    assert variance(trk, work=None) == INVALID and "workspace" in err(trk)
    assert variance(trk, nbytes=need - 1) == INVALID and "workspace" in err(trk)
    assert variance(trk, work=C.byref(BUF, 4)) == INVALID and "8-byte aligned" in err(trk)
    assert variance(trk, P=0, work=None, nbytes=0) == OK
    # an argument error speaks before the limits
    assert variance(trk, K=4097, dim=0) == INVALID


def test_the_variance_names_the_limit_it_refuses_and_sizes_its_workspace(trk):
    for P in (1, 0):
        assert variance(trk, P=P, K=4097) == UNSUPPORTED and "TRK_WAYPOINT_VAR_MAX_PARTICLES (4096)" in err(trk)
        assert variance(trk, P=P, Sd=40, dim=33) == UNSUPPORTED and "TRK_WAYPOINT_VAR_MAX_DIM (32)" in err(trk)
    for K, H, Sd, dim in ((1, 1, 1, 1), (4096, 64, 32, 32), (8, 64, 14, 7)):
        assert variance(trk, P=0, K=K, H=H, Sd=Sd, dim=dim) == OK
    q = trk.trk_traj_waypoint_variance_workspace_bytes
    # tiles of 64 particles, one (S1, S2) pair of doubles per (problem, tile pair, way point)
    assert q(1, 64, 1) == 16 and q(1, 65, 1) == 3 * 16 and q(5, 257, 3) == 5 * 15 * 3 * 16 and q(1, 4096, 64) == 2080 * 64 * 16
    assert q(0, 8, 8) == 0
    assert q(-1, 8, 8) == -1 and q(1, 0, 8) == -1 and q(1, 4097, 8) == -1 and q(1, 8, 0) == -1


def test_the_fp64_restatement_agrees_with_the_references_spline(golden):
    """the reference's scipy route against the dense-solve Hermite form: positions within 1e-12 of the column's magnitude, the
    derivative within 1e-12 (N - 1) of it, the average velocity within 2^-24 relative (the kernel's S dt is rounded to fp32 once)"""
    seen = set()
    for k in range(int(golden["spline/n"])):
        y = golden[f"spline/{k}/y"]
        S, mode, kind = (int(v) for v in golden[f"spline/{k}/meta"])
        pos, vel = tp.spline64(y, S, MODE_NAMES[mode], float(golden[f"spline/{k}/dt"]))
        mag = tp.column_mag(y)
        assert (np.abs(pos - golden[f"spline/{k}/pos"]) <= 1e-12 * mag).all(), k
        bound = {0: 0.0, 1: 2.0 ** -24 * np.abs(golden[f"spline/{k}/vel"]), 2: 1e-12 * mag * (y.shape[0] - 1)}[mode]
        assert (np.abs(vel - golden[f"spline/{k}/vel"]) <= bound).all(), k
        seen.add((y.shape[0], S, y.shape[1], mode, kind))
    for at, want in enumerate(((2, 3, 4, 17, 64), (2, 3, 30, 64, 127), (1, 3, 7), (0, 1, 2), (0, 1, 2))):
        assert sorted({s[at] for s in seen}) == list(want)


def test_the_fp64_restatement_agrees_with_the_references_variance(golden):
    shapes = []
    for k in range(int(golden["var/n"])):
        x, want = golden[f"var/{k}/x"], float(golden[f"var/{k}/value"])
        got = float(tp.variance64(x[None], 0, x.shape[-1])[0])
        shapes.append(x.shape)
        if x.shape[0] == 1:
            assert np.isnan(want) and np.isnan(got)
        else:
            assert abs(got - want) <= 1e-12 * abs(want), k
    assert shapes == [(2, 4, 3), (8, 16, 7), (64, 8, 7), (300, 4, 2), (32, 4, 3), (1, 4, 3)]
    # the clustered case separates the two ways of forming a distance: the reference's own fp32 run and the restated cdist route miss
    # the fp64 value by far more than the GPU test allows
    k = int(golden["var/clustered"])
    x, want = golden[f"var/{k}/x"], float(golden[f"var/{k}/value"])
    assert abs(float(golden[f"var/{k}/value_fp32_reference"]) - want) > 100 * tp.var_rtol(3) * want
    assert abs(float(tp.variance_cdist32(x[None], 0, 3)[0]) - want) > 100 * tp.var_rtol(3) * want


def test_a_sequential_fp32_spline_stays_within_a_quarter_of_the_tolerances():
    """2000 random columns (walks, walks with an O(3) offset, white noise), N in {2 .. 256}, S in {2 .. 1024}: the worst
    |spline32 - spline64| is what C_P and C_V are 4 x of."""
    rng = np.random.default_rng(0)
    worst_p = worst_v = 0.0
    for case in range(2000):
        N = int(rng.choice([2, 3, 4, 5, 17, 64, 65, 100, 256]))
        S = int(rng.choice([2, 3, 30, 64, 127, 257, 1024]))
        kind = case % 3
        y = np.cumsum(0.3 * rng.standard_normal((N, 1)), 0) + (3.0 if kind == 1 else 0.0)
        if kind == 2:
            y = rng.standard_normal((N, 1))
        y = y.astype(np.float32)
        p64, v64 = tp.spline64(y, S, "spline")
        p32, v32 = tp.spline32(y, S, "spline")
        mag = tp.column_mag(y)
        worst_p = max(worst_p, float((np.abs(p32 - p64) / (tp.EPS * mag)).max()))
        worst_v = max(worst_v, float((np.abs(v32 - v64) / (tp.EPS * mag * (N - 1))).max()))
    print(f"worst ratios over 2000 cases: position {worst_p:.3f}, velocity {worst_v:.3f}")
    assert worst_p <= tp.C_P / 4 and worst_v <= tp.C_V / 4


def test_the_fp32_restatement_keeps_the_bit_properties_of_the_header():
    rng = np.random.default_rng(1)
    for N, S in ((5, 9), (64, 127), (2, 2), (3, 30), (17, 1024)):
        y = (3.0 + rng.standard_normal((N, 3))).astype(np.float32)
        y[:, 1] = np.float32(0.3)                                          # a constant column
        pos, vel = tp.spline32(y, S, "spline")
        assert np.array_equal(pos[0], y[0]) and np.array_equal(pos[-1], y[-1])
        assert np.array_equal(pos[:, 1], np.full(S, np.float32(0.3)))
        assert (vel[0] == 0).all() and (vel[-1] == 0).all()
        if (S - 1) % (N - 1) == 0:
            assert np.array_equal(pos[::(S - 1) // (N - 1)], y)


def test_the_python_wrappers_keep_the_references_assertion_and_index_error():
    y = torch.zeros((5, 3))
    with pytest.raises(AssertionError, match="Either sets the average velocity or zero velocity"):
        tra.smoothen_trajectory(y, set_average_velocity=True, zero_velocity=True)
    with pytest.raises(IndexError):
        tra.smoothen_trajectory(torch.zeros((1, 3)))
    with pytest.raises(IndexError):
        tra.smoothen_trajectory(torch.zeros((4, 1, 3)), set_average_velocity=False)
    with pytest.raises(ValueError, match="vel_mode must be one of"):
        tra.ops.traj_spline_resample(y, 8, vel_mode="fast")
    with pytest.raises(AssertionError):
        tra.compute_variance_waypoints(torch.zeros((5, 3)), None)


# the spline's tile and table are dynamic LDS (the launch asks for at most 72 KiB); the finishing kernel folds 256 doubles
LDS_STATIC = {"k_spline_resample": 0, "k_waypoint_var_pairs": 0, "k_waypoint_var_finish": 2048}


def test_the_kernels_compile_without_scratch_and_within_the_lds_design_states():
    csrc = ROOT / "torch_robotics_amd" / "csrc"
    make = (csrc / "Makefile").read_text()
    assert re.search(r"^SRCS := .*\btrk_traj_post\.hip\b", make, flags=re.M)
    hipcc = re.search(r"^HIPCC \?= (.*)$", make, flags=re.M).group(1).strip()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", make, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    with tempfile.TemporaryDirectory() as d:
        res = subprocess.run([hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "trk_traj_post.hip", "-o",
                              str(Path(d) / "traj_post_device.o")], cwd=csrc, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    seen = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", res.stderr)[1:]:
        name = block.split()[0]
        num = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))
        m = re.search(r"k_waypoint_var_pairsILi(\d+)E", name)
        for key in LDS_STATIC:
            if key in name:
                seen[(key, int(m.group(1)) if m else 0)] = (num("ScratchSize [bytes/lane]"), num("VGPRs"), num("LDS Size [bytes/block]"))
    assert sorted(seen) == [("k_spline_resample", 0), ("k_waypoint_var_finish", 0)] + [("k_waypoint_var_pairs", d) for d in (2, 4, 8, 16, 32)]
    for key, (scratch, vgprs, lds) in seen.items():
        print(f"{key}: {vgprs} VGPRs, {lds} B of static LDS, {scratch} B of scratch")
        assert scratch == 0, key
        assert lds == LDS_STATIC[key[0]], (key, lds)
        assert vgprs <= 128, key                                            # four wavefronts a SIMD at the least
    # the dynamic LDS of the spline's launch: the tile's budget and the sample table, as the source states them
    src = (csrc / "trk_traj_post.hip").read_text()
    assert re.search(r"SPLINE_TILE_BYTES = 64 \* 1024;", src) and "SPLINE_TILE_BYTES + 8 * TRK_SPLINE_MAX_OUT" in src
    assert 64 * 1024 + 8 * _abi.TRK_SPLINE_MAX_OUT <= 160 * 1024 // 2      # two workgroups of the largest launch fit one CU
