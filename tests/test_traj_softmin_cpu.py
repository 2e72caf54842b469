"""CPU-only checks of the sampling-based trajectory update (trk_traj_softmin_weights, trk_traj_weighted_update): header, ctypes
mirror, EXPORTS, library and INTEGRATION.md agree; every refusal of include/trk.h comes before any device work (the buffers are
host memory that is never read) and names its argument; an empty batch returns early; the workspace query; the kernels compile
for gfx950 without scratch and with the static LDS DESIGN.md states; the fp64 restatement of traj_softmin_helpers against
scipy.special.softmax; the fp32 restatement of the update against its fp64 form within the a-priori bound."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest
from scipy.special import softmax

import torch_robotics_amd as tra
import traj_softmin_helpers as sm
from torch_robotics_amd import _abi, _lib

ROOT = Path(__file__).resolve().parent.parent
NEW = ("trk_traj_softmin_weights", "trk_traj_weighted_update", "trk_traj_weighted_update_workspace_bytes",
       "trk_traj_softmin_weights_workspace_bytes")
OK, INVALID, UNSUPPORTED = _abi.TRK_OK, _abi.TRK_ERR_INVALID_ARG, _abi.TRK_ERR_UNSUPPORTED
NAN, INF = float("nan"), float("inf")
BUF = (C.c_double * 4096)()
KEEP = object()


@pytest.fixture(scope="module")
def trk():
    if not _lib.LIB_PATH.exists():
        _lib.build()
    return _lib.lib()


def err(trk):
    return trk.trk_last_error().decode()


def weights(trk, s=KEEP, temperature=1.0, mode=0, K=3, cost=BUF, valid=None, P=2, H=4, w=BUF, ess=BUF, work=BUF, nbytes=C.sizeof(BUF)):
    s = C.byref(_abi.Softmin(temperature, mode, K)) if s is KEEP else s
    return trk.trk_traj_softmin_weights(s, cost, valid, P, H, w, ess, work, nbytes, None)


def update(trk, u=KEEP, step=1.0, pin=3, K=3, per_wp=0, x=BUF, mean=BUF, w=BUF, lo=None, hi=None, P=2, H=4, D=3, out=BUF, work=BUF,
           nbytes=C.sizeof(BUF)):
    u = C.byref(_abi.WeightedUpdate(step, pin, K, per_wp)) if u is KEEP else u
    return trk.trk_traj_weighted_update(u, x, mean, w, lo, hi, P, H, D, out, work, nbytes, None)


def test_header_mirror_exports_library_and_documents_agree(trk):
    header = (ROOT / "include" / "trk.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(trk_[a-z0-9_]+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(trk, name), name
        assert name in (ROOT / "INTEGRATION.md").read_text(), name
    assert re.search(r"#define\s+TRK_SOFTMIN_MAX_PARTICLES\s+4096\b", header) and _abi.TRK_SOFTMIN_MAX_PARTICLES == 4096
    assert re.search(r"TRK_SOFTMIN_TRAJECTORY = 0, TRK_SOFTMIN_WAYPOINT = 1", header)
    assert (_abi.TRK_SOFTMIN_TRAJECTORY, _abi.TRK_SOFTMIN_WAYPOINT) == (0, 1)
    assert re.search(r"#define\s+TRK_ABI_VERSION\s+5\b", header) and _abi.TRK_ABI_VERSION == 5      # additive: the version stays
    assert hasattr(tra.ops, "traj_softmin_weights") and hasattr(tra.ops, "traj_weighted_update")
    assert callable(tra.PlanningTask.sampling_optimizer)
    src = '#include <stdio.h>\n#include "trk.h"\nint main(){printf("%zu %zu\\n",sizeof(TrkSoftmin),sizeof(TrkWeightedUpdate));}'
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")], check=True)
        out = subprocess.run([str(Path(d) / "s")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(_abi.Softmin), C.sizeof(_abi.WeightedUpdate)] == [12, 16]


def test_the_weights_refuse_invalid_arguments_before_any_device_work(trk):
    who = "trk_traj_softmin_weights:"
    for P in (2, 0):
        assert weights(trk, s=None, P=P) == INVALID and err(trk).startswith(who) and "null s" in err(trk)
        for bad in (NAN, INF, -INF, 0.0, -1.0):
            assert weights(trk, temperature=bad, P=P) == INVALID and "temperature must be finite and > 0" in err(trk), bad
        for mode in (-1, 2, 7):
            assert weights(trk, mode=mode, P=P) == INVALID and "mode must be TRK_SOFTMIN_TRAJECTORY (0) or TRK_SOFTMIN_WAYPOINT (1)" in err(trk)
        for kw in (dict(K=0), dict(K=-3), dict(H=0), dict(H=-1)):
            assert weights(trk, P=P, **kw) == INVALID and "n_problems >= 0, n_particles >= 1 and horizon >= 1" in err(trk), kw
    assert weights(trk, P=-1) == INVALID and "n_problems >= 0" in err(trk)
    assert weights(trk, P=0x3fffffff // 3 + 1) == INVALID and "n_problems * n_particles above 0x3fffffff" in err(trk)
    assert weights(trk, P=0x3fffffff, K=1, H=64, mode=1) == INVALID and "n_problems * ceil(horizon / 16) above 0x7fffffff" in err(trk)
    for name in ("cost", "w"):
        assert weights(trk, **{name: None}) == INVALID and err(trk).startswith(who) and "null cost / w" in err(trk), name
        assert weights(trk, P=0, **{name: None}) == OK, name
    # an argument error speaks before the limit, and with an empty batch too
    assert weights(trk, K=4097, mode=5) == INVALID and weights(trk, K=4097, temperature=0.0, P=0) == INVALID


def test_the_weights_name_the_limit_and_return_early_on_an_empty_batch(trk):
    for P in (1, 0):
        for mode in (0, 1):
            assert weights(trk, P=P, K=4097, mode=mode) == UNSUPPORTED and "TRK_SOFTMIN_MAX_PARTICLES (4096)" in err(trk)
    for K, H in ((1, 1), (4096, 256), (8, 64)):
        for mode in (0, 1):
            assert weights(trk, P=0, K=K, H=H, mode=mode) == OK
            assert weights(trk, P=0, K=K, H=H, mode=mode, ess=None, valid=None, cost=None, w=None, work=None, nbytes=0) == OK
    q = trk.trk_traj_softmin_weights_workspace_bytes
    # one launch up to 256 particles, at horizon 1 and in the way-point mode; beyond: one double per row
    assert q(5, 256, 64, 0) == 0 and q(5, 257, 1, 0) == 0 and q(5, 4096, 64, 1) == 0 and q(0, 257, 64, 0) == 0
    assert q(5, 257, 2, 0) == 5 * 257 * 8 and q(1, 4096, 64, 0) == 4096 * 8
    for bad in ((-1, 8, 8, 0), (1, 0, 8, 0), (1, 4097, 8, 0), (1, 8, 0, 0), (1, 8, 8, 2), (1, 8, 8, -1), (1 << 29, 8, 1, 0)):
        assert q(*bad) == -1, bad
    who = "trk_traj_softmin_weights:"
    assert weights(trk, K=257, work=None) == INVALID and err(trk).startswith(who) and "workspace" in err(trk)
    assert weights(trk, K=257, nbytes=2 * 257 * 8 - 1) == INVALID and "trk_traj_softmin_weights_workspace_bytes" in err(trk)
    assert weights(trk, K=257, work=C.byref(BUF, 4)) == INVALID and "8-byte aligned" in err(trk)
    assert weights(trk, K=257, mode=1, work=None, nbytes=0, cost=None) == INVALID and "null cost / w" in err(trk)      # no workspace needed there
    assert weights(trk, K=4097, work=None) == UNSUPPORTED


def test_the_update_refuses_invalid_arguments_before_any_device_work(trk):
    who = "trk_traj_weighted_update:"
    for P in (2, 0):
        assert update(trk, u=None, P=P) == INVALID and err(trk).startswith(who) and "null u" in err(trk)
        for bad in (NAN, INF, -INF):
            assert update(trk, step=bad, P=P) == INVALID and "step must be finite" in err(trk), bad
        for pin in (-1, 4, 15):
            assert update(trk, pin=pin, P=P) == INVALID and "pin must be 0 .. 3" in err(trk), pin
        for per_wp in (-1, 2):
            assert update(trk, per_wp=per_wp, P=P) == INVALID and "w_per_waypoint must be 0 or 1" in err(trk), per_wp
        for kw in (dict(K=0), dict(K=-3), dict(H=0), dict(H=-1), dict(D=0), dict(D=-2)):
            assert update(trk, P=P, **kw) == INVALID and "n_problems >= 0, n_particles >= 1, horizon >= 1 and dim >= 1" in err(trk), kw
        for kw in (dict(lo=BUF), dict(hi=BUF)):
            assert update(trk, P=P, **kw) == INVALID and "only one of lo / hi" in err(trk), kw
        assert update(trk, P=P, H=1 << 20, D=1 << 11) == INVALID and "horizon * dim above 0x3fffffff" in err(trk)
    assert update(trk, P=-1) == INVALID and "n_problems >= 0" in err(trk)
    assert update(trk, P=0x3fffffff // 3 + 1) == INVALID and "n_problems * n_particles above 0x3fffffff" in err(trk)
    assert update(trk, P=0x3fffffff, K=1, H=1 << 10, D=1 << 10) == INVALID and "above 0x7fffffff" in err(trk)
    for name in ("x", "mean", "w", "out"):
        assert update(trk, **{name: None}) == INVALID and err(trk).startswith(who) and "null x / mean / w / out" in err(trk), name
        assert update(trk, P=0, **{name: None}) == OK, name
    for step in (0.0, -0.5, 1.0, 3.0):
        for pin in (0, 1, 2, 3):
            assert update(trk, P=0, step=step, pin=pin, lo=BUF, hi=BUF) == OK and update(trk, P=0, step=step, pin=pin, per_wp=1) == OK
    # an argument error speaks before the limit
    assert update(trk, K=4097, pin=9) == INVALID


def test_the_update_names_the_limit_and_sizes_its_workspace(trk):
    for P in (1, 0):
        assert update(trk, P=P, K=4097) == UNSUPPORTED and "TRK_SOFTMIN_MAX_PARTICLES (4096)" in err(trk)
    q = trk.trk_traj_weighted_update_workspace_bytes
    # up to 64 particles: one launch, no workspace; beyond: one fp32 sum per (problem, chunk of 64 particles, element)
    assert q(5, 1, 3, 7) == 0 and q(5, 64, 3, 7) == 0 and q(0, 65, 3, 7) == 0
    assert q(5, 65, 3, 7) == 5 * 2 * 21 * 4 and q(1, 4096, 64, 7) == 64 * 448 * 4 and q(2, 257, 1, 1) == 2 * 5 * 4
    for bad in ((-1, 8, 8, 3), (1, 0, 8, 3), (1, 4097, 8, 3), (1, 8, 0, 3), (1, 8, 8, 0), (1, 8, 1 << 20, 1 << 11), (1 << 29, 8, 1, 1)):
        assert q(*bad) == -1, bad
    # K <= 64 needs none; K > 64 refuses a workspace that is null, misaligned or too small -- after the limit, not with an empty batch
    assert update(trk, P=0, K=64, work=None, nbytes=0) == OK and update(trk, P=0, K=65, work=None, nbytes=0) == OK
    need = q(2, 65, 4, 3)
    assert need == 2 * 2 * 12 * 4
    who = "trk_traj_weighted_update:"
    assert update(trk, K=65, work=None) == INVALID and err(trk).startswith(who) and "workspace" in err(trk)
    assert update(trk, K=65, nbytes=need - 1) == INVALID and "trk_traj_weighted_update_workspace_bytes" in err(trk)
    assert update(trk, K=65, work=C.byref(BUF, 2)) == INVALID and "4-byte aligned" in err(trk)
    assert update(trk, K=4097, work=None) == UNSUPPORTED


# the two folds of 1024 doubles, and in the trajectory mode the 4096 summed scores of a problem
LDS_STATIC = {"k_softmin_row_sums": 0, "k_softmin_weightsILb0E": 49152, "k_softmin_weightsILb1E": 16384, "k_weighted_updateILb0E": 0, "k_weighted_updateILb1E": 0,
              "k_weighted_update_finish": 0}


def test_the_kernels_compile_without_scratch_and_with_the_lds_design_states():
    csrc = ROOT / "torch_robotics_amd" / "csrc"
    make = (csrc / "Makefile").read_text()
    assert re.search(r"^SRCS := .*\btrk_traj_softmin\.hip\b", make, flags=re.M)
    hipcc = re.search(r"^HIPCC \?= (.*)$", make, flags=re.M).group(1).strip()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", make, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    assert "-ffp-contract=off" in flags                                    # the fp32 half is restated operation by operation
    with tempfile.TemporaryDirectory() as d:
        res = subprocess.run([hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "trk_traj_softmin.hip",
                              "-o", str(Path(d) / "traj_softmin_device.o")], cwd=csrc, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    seen = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", res.stderr)[1:]:
        name = block.split()[0]
        num = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))
        for key in LDS_STATIC:
            if key in name:
                seen[key] = (num("ScratchSize [bytes/lane]"), num("VGPRs"), num("LDS Size [bytes/block]"))
    assert sorted(seen) == sorted(LDS_STATIC)
    for key, (scratch, vgprs, lds) in seen.items():
        print(f"{key}: {vgprs} VGPRs, {lds} B of static LDS, {scratch} B of scratch")
        assert scratch == 0, key
        assert lds == LDS_STATIC[key], (key, lds)
        assert vgprs <= 128, key                    # a workgroup of 1024 lanes is four wavefronts a SIMD: 128 registers at the most


def test_the_fp64_restatement_agrees_with_scipys_softmax():
    """trajectory mode: softmax(-S / lambda) of the summed scores; way-point mode: softmax(-(c - lo) / ((hi - lo) lambda)) down the
    particles; both within 1e-13 relative (plus the rounding of scipy's exponent), weights summing to 1, ess = 1 / sum w^2, uniform scores giving 1 / K and ess = K"""
    rng = np.random.default_rng(0)
    for K in (1, 2, 3, 63, 64, 65, 130, 257):
        for H in (1, 3, 64, 65):
            P = 3
            c = (rng.random((P * K, H)) * 4).astype(np.float32)
            c64 = c.astype(np.float64)
            for lam in (0.1, 1.0, 50.0):
                lam32 = float(np.float32(lam))
                w, ess = sm.weights64(c, K, lam, "trajectory")
                want = softmax(-c64.sum(1).reshape(P, K) / lam32, axis=1)
                # scipy rounds -S / lambda before it subtracts the maximum: the exponents differ by a few 2^-53 of the largest one
                rt = 1e-13 + 8 * 2.0 ** -53 * float(c64.sum(1).max()) / lam32
                assert w.shape == (P * K,) and ess.shape == (P,)
                assert np.allclose(w.reshape(P, K), want, rtol=rt, atol=1e-300)
                assert np.allclose(w.reshape(P, K).sum(1), 1.0, rtol=1e-13) and np.allclose(ess, 1.0 / (want ** 2).sum(1), rtol=4 * rt)
                w, ess = sm.weights64(c, K, lam, "waypoint")
                v = c64.reshape(P, K, H)
                lo, hi = v.min(1, keepdims=True), v.max(1, keepdims=True)
                want = softmax(-(v - lo) / np.where(hi > lo, (hi - lo) * lam32, 1.0), axis=1)
                assert w.shape == (P * K, H) and ess.shape == (P, H)
                assert np.allclose(w.reshape(P, K, H), want, rtol=1e-13, atol=1e-300)
                assert np.allclose(w.reshape(P, K, H).sum(1), 1.0, rtol=1e-13) and np.allclose(ess, 1.0 / (want ** 2).sum(1), rtol=1e-12)
            for mode in ("trajectory", "waypoint"):
                w, ess = sm.weights64(np.full((P * K, H), 2.5, np.float32), K, 1.0, mode)
                assert np.allclose(w, 1.0 / K, rtol=1e-15) and np.allclose(ess, K, rtol=1e-13)


def test_the_fp64_restatement_rejects_invalid_and_non_finite_scores():
    c = np.array([[1.0, 2.0], [NAN, 1.0], [INF, 0.5], [0.5, -INF], [0.25, 0.25], [3.0, 3.0]], np.float32)
    valid = np.array([1, 1, 1, 1, 0, 7], np.uint8)
    w, ess = sm.weights64(c, 6, 1.0, "trajectory", valid)
    assert (w[[1, 2, 3, 4]] == 0).all() and w[0] > w[5] > 0 and abs(w.sum() - 1) < 1e-15 and 1 < ess[0] < 2
    w, ess = sm.weights64(c, 6, 1.0, "waypoint", valid)
    assert (w[[1, 2], 0] == 0).all() and (w[3, 1] == 0) and (w[4] == 0).all() and np.allclose(w.sum(0), 1.0)
    assert w[1, 1] > 0 and w[2, 1] == w[:, 1].max()
    # no candidate: zeros and ess 0, in its own problem only
    w, ess = sm.weights64(c, 3, 1.0, "trajectory", np.array([1, 1, 1, 0, 0, 0], np.uint8))
    assert w[0] == 1 and (w[1:] == 0).all() and ess.tolist() == [1.0, 0.0]


def test_the_fp32_update_restatement_stays_within_the_a_priori_bound():
    """every (K, H, dim) of the GPU test's grid, both weight layouts, three steps, with pins and limits: |update32 - update64| <=
    (K + 3) 2^-24 (|mean| + |step| sum |w| |x - mean|); the worst fraction is printed"""
    rng = np.random.default_rng(1)
    worst = 0.0
    for K in (1, 2, 3, 63, 64, 65, 130, 257):
        for H, D in ((1, 1), (3, 7), (64, 3), (3, 32), (1, 14)):
            P = 2
            mean = rng.standard_normal((P, H, D)).astype(np.float32)
            x = (mean[:, None] + 0.3 * rng.standard_normal((P, K, H, D))).astype(np.float32).reshape(P * K, H, D)
            for per_wp in (False, True):
                w = sm.weights64(rng.random((P * K, H)).astype(np.float32) * 3, K, 0.5, "waypoint" if per_wp else "trajectory")[0].astype(np.float32)
                for step in (0.0, 0.5, 1.0):
                    for pin, lim in ((0, None), (3, (np.full(D, -0.8, np.float32), np.full(D, 0.9, np.float32)))):
                        lo, hi = lim if lim else (None, None)
                        got = sm.update32(mean, x, w, step, pin, lo, hi)
                        ref, mag = sm.update64(mean, x, w, step, pin, lo, hi)
                        e = np.abs(got.astype(np.float64) - ref)
                        assert (e <= sm.update_bound(K, mag)).all(), (K, H, D, per_wp, step, pin)
                        worst = max(worst, float((e / sm.update_bound(K, mag)).max()))
                        if step == 0.0 and lim is None:
                            assert np.array_equal(got.view(np.uint32), mean.view(np.uint32))
                        if pin == 3:
                            assert np.array_equal(got[:, 0].view(np.uint32), mean[:, 0].view(np.uint32))
                            assert np.array_equal(got[:, -1].view(np.uint32), mean[:, -1].view(np.uint32))
    print(f"worst |update32 - update64| / bound = {worst:.3f}")


def test_the_update_restatement_skips_zero_weights_by_select():
    mean = np.zeros((1, 2, 2), np.float32)
    x = np.array([[[1, 2], [3, 4]], [[NAN, INF], [-INF, NAN]], [[2, 2], [2, 2]]], np.float32)
    w = np.array([0.25, 0.0, 0.75], np.float32)
    got = sm.update32(mean, x, w, 1.0)
    assert np.array_equal(got, np.array([[[1.75, 2.0], [2.25, 2.5]]], np.float32))
    assert np.array_equal(sm.update64(mean, x, w, 1.0)[0], got.astype(np.float64))
    w[1] = -0.0
    assert np.array_equal(sm.update32(mean, x, w, 1.0), got)


def test_the_python_wrappers_refuse_host_tensors_and_unknown_modes():
    import torch
    with pytest.raises(ValueError, match="mode must be one of"):
        tra.ops.traj_softmin_weights(torch.zeros((4, 3)), 2, 1.0, mode="softmax")
    with pytest.raises(ValueError, match=r"cost must be a \(problems \* n_particles, horizon\).*no CPU path"):
        tra.ops.traj_softmin_weights(torch.zeros((4, 3)), 2, 1.0)
    with pytest.raises(ValueError, match=r"mean must be a \(problems, horizon, dim\) tensor on a GPU \(there is no CPU path\)"):
        tra.ops.traj_weighted_update(torch.zeros((2, 3, 4)), torch.zeros((4, 3, 4)), torch.zeros((4,)))
