"""CPU-only checks of multi-particle planning (trk_gp_prior_sample, trk_traj_select_best): header, ctypes mirror, EXPORTS, library and
INTEGRATION.md agree; every refusal of include/trk.h comes before any device work (the buffers are host memory that is never read);
the fp64 reference of gp_sample_helpers is the conditional Gaussian of the prior's precision and a straight line at eps = 0; a
sequential fp32 restatement stays well inside the tolerance the GPU tests allow; the kernels compile for gfx950 without scratch and
within the LDS cap."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import torch_robotics_amd as tra
import gp_sample_helpers as gs
from torch_robotics_amd import _abi, _lib

ROOT = Path(__file__).resolve().parent.parent
NEW = ("trk_gp_prior_sample", "trk_traj_select_best")
OK, INVALID, UNSUPPORTED = _abi.TRK_OK, _abi.TRK_ERR_INVALID_ARG, _abi.TRK_ERR_UNSUPPORTED
NAN, INF = float("nan"), float("inf")
BUF = (C.c_float * 4096)()


@pytest.fixture(scope="module")
def trk():
    if not _lib.LIB_PATH.exists():
        _lib.build()
    return _lib.lib()


def err(trk):
    return trk.trk_last_error().decode()


def sample(trk, s=(0.08, 1.0, 2, 0), start=BUF, goal=BUF, sv=BUF, gv=BUF, eps=BUF, q_min=BUF, q_max=BUF, P=2, H=8, D=3, q=BUF, qd=BUF):
    st = None if s is None else _abi.GpSample(*s)
    return trk.trk_gp_prior_sample(None if st is None else C.byref(st), start, goal, sv, gv, eps, q_min, q_max, P, H, D, q, qd, None)


def select(trk, score=BUF, is_free=BUF, P=2, K=3, best=BUF, best_score=BUF, n_free=BUF):
    return trk.trk_traj_select_best(score, is_free, P, K, best, best_score, n_free, None)


def test_header_mirror_exports_library_and_documents_agree(trk):
    header = (ROOT / "include" / "trk.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(trk_[a-z0-9_]+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(trk, name)
        assert name in (ROOT / "INTEGRATION.md").read_text()
    assert re.search(r"#define\s+TRK_GP_SAMPLE_MAX_HORIZON\s+256\b", header) and _abi.TRK_GP_SAMPLE_MAX_HORIZON == 256
    assert re.search(r"#define\s+TRK_GP_SAMPLE_MAX_DOF\s+32\b", header) and _abi.TRK_GP_SAMPLE_MAX_DOF == 32
    assert re.search(r"#define\s+TRK_ABI_VERSION\s+5\b", header) and _abi.TRK_ABI_VERSION == 5      # additive: the version stays
    # TrkGpSample as the C compiler lays it out against the ctypes mirror
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "trk.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n",sizeof(TrkGpSample),'
           'offsetof(TrkGpSample,dt),offsetof(TrkGpSample,sigma),offsetof(TrkGpSample,n_particles),offsetof(TrkGpSample,pin_vel));}')
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")], check=True)
        out = [int(v) for v in subprocess.run([str(Path(d) / "s")], capture_output=True, text=True, check=True).stdout.split()]
    S = _abi.GpSample
    assert out == [C.sizeof(S), S.dt.offset, S.sigma.offset, S.n_particles.offset, S.pin_vel.offset] == [16, 0, 4, 8, 12]
    assert hasattr(tra.ops, "gp_prior_sample") and hasattr(tra.ops, "traj_select_best")
    assert hasattr(tra.PlanningTask, "sample_gp_trajs") and hasattr(tra.PlanningTask, "select_best_trajs")


def test_the_sampler_refuses_invalid_arguments_before_any_device_work(trk):
    who = "trk_gp_prior_sample:"
    assert sample(trk, s=None) == INVALID and err(trk).startswith(who) and "null TrkGpSample" in err(trk)
    for name in ("start", "goal", "eps", "q", "qd"):
        assert sample(trk, **{name: None}) == INVALID and "null start / goal / eps / q / qd" in err(trk), name
        assert sample(trk, P=0, **{name: None}) == OK, name               # nothing to point at
    for name in ("sv", "gv"):
        assert sample(trk, s=(0.08, 1.0, 2, 1), **{name: None}) == INVALID and "pin_vel needs start_vel and goal_vel" in err(trk), name
        assert sample(trk, s=(0.08, 1.0, 2, 1), P=0, **{name: None}) == INVALID, name
        assert sample(trk, s=(0.08, 1.0, 2, 0), P=0, **{name: None}) == OK, name      # ignored without pin_vel
    assert sample(trk, q_min=None) == INVALID and "only one of q_min / q_max" in err(trk)
    assert sample(trk, q_max=None) == INVALID and "only one of q_min / q_max" in err(trk)
    assert sample(trk, q_min=None, q_max=None, P=0) == OK
    for bad in (NAN, INF, -INF, 0.0, -0.1):
        assert sample(trk, s=(bad, 1.0, 2, 0)) == INVALID and "dt and sigma must be finite and > 0" in err(trk), bad
        assert sample(trk, s=(0.08, bad, 2, 0), P=0) == INVALID and "dt and sigma must be finite and > 0" in err(trk), bad
    for k in (0, -1):
        assert sample(trk, s=(0.08, 1.0, k, 0)) == INVALID and "n_particles must be >= 1" in err(trk), k
    for pv in (-1, 2, 7):
        assert sample(trk, s=(0.08, 1.0, 2, pv)) == INVALID and "pin_vel 0 or 1" in err(trk), pv
    for kw in (dict(H=1), dict(H=0), dict(H=-5), dict(D=0), dict(D=-1), dict(P=-1)):
        assert sample(trk, **kw) == INVALID and "n_problems >= 0, horizon >= 2 and dof >= 1" in err(trk), kw
    assert sample(trk, s=(0.08, 1.0, 2, 0), P=0x20000000) == INVALID and "above 0x3fffffff" in err(trk)
    assert sample(trk, s=(0.08, 1.0, 0x40000000, 0), P=1) == INVALID and "above 0x3fffffff" in err(trk)
    # an argument error speaks before the limits, and with an empty batch too
    assert sample(trk, H=257, s=(NAN, 1.0, 2, 0)) == INVALID
    assert sample(trk, D=33, P=0, q_min=None) == INVALID


def test_the_sampler_names_the_limit_it_refuses(trk):
    for P in (2, 0):
        assert sample(trk, H=257, P=P) == UNSUPPORTED and "TRK_GP_SAMPLE_MAX_HORIZON (256)" in err(trk)
        assert sample(trk, D=33, P=P) == UNSUPPORTED and "TRK_GP_SAMPLE_MAX_DOF (32)" in err(trk)
    for H, D in ((2, 1), (256, 32), (64, 7)):
        assert sample(trk, H=H, D=D, P=0) == OK


def test_the_pick_refuses_invalid_arguments_before_any_device_work(trk):
    who = "trk_traj_select_best:"
    for kw in (dict(P=-1), dict(K=0), dict(K=-3)):
        assert select(trk, **kw) == INVALID and err(trk).startswith(who) and "n_problems >= 0 and n_particles >= 1" in err(trk), kw
    assert select(trk, P=0, K=0) == INVALID                                # with an empty batch too
    assert select(trk, P=0x20000000, K=2) == INVALID and "above 0x3fffffff" in err(trk)
    for name in ("score", "best"):
        assert select(trk, **{name: None}) == INVALID and "null score / best" in err(trk), name
        assert select(trk, P=0, **{name: None}) == OK
    assert select(trk, P=0, is_free=None, best_score=None, n_free=None) == OK


@pytest.mark.parametrize("pin_vel", (False, True))
def test_the_reference_is_the_conditional_gaussian_of_the_priors_precision(pin_vel):
    """sample64 is affine in eps: x = m + A eps.  With unit normals its covariance is A A^T and its mean m; both against dense
    conditioning of the block-tridiagonal precision built from the a, b, c of trk_gp_prior_cost_grad, at H = 9 in fp64.  The bounds
    are fp64 roundings through the inverse of a matrix whose condition number is ~ 1e6 (relative 1e-9 of the largest entry)."""
    H, dt, sigma = 9, 5.0 / 64, 2.0
    start, goal, sv, gv = 0.7, -1.3, 0.4, -0.9
    one = lambda v: np.array([[v]])

    def run(eps):
        q, qd, _, _ = gs.sample64(one(start), one(goal), eps.reshape(1, H - 1, 1, 2), dt, sigma, 1, pin_vel, one(sv), one(gv), rounded=False)
        x = np.empty(2 * H)
        x[0::2], x[1::2] = q[0, :, 0], qd[0, :, 0]
        return x

    m = run(np.zeros((H - 1, 2)))
    A = np.stack([run(np.eye(2 * (H - 1))[i].reshape(H - 1, 2)) - m for i in range(2 * (H - 1))], 1)
    F, mean, cov = gs.dense_conditioning(H, dt, sigma, pin_vel, start, goal, sv, gv)
    got = (A @ A.T)[np.ix_(F, F)]
    print(f"pin_vel={pin_vel}: covariance off by {np.abs(got - cov).max() / np.abs(cov).max():.2e} of its largest entry, "
          f"mean by {np.abs(m[F] - mean).max():.2e}")
    assert np.abs(got - cov).max() <= 1e-9 * np.abs(cov).max()
    assert np.abs(m[F] - mean).max() <= 1e-9 * max(1.0, np.abs(mean).max())
    # the pinned components are the given values, and no noise reaches them
    pinned = [i for i in range(2 * H) if i not in F]
    assert len(pinned) == (4 if pin_vel else 2) and np.abs(A[pinned]).max() == 0.0


def test_without_noise_the_free_velocity_draw_is_the_straight_line():
    rng = np.random.default_rng(3)
    for H in (2, 3, 9, 64):
        P, K, D = 3, 2, 4
        st, go = rng.standard_normal((P, D)), rng.standard_normal((P, D))
        dt = 5.0 / 64
        q, qd, _, _ = gs.sample64(st, go, np.zeros((P * K, H - 1, D, 2)), dt, 2.0, K, rounded=False)
        s = np.linspace(0.0, 1.0, H).reshape(1, H, 1)
        line = np.repeat(st, K, 0)[:, None] + s * np.repeat(go - st, K, 0)[:, None]
        vel = np.repeat((go - st) / ((H - 1) * float(np.float32(dt))), K, 0)[:, None] * np.ones((1, H, 1))
        assert np.abs(q - line).max() <= 1e-14 * 8 and np.abs(qd - vel).max() <= 1e-12


def test_a_sequential_fp32_walk_stays_well_inside_the_tolerance():
    """2000 random cases (one trajectory of one coordinate each; start, goal and the velocities unit normal), H in {2, 3, 64, 100,
    256}, both pin modes, both (dt, sigma) of the GPU tests: |sample32 - sample64| <= 0.16 tol(H) mag everywhere."""
    rng = np.random.default_rng(0)
    worst = 0.0
    for case in range(2000):
        H, pin = int(rng.choice([2, 3, 64, 100, 256])), bool(case & 1)
        dt, sigma = ((5.0 / 64, 2.0), (5.0 / 128, 0.1))[(case >> 1) & 1]
        st, go, sv, gv = (rng.standard_normal((1, 1)).astype(np.float32) for _ in range(4))
        eps = rng.standard_normal((1, H - 1, 1, 2)).astype(np.float32)
        q, qd, mq, mqd = gs.sample64(st, go, eps, dt, sigma, 1, pin, sv, gv)
        q32, qd32 = gs.sample32(st, go, eps, dt, sigma, 1, pin, sv, gv)
        for got, ref, mag in ((q32, q, mq), (qd32, qd, mqd)):
            assert (np.abs(got - ref)[mag == 0] == 0).all()
            worst = max(worst, float((np.abs(got - ref)[mag > 0] / (gs.tol(H) * mag[mag > 0])).max()))
    print(f"worst |fp32 walk - fp64| / (tol(H) mag) over 2000 cases: {worst:.3f}")
    assert worst <= 0.16


def test_the_select_reference_on_a_case_by_hand():
    s = np.array([3.0, 1.0, 1.0, NAN, -INF, 2.0, 0.0, -0.0, 5.0], np.float32)
    fr = np.array([1, 1, 1, 1, 0, 1, 1, 1, 0], np.uint8)
    best, bs, nf = gs.select_best_ref(s, fr, 3)
    assert best.tolist() == [1, 5, 6] and bs.tolist() == [1.0, 2.0, 0.0] and nf.tolist() == [3, 2, 2]
    best, bs, nf = gs.select_best_ref(s, np.zeros(9, np.uint8), 3)
    assert best.tolist() == [-1, -1, -1] and np.isinf(bs).all() and nf.tolist() == [0, 0, 0]


LDS_CAP = 64 * 1024
# lanes of a workgroup x 4 bytes x the elements a lane keeps (csrc/trk_gp_sample.hip: EMAX, LANES)
LDS_BYTES = {(4, 256): 4096, (8, 256): 8192, (8, 512): 16384, (8, 1024): 32768}


def test_the_kernels_compile_without_scratch_and_within_the_lds_cap():
    csrc = ROOT / "torch_robotics_amd" / "csrc"
    make = (csrc / "Makefile").read_text()
    assert re.search(r"^SRCS := .*\btrk_gp_sample\.hip\b", make, flags=re.M)
    hipcc = re.search(r"^HIPCC \?= (.*)$", make, flags=re.M).group(1).strip()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", make, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    with tempfile.TemporaryDirectory() as d:
        res = subprocess.run([hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "trk_gp_sample.hip", "-o",
                              str(Path(d) / "gp_sample_device.o")], cwd=csrc, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    seen = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", res.stderr)[1:]:
        name = block.split()[0]
        num = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))
        m = re.match(r"_ZN\d+_GLOBAL__N_1\d+k_gp_sampleILi(\d+)ELi(\d+)EEE", name)
        key = (int(m.group(1)), int(m.group(2))) if m else ("select" if "k_select_best" in name else None)
        if key is not None:
            seen[key] = (num("ScratchSize [bytes/lane]"), num("VGPRs"), num("LDS Size [bytes/block]"))
    assert sorted(seen, key=str) == sorted(list(LDS_BYTES) + ["select"], key=str), sorted(seen, key=str)
    for key, (scratch, vgprs, lds) in seen.items():
        print(f"{key}: {vgprs} VGPRs, {lds} B of LDS, {scratch} B of scratch")
        assert scratch == 0, key
        assert lds <= LDS_CAP and lds == (0 if key == "select" else LDS_BYTES[key]), (key, lds)
