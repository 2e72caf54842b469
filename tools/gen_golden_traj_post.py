"""Fixtures of trajectory post-processing, recorded from the reference on the CPU.

TEST INFRASTRUCTURE -- never imported by the product, and run only where the reference checkout exists.  It imports the reference
read-only (with the stand-in parser of oracle/refshim on the path) and writes tests/golden/traj_post.npz:

  spline/<k>/...   the reference's own smoothen_trajectory (scipy's clamped make_interp_spline) with float64 tensor_args on paths whose
                   values are exact in fp32: y [N, D] fp32, S, mode (0 zero, 1 average, 2 spline), dt, pos and vel [S, D] fp64.
                   N in {2, 3, 4, 17, 64}, S in {2, 3, 30, 64, 127}, D in {1, 3, 7}, the three velocity modes, and three kinds of
                   path (a random walk, a walk with an O(3) offset, a straight line) in a covering design: every value of every
                   factor several times, every (N, S) pair of the design once.
  var/<k>/...      the reference's compute_variance_waypoints on float64 inputs that are exact in fp32: x [K, H, D] fp32 and the
                   value (fp64): (K, H, D) in {(2,4,3), (8,16,7), (64,8,7), (300,4,2)}, a clustered set (32 particles spread 1e-3
                   around an O(1) mean; with it the reference's value on the fp32 input, which torch.cdist forms by the
                   |a|^2 + |b|^2 - 2 a.b route), and K = 1 (NaN).

The archive is written with a fixed time stamp, and left alone when it already holds exactly these arrays: a rerun is byte-identical.

    python tools/gen_golden_traj_post.py [reference checkout]
"""
import io
import os
import sys
import zipfile
from pathlib import Path

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parent.parent
REF = Path(sys.argv[1] if len(sys.argv) > 1 else REPO.parent / "reference")
sys.path.insert(0, str(REPO / "oracle" / "refshim"))
sys.path.insert(0, str(REF))

import numpy as np  # noqa: E402
import torch  # noqa: E402

GOLD = REPO / "tests" / "golden"
TA64 = dict(device="cpu", dtype=torch.float64)
NS, SS, DS = (2, 3, 4, 17, 64), (2, 3, 30, 64, 127), (1, 3, 7)
VAR_SHAPES = ((2, 4, 3), (8, 16, 7), (64, 8, 7), (300, 4, 2))


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp; the file is left alone when it already holds exactly these arrays."""
    arrays = {k: np.asanyarray(v) for k, v in arrays.items()}
    if path.exists():
        with np.load(path) as z:
            if list(z.files) == list(arrays) and all(z[k].dtype == v.dtype and z[k].shape == v.shape and
                                                       np.array_equal(z[k], v, equal_nan=v.dtype.kind == "f")
                                                       for k, v in arrays.items()):
                return False
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, v, allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    return True


class Positions:
    """the one thing compute_variance_waypoints asks of a robot"""
    @staticmethod
    def get_position(x):
        return x


def path(rng, kind, N, D):
    if kind == 0:                                                   # a random walk
        y = np.cumsum(0.3 * rng.standard_normal((N, D)), 0)
    elif kind == 1:                                                 # the same with an O(3) offset
        y = 3.0 + np.cumsum(0.3 * rng.standard_normal((N, D)), 0)
    else:                                                           # a straight line
        y = rng.standard_normal((1, D)) + np.linspace(0.0, 1.0, N)[:, None] * rng.standard_normal((1, D))
    return y.astype(np.float32)


def main():
    from torch_robotics.trajectory.metrics import compute_variance_waypoints
    from torch_robotics.trajectory.utils import smoothen_trajectory
    rng = np.random.default_rng(20260101)
    out = {}
    k = 0
    for a, N in enumerate(NS):
        for b, S in enumerate(SS):
            if (a + b) % 5 not in (0, 1, 3):
                continue
            D, mode, kind = DS[(a + 2 * b) % 3], (a + b + k) % 3, (2 * a + b + k // 3) % 3
            dt = (0.02, 0.1)[k % 2]
            y = path(rng, kind, N, D)
            pos, vel = smoothen_trajectory(y.astype(np.float64), n_support_points=S, dt=float(np.float32(dt)), set_average_velocity=mode == 1,
                                           zero_velocity=mode == 0, tensor_args=TA64)
            out[f"spline/{k}/y"] = y
            out[f"spline/{k}/meta"] = np.array([S, mode, kind], np.int32)
            out[f"spline/{k}/dt"] = np.float32(dt)
            out[f"spline/{k}/pos"] = pos.numpy()
            out[f"spline/{k}/vel"] = vel.numpy()
            k += 1
    out["spline/n"] = np.int32(k)
    k = 0
    for K, H, D in VAR_SHAPES + ((32, 4, 3), (1, 4, 3)):
        x = rng.standard_normal((K, H, D))
        if (K, H, D) == (32, 4, 3):                                 # clustered: spread 1e-3 around an O(1) mean
            x = rng.standard_normal((1, H, D)) + 1e-3 * x
        x = x.astype(np.float32)
        out[f"var/{k}/x"] = x
        out[f"var/{k}/value"] = np.float64(compute_variance_waypoints(torch.from_numpy(x).to(torch.float64), Positions))
        if (K, H, D) == (32, 4, 3):
            out[f"var/{k}/value_fp32_reference"] = np.float64(compute_variance_waypoints(torch.from_numpy(x), Positions))
            out["var/clustered"] = np.int32(k)
        k += 1
    out["var/n"] = np.int32(k)
    wrote = save_npz(GOLD / "traj_post.npz", out)
    print("traj_post:", int(out["spline/n"]), "spline cases,", k, "variance cases,", "written" if wrote else "unchanged",
          (GOLD / "traj_post.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
