"""What the FK edge tests share (test_device_math_cpu.py, test_fk_refs_cpu.py, test_gpu_fk_edges.py): the probe angles of the device
sin/cos and the stand-alone host program that evaluates trk_device.h's trk_sincos on them, the star robots whose matrices hold the
device's sin/cos unrounded, the rows on, next to and beyond every joint limit, the chain mask of a one-hot adjoint, and the
comparison functions -- plain numpy on results, so that the CPU tests can hand them seeded wrong answers.

A comparison function returns the offences it found (an empty list or array: none)."""
import re
import subprocess
from pathlib import Path

import numpy as np

from helpers import GRAD_ATOL, GRAD_RTOL, ROOT, grad_close

TOL_H = 2e-6                               # DESIGN section 2's bound on an fp32 pose entry, per max(1, largest |translation|)
SINCOS_BOUND = 3 * 2.0 ** -24              # three half-ulps of a result near 1
GOLDEN_SINCOS = ROOT / "tests" / "golden" / "sincos_host_bits.npz"
CSRC = ROOT / "torch_robotics_amd" / "csrc"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits_nz(a):
    """bit patterns with -0 folded onto +0"""
    b = bits(a).copy()
    b[b == 0x80000000] = 0
    return b


# ---------------------------------------------------------------------------------------------------------------------------
# device sin/cos: the probe angles and the host program
# ---------------------------------------------------------------------------------------------------------------------------
SINCOS_WORST = ["0x1.920decp+0", "0x1.97aa0cp+0", "0x1.2d9be2p+2", "0x1.edb134p+2", "0x1.1474bp+4", "0x1.de4ecp+9",
                "0x1.4ad7dep+11", "0x1.794a58p+12", "0x1.04e642p+13", "0x1.464544p+15", "0x1.a44c68p+15"]


def _ulps(x, steps):
    """the fp32 value `x` and its neighbours `steps` ulps away (x > 0 and far from the format's ends: its bit pattern +- steps)"""
    b = np.float32(x).view(np.uint32).astype(np.int64)
    return [np.uint32(b + s).view(np.float32) for s in steps]


def probe_angles():
    """The probe list of the device sin/cos, fp32 (n,): zeros, the smallest subnormal and normal, powers of two; fp32(k pi / 2) with
    its neighbours up to 2 ulp away for k = 1..64, 1000, 10 000, 63 661 (where one of sin, cos is all rounding error of the
    reduction); the fp32 values nearest (m + 1/2) pi with their neighbours -- the ties of k = rint(x / pi) --; the worst cases of the
    exhaustive host sweep; 1024 seeded log-uniform values in [1e-3, 1e5].  Every value with both signs, each bit pattern once."""
    pos = [np.float32(0.0), np.uint32(1).view(np.float32), np.float32(2.0 ** -126)] + [np.float32(2.0 ** -k) for k in range(1, 41)]
    for k in list(range(1, 65)) + [1000, 10000, 63661]:
        pos += _ulps(np.float32(k * np.pi / 2), (0, -1, 1, -2, 2))
    for m in list(range(9)) + [100, 1000, 30000]:
        pos += _ulps(np.float32((m + 0.5) * np.pi), (0, -1, 1))
    pos += [np.float32(float.fromhex(h)) for h in SINCOS_WORST]
    rng = np.random.default_rng(20240)
    pos += list(np.exp(rng.uniform(np.log(1e-3), np.log(1e5), 1024)).astype(np.float32))
    pos = np.asarray(pos, np.float32)
    both = np.concatenate([pos, -pos])
    _, first = np.unique(bits(both), return_index=True)
    return both[np.sort(first)]


SINCOS_PROGRAM = r"""
// host side of trk_sincos (trk_device.h) against fp64 libm; no HIP call is made
#include "trk_device.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
static float f_of(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
static uint32_t b_of(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
static uint32_t nz(uint32_t b) { return b == 0x80000000u ? 0u : b; }
struct Stat { double es = 0, ec = 0; uint32_t xs = 0, xc = 0; long n = 0, asym = 0; };
static void visit(Stat& st, uint32_t xb) {
    const float x = f_of(xb);
    float s, c, sm, cm;
    trk_sincos(x, &s, &c);
    trk_sincos(-x, &sm, &cm);
    if (nz(b_of(sm)) != nz(b_of(-s)) || nz(b_of(cm)) != nz(b_of(c))) ++st.asym;
    const double es = std::fabs((double)s - std::sin((double)x)), ec = std::fabs((double)c - std::cos((double)x));
    if (es > st.es) { st.es = es; st.xs = xb; }
    if (ec > st.ec) { st.ec = ec; st.xc = xb; }
    ++st.n;
}
static void report(const char* name, const Stat& st) {
    std::printf("%s n %ld max_sin %.9e at %a max_cos %.9e at %a asym %ld\n", name, st.n, st.es, (double)f_of(st.xs), st.ec,
                (double)f_of(st.xc), st.asym);
}
int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "probe")) {          // file of fp32 bit patterns -> file of (x, sin, cos) bit patterns
        std::FILE* in = std::fopen(argv[2], "rb");
        std::FILE* out = std::fopen(argv[3], "wb");
        if (!in || !out) return 2;
        Stat st;
        uint32_t xb;
        while (std::fread(&xb, 4, 1, in) == 1) {
            float s, c;
            trk_sincos(f_of(xb), &s, &c);
            const uint32_t rec[3] = {xb, b_of(s), b_of(c)};
            std::fwrite(rec, 4, 3, out);
            visit(st, xb);
        }
        std::fclose(in); std::fclose(out);
        report("probe", st);
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
        Stat a, b;
        for (uint32_t xb = b_of(2.0f); xb < b_of(8.0f); ++xb) visit(a, xb);            // every fp32 in [2, 8)
        for (uint32_t xb = 0; xb <= b_of(1e5f); xb += 61) visit(b, xb);                // every 61st fp32 in [0, 1e5]
        report("dense_2_8", a);
        report("stride61_0_1e5", b);
        return 0;
    }
    return 2;
}
"""


def makefile_hipcc():
    return re.search(r"^HIPCC \?= (.*)$", (CSRC / "Makefile").read_text(), flags=re.M).group(1).strip()


def build_sincos_program(workdir):
    """Compile SINCOS_PROGRAM with the Makefile's compiler driver (host code is what runs; -ffp-contract=off as in the library's build,
    so the result rests on the header's explicit fmaf calls alone) -> path of the executable."""
    workdir = Path(workdir)
    src, exe = workdir / "sincos_host.hip", workdir / "sincos_host"
    src.write_text(SINCOS_PROGRAM)
    subprocess.run([makefile_hipcc(), "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{CSRC}", str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    return exe


def parse_report(text):
    """{set name: dict(n, max_sin, at_sin, max_cos, at_cos, asym)} of the program's report lines"""
    out = {}
    for line in text.splitlines():
        m = re.match(r"(\w+) n (\d+) max_sin (\S+) at (\S+) max_cos (\S+) at (\S+) asym (\d+)$", line.strip())
        if m:
            out[m.group(1)] = dict(n=int(m.group(2)), max_sin=float(m.group(3)), at_sin=m.group(4), max_cos=float(m.group(5)),
                                   at_cos=m.group(6), asym=int(m.group(7)))
    return out


def run_sincos_probe(exe, x, workdir):
    """the host trk_sincos of the fp32 values x -> (sin bits, cos bits, report)"""
    workdir = Path(workdir)
    bits(x).tofile(workdir / "probe_in.bin")
    res = subprocess.run([str(exe), "probe", str(workdir / "probe_in.bin"), str(workdir / "probe_out.bin")], check=True,
                         capture_output=True, text=True)
    rec = np.fromfile(workdir / "probe_out.bin", np.uint32).reshape(-1, 3)
    assert (rec[:, 0] == bits(x)).all()
    return rec[:, 1].copy(), rec[:, 2].copy(), parse_report(res.stdout)["probe"]


def sincos_bit_faults(got_s, got_c, want_s_bits, want_c_bits):
    """rows where a sine or cosine (fp32 values) is not the recorded bit pattern, +0 and -0 taken as equal"""
    ws, wc = np.asarray(want_s_bits, np.uint32).copy(), np.asarray(want_c_bits, np.uint32).copy()
    ws[ws == 0x80000000] = 0
    wc[wc == 0x80000000] = 0
    return np.flatnonzero((bits_nz(got_s) != ws) | (bits_nz(got_c) != wc))


def sincos_error_faults(x, s, c, bound=SINCOS_BOUND):
    """rows where sin or cos (fp32 values) of the fp32 angles x is further than `bound` from fp64 libm"""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    es = np.abs(np.asarray(s, np.float32).astype(np.float64) - np.sin(x64))
    ec = np.abs(np.asarray(c, np.float32).astype(np.float64) - np.cos(x64))
    return np.flatnonzero((es > bound) | (ec > bound))


# ---------------------------------------------------------------------------------------------------------------------------
# star robots: five continuous joints on the root, identity origins
# ---------------------------------------------------------------------------------------------------------------------------
STAR_AXES = {"z": ["0 0 1"] * 5, "mixed": ["0 0 1", "0 0 -1", "1 0 0", "0 1 0", "0 -1 0"]}


def write_star_urdf(path, axes):
    text = ['<?xml version="1.0"?>', '<robot name="star">', '  <link name="root"/>'] + [f'  <link name="l{i}"/>' for i in range(len(axes))]
    for i, ax in enumerate(axes):
        text += [f'  <joint name="j{i}" type="continuous">', f'    <parent link="root"/><child link="l{i}"/>',
                 '    <origin xyz="0 0 0" rpy="0 0 0"/>', f'    <axis xyz="{ax}"/>', "  </joint>"]
    Path(path).write_text("\n".join(text + ["</robot>"]))


def star_rows(x, n_dofs):
    """q (n, D): row i holds x[i], x[i + 1], ... cyclically, so every DOF sees every angle"""
    x = np.asarray(x, np.float32)
    idx = (np.arange(len(x))[:, None] + np.arange(n_dofs)[None, :]) % len(x)
    return x[idx], idx


def star_expected(model, s, c):
    """H (n, L, 4, 4) fp32 of a star robot whose link j turns by the angle with sine s[:, dof] and cosine c[:, dof] (of rot_sign * q,
    what joint_compose hands to trk_sincos): Rz = [c -s 0; s c 0; 0 0 1], Rx = [1 0 0; 0 c -s; 0 s c], Ry = [c 0 s; 0 1 0; -s 0 c]."""
    n = len(s)
    H = np.zeros((n, model.n_links, 4, 4), np.float32)
    H[:, :, np.arange(4), np.arange(4)] = 1.0
    for j in range(1, model.n_links):
        d, ax = int(model.dof_idx[j]), int(model.rot_axis[j])
        a, b = [(1, 2), (2, 0), (0, 1)][ax]
        H[:, j, a, a] = c[:, d]; H[:, j, b, b] = c[:, d]
        H[:, j, b, a] = s[:, d]; H[:, j, a, b] = -s[:, d]
    return H


def star_angles(model, q):
    """the angle joint_compose hands to trk_sincos per DOF: rot_sign * q (n, D) fp32, exact"""
    sign = np.ones(model.n_dofs, np.float32)
    for j in range(1, model.n_links):
        if int(model.dof_idx[j]) >= 0:
            sign[int(model.dof_idx[j])] = np.float32(model.rot_sign[j])
    return (np.asarray(q, np.float32) * sign[None, :]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# trees: leaves, chains, seeded q inside the limits
# ---------------------------------------------------------------------------------------------------------------------------
def leaf_links(model):
    par = np.asarray(model.parent, np.int64)
    return [i for i in range(model.n_links) if not (par == i).any()]


def onehot_links(model, cap=32):
    """the links that carry a one-hot adjoint: every leaf, the rest interior links in file order, `cap` at the most"""
    leaves = leaf_links(model)
    rest = [i for i in range(model.n_links) if i not in leaves]
    return (leaves + rest)[:cap]


def chain_dofs(model):
    """bool (L, D): DOF d belongs to a joint on the path from the root to link i, built from model.parent alone"""
    out = np.zeros((model.n_links, model.n_dofs), bool)
    for i in range(model.n_links):
        j = i
        while j >= 0 and int(model.parent[j]) >= 0:
            if int(model.dof_idx[j]) >= 0:
                out[i, int(model.dof_idx[j])] = True
            j = int(model.parent[j])
    return out


def dof_joints(model):
    """per DOF: (link index of its joint, clamped by the stateless walk?, lower, upper as fp32)"""
    out = [None] * model.n_dofs
    for j in range(1, model.n_links):
        d = int(model.dof_idx[j])
        if d >= 0:
            out[d] = (j, bool(model.clamp[j]), np.float32(model.lower[j]), np.float32(model.upper[j]))
    return out


def inside_q(model, n, seed, free=3.0, span=None):
    """q (n, D) fp32: clamped joints uniform over the middle 80 % of their limits (`span`: at most that far from the middle), the
    others uniform in +-free"""
    rng = np.random.default_rng(seed)
    q = np.empty((n, model.n_dofs), np.float32)
    for d, (j, clamped, lo, hi) in enumerate(dof_joints(model)):
        if clamped:
            mid, half = 0.5 * (float(lo) + float(hi)), 0.4 * (float(hi) - float(lo))
            half = half if span is None else min(half, span)
            q[:, d] = rng.uniform(mid - half, mid + half, n)
            assert (q[:, d] > lo).all() and (q[:, d] < hi).all()
        else:
            q[:, d] = rng.uniform(-free, free, n)
    return q


class LimitRows:
    """Rows that probe the joint limits.  For every DOF d the stateless walk clamps: q[d] = lower, upper, one ulp outside and inside
    each, lower - 1, upper + 1, and -0.0 where a limit is zero (+0.0 is that limit's row) -- at most 9 rows per DOF --; the other DOFs at seeded values strictly inside their limits (one
    draw per d).  For every DOF it does not clamp (continuous joints): +-1, +-pi, +-10, where the gradient passes everywhere.
    q (n, D) fp32; dof (n,); passes (n,): the reference's decision, lower <= q <= upper; twin (n,): for a row outside a limit the row
    with q[d] ON that limit, -1 elsewhere; kind (n,) names."""

    def __init__(self, model, seed):
        base = inside_q(model, model.n_dofs, seed, free=2.0)
        up, dn = np.float32(np.inf), np.float32(-np.inf)
        q, dof, passes, twin, kind = [], [], [], [], []

        def add(d, v, k, tw=-1):
            row = base[d].copy()
            row[d] = np.float32(v)
            q.append(row); dof.append(d); kind.append(k); twin.append(tw)
            return len(q) - 1

        for d, (j, clamped, lo, hi) in enumerate(dof_joints(model)):
            if not clamped:
                for v in (1.0, -1.0, np.pi, -np.pi, 10.0, -10.0):
                    add(d, v, "free")
                continue
            assert lo < hi
            r_lo, r_hi = add(d, lo, "lower"), add(d, hi, "upper")
            add(d, np.nextafter(lo, dn), "below", r_lo); add(d, np.nextafter(hi, up), "above", r_hi)
            add(d, np.nextafter(lo, up), "in_lower"); add(d, np.nextafter(hi, dn), "in_upper")
            add(d, np.float32(lo - np.float32(1.0)), "far_below", r_lo); add(d, np.float32(hi + np.float32(1.0)), "far_above", r_hi)
            if lo == 0 or hi == 0:                       # +0.0 is the limit's own row
                add(d, np.float32(-0.0), "neg_zero")
        self.q = np.asarray(q, np.float32)
        self.dof, self.twin, self.kind = np.asarray(dof), np.asarray(twin), np.asarray(kind)
        self.passes = self.twin < 0
        lim = dof_joints(model)
        for r in range(len(self.q)):                     # the rows' own bookkeeping against the reference's rule
            j, clamped, lo, hi = lim[self.dof[r]]
            v = self.q[r, self.dof[r]]
            assert self.passes[r] == (not clamped or bool(lo <= v <= hi)), (r, self.kind[r])

    @property
    def outside(self):
        return np.flatnonzero(~self.passes)


def outside_pose_faults(rows, out):
    """Outside rows whose output (n, ...) fp32 is not, bit for bit, the output of the row ON the limit: the clamp hands the same
    arithmetic the same number."""
    out = np.ascontiguousarray(out, np.float32)
    b = out.view(np.uint32).reshape(len(out), -1)
    return [int(r) for r in rows.outside if (b[r] != b[rows.twin[r]]).any()]


def limit_gradient_faults(rows, gq, ref64, scale=1.0):
    """gq (n, D) fp32 of LimitRows against the fp64 oracle's ref64: on an outside row gq[d] is exactly zero and the other DOFs' entries
    are bit-equal to the at-limit row's; on every other row gq[d] is non-zero wherever the oracle's entry exceeds 1e-3 of the row's
    largest (the gradient passes ON the limit); the whole tensor is grad_close to the oracle."""
    gq = np.ascontiguousarray(gq, np.float32).reshape(ref64.shape)
    ref64 = np.asarray(ref64, np.float64)
    faults = []
    b = gq.view(np.uint32)
    for r in range(len(gq)):
        d = int(rows.dof[r])
        if not rows.passes[r]:
            if gq[r, d] != 0:
                faults.append((r, str(rows.kind[r]), "gradient survives outside the limit", float(gq[r, d])))
            others = np.arange(gq.shape[1]) != d
            if (b[r, others] != b[rows.twin[r], others]).any():
                faults.append((r, str(rows.kind[r]), "other DOFs differ from the at-limit row"))
        elif abs(ref64[r, d]) > 1e-3 * np.abs(ref64[r]).max() and gq[r, d] == 0:
            faults.append((r, str(rows.kind[r]), "gradient killed inside or on the limit", float(ref64[r, d])))
    if not grad_close(gq, ref64, scale=scale):
        bad = np.argwhere(np.abs(gq - ref64) > GRAD_RTOL * np.abs(ref64) + GRAD_ATOL * scale * np.abs(ref64).max())
        faults.append(("grad_close", [(int(r), int(d), str(rows.kind[r])) for r, d in bad[:8]]))
    return faults


def offchain_faults(gq, links, mask):
    """(row, dof) where row i's gradient is not exactly zero at a DOF off the chain of its link links[i] (mask: chain_dofs)"""
    gq = np.asarray(gq, np.float32)
    off = ~np.asarray(mask)[np.asarray(links)]
    return np.argwhere((gq != 0) & off)


def pose_tolerance_faults(got, ref64, scale):
    """entries of a pose / position output further than TOL_H * scale from the oracle"""
    return np.argwhere(np.abs(np.asarray(got, np.float64) - np.asarray(ref64, np.float64)) >= TOL_H * scale)


def dense_adjoints(n, n_links, n_points, seed):
    """seeded dense adjoints fp32: gH (n, L, 4, 4), gpos (n, L, 3), gpts (n, P, 3)"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, n_links, 4, 4)).astype(np.float32), rng.standard_normal((n, n_links, 3)).astype(np.float32),
            rng.standard_normal((n, n_points, 3)).astype(np.float32))


def gpos_as_gH(gpos):
    """a position adjoint (n, L, 3) as the matrix adjoint (n, L, 4, 4) fp64 the oracle's fk_backward takes"""
    gH = np.zeros(gpos.shape[:2] + (4, 4))
    gH[..., :3, 3] = gpos
    return gH


def limit_case(model, oracle, seed, point_set=None):
    """LimitRows of a model with dense seeded adjoints (a row outside a limit shares its at-limit row's) and the fp64 oracle's answers,
    computed once per robot: dict(rows, q, gH, gpos,
    gpts, pl, po, H64, P64, scale, g_H, g_pos, g_pts)"""
    rows = LimitRows(model, seed)
    q = rows.q
    pl, po = point_set if point_set is not None else small_point_set(model, seed + 1)
    gH, gpos, gpts = dense_adjoints(len(q), model.n_links, len(pl), seed + 2)
    for g in (gH, gpos, gpts):                           # an outside row carries the adjoint of its at-limit row: only q[d] differs
        g[rows.outside] = g[rows.twin[rows.outside]]
    q64 = q.astype(np.float64)
    H64 = oracle.fk(q64, "f64")
    return dict(rows=rows, q=q, gH=gH, gpos=gpos, gpts=gpts, pl=pl, po=po, H64=H64, P64=oracle.fk_points(pl, po, q64, "f64"),
                scale=max(1.0, float(np.abs(H64[..., :3, 3]).max())),
                g_H=oracle.fk_backward(q64, gH.astype(np.float64), "f64"), g_pos=oracle.fk_backward(q64, gpos_as_gH(gpos), "f64"),
                g_pts=oracle.fk_points_backward(pl, po, q64, gpts.astype(np.float64), "f64"))


def onehot_point_set(model, links):
    """two points on each of `links` -- its origin and a fixed offset --, columns in walk order -> (point_link, point_offset, per entry of
    `links` the two columns of its points)"""
    pos = {int(v): k for k, v in enumerate(model.order)}
    by_walk = sorted(links, key=lambda i: pos[int(i)])
    pl = np.repeat(np.asarray(by_walk, np.int32), 2)
    po = np.tile(np.asarray([[0.0, 0.0, 0.0], [0.05, -0.03, 0.07]], np.float32), (len(by_walk), 1))
    cols = [[2 * by_walk.index(i), 2 * by_walk.index(i) + 1] for i in links]
    return pl, po, cols


def onehot_case(model, oracle, seed, point_set=None):
    """One row per link of onehot_links, the adjoint on that link alone: dict(links, mask (L, D), q, gH, gpos, gpts, pl, po, scale, g_H,
    g_pos, g_pts) with the fp64 oracle's gradients; q seeded inside the limits (a mobile base anywhere in its range).  point_set: a
    (point_link, point_offset) that has points on every link, instead of onehot_point_set's."""
    links = onehot_links(model)
    n = len(links)
    q = inside_q(model, n, seed)
    if point_set is None:
        pl, po, cols = onehot_point_set(model, links)
    else:
        pl, po = point_set
        cols = [np.flatnonzero(np.asarray(pl) == i) for i in links]
        assert all(len(c) for c in cols)
    rng = np.random.default_rng(seed + 1)
    gH, gpos, gpts = np.zeros((n, model.n_links, 4, 4), np.float32), np.zeros((n, model.n_links, 3), np.float32), np.zeros((n, len(pl), 3), np.float32)
    for r, i in enumerate(links):
        gH[r, i] = rng.standard_normal((4, 4)).astype(np.float32)
        gpos[r, i] = rng.standard_normal(3).astype(np.float32)
        gpts[r, cols[r]] = rng.standard_normal((len(cols[r]), 3)).astype(np.float32)
    q64 = q.astype(np.float64)
    H64 = oracle.fk(q64, "f64")
    return dict(links=links, mask=chain_dofs(model), q=q, gH=gH, gpos=gpos, gpts=gpts, pl=pl, po=po,
                scale=max(1.0, float(np.abs(H64[..., :3, 3]).max())),
                g_H=oracle.fk_backward(q64, gH.astype(np.float64), "f64"), g_pos=oracle.fk_backward(q64, gpos_as_gH(gpos), "f64"),
                g_pts=oracle.fk_points_backward(pl, po, q64, gpts.astype(np.float64), "f64"))


def onehot_faults(case, gq, ref64):
    """a one-hot gradient (n, D): exact zeros off the chain, grad_close to the oracle (whose off-chain zeros are exact) on it"""
    faults = [("off-chain residue", int(r), int(d), float(np.asarray(gq)[r, d])) for r, d in offchain_faults(gq, case["links"], case["mask"])[:8]]
    if not grad_close(gq, ref64, scale=case["scale"]):
        faults.append(("grad_close",))
    return faults


def small_point_set(model, seed):
    """A small attached-point set, columns in walk order: every third link of the walk carries its origin (a zero offset) and two
    seeded points, the last link too.  -> (point_link int32 (P,), point_offset fp32 (P, 3))"""
    rng = np.random.default_rng(seed)
    order = [int(v) for v in model.order]
    pl, po = [], []
    for k, i in enumerate(order):
        if k % 3 == 1 or k == len(order) - 1:
            pl += [i, i, i]
            po += [(0.0, 0.0, 0.0)] + [tuple(v) for v in rng.uniform(-0.1, 0.1, (2, 3))]
    return np.asarray(pl, np.int32), np.asarray(po, np.float32)


if __name__ == "__main__":          # PYTHONPATH=. python tests/fk_helpers.py: record the host bits of the probe list (tests/golden/sincos_host_bits.npz)
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        xs = probe_angles()
        sb, cb, rep = run_sincos_probe(build_sincos_program(tmp), xs, tmp)
    np.savez_compressed(GOLDEN_SINCOS, x=bits(xs), sin=sb, cos=cb)
    print(f"{GOLDEN_SINCOS.name}: {len(xs)} angles, {rep}")
