"""Inputs, fp64 references and error bounds for the workspace, self-pair and end-effector terms at their hinges, ties and zeros
(tests/test_term_edges_refs_cpu.py checks them on the CPU, tests/test_gpu_term_edges.py holds the kernels to them).

Everything is built from dyadic numbers, so that the plane distances p - min, max - p and the pair separations are exact in fp32 and
an edge (a hinge at zero, a tie of two planes, a separation of exactly 0) is where it was put, bit for bit.

Error bounds, derived from the code (u32(v) = the fp32 ulp of |v|):

  Workspace, ws_cost_point (csrc/trk_device.h).  Per axis k it forms d_k = p_k - c_k, m_k = h_k - |d_k|, then m = min_k m_k and
  v = margin - m, with c = 0.5f * (min + max) and h = 0.5f * (max - min) rounded once on the host.  Five roundings per axis: c_k and
  h_k (their actual errors e_c, e_h are computed here: 0 for a box whose centre and half width are representable), d_k, m_k and v,
  each at most half an ulp of its own RESULT -- which is at most half an ulp of the largest magnitude among the coordinate, the two
  bounds and the margin --, and none where the exact result is representable.  (On a dyadic box c and h are exact, but p_k - c_k is
  not always: 0.125 + k * 2^-26 is a float, that minus 1 is not.  There the plane form p - min, which the booleans evaluate, is exact
  and the cost's hinge is up to u32(p_k - c_k) / 2 away from it.)  With e_k = e_c + e_h + u32(d_k) / 2 + u32(m_k) / 2 the minimum over the intervals m_k +- e_k lies in
  [min_k (m_k - e_k), min_k (m_k + e_k)] -- an axis that cannot be the minimum adds nothing --, so
      |v - v64| <= max(m - min_k (m_k - e_k), min_k (m_k + e_k) - m) + u32(v) / 2                                  (ws_bound)
  The sum over K links adds K roundings of at most half an ulp of the sum of the |terms| (row_sum_bound).

  Self pair, spec_self_pair (csrc/trk_spec_common.h) and fields_eval (csrc/trk_kernels.hip).  d = pa - pb per axis (half an ulp each,
  0 for the separations built here), n2 = fma(dx, dx, fma(dy, dy, dz * dz)): three roundings of at most 2^-24 n2, i.e. 1.5 * 2^-24 of
  the norm; the 1-ulp v_rsq_f32 (or v_sqrt_f32): 2^-23 of the norm; the multiply n2 * rsq: 2^-24 of the norm; margin - norm: half
  an ulp of the result:
      |v - v64| <= sum_k u32(d_k) / 2 + 4.5 * 2^-24 * norm + u32(v) / 2                                              (pair_bound)
  A squared distance below the smallest normal float counts as 0 (v_rsq_f32 reads a subnormal as zero; the guards compare with
  FLT_MIN): there the norm itself, at most 1.1e-19 m, is the error, and the gradient is 0.

A term whose fp64 hinge value lies within its bound of zero may come back on either side of the clamp; a workspace point whose
runner-up plane lies within twice the bound of the winner may come back with either plane's gradient (ws_candidates64).  Every
other row is decided."""
import numpy as np

from helpers import gold
from torch_robotics_amd.costmodel import CostModelSpec

OFFSETS = [(0.0, 0.0, 0.0), (1.0, 0.3, 0.2), (3.0, 1.0, 0.5), (10.0, 3.0, 2.0), (30.0, -20.0, 1.0)]     # test_gpu_edges.OFFSETS
FAR_OFFSET = (300.0, -250.5, 128.25)
LADDER_K = (-64, -16, -4, -2, -1, 0, 1, 2, 4, 16, 64)
PAIR_K = (-64, -4, -2, -1, 0, 1, 2, 4, 64)
TOL_C = 2e-6                                   # the project's cost tolerance: TOL_C * max(1, |cost|)
FLT_MIN = float(np.finfo(np.float32).tiny)
TINY = 2.0 ** -67                              # about 1e-20 m and a float: its square, 2^-134, is subnormal in fp32


def u32(v):
    """the fp32 ulp of |v| (fp64 array)"""
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def dyadic_offset(O):
    """an offset moved onto the 1/64 m grid: box bounds, parked points and ladders about it stay representable out to 2048 m"""
    return np.round(np.asarray(O, np.float64) * 64.0) / 64.0


def is_f32(x):
    x = np.asarray(x, np.float64)
    return x.astype(np.float32).astype(np.float64) == x


# ---------------------------------------------------------------------------------------------------------------------------
# workspace box
# ---------------------------------------------------------------------------------------------------------------------------
WS_HALF = np.array([1.0, 1.5, 1.75])                                               # three different sides
WS_MARGINS = np.array([0.125, 0.25, 0.1875, 0.375, 0.3125], np.float32)            # one per collision link of the Panda's template
WS_PARK = np.array([[0.25 + 0.0625 * l, 0.125, -0.0625] for l in range(5)])        # parked links: x is the nearest axis, 0.5 .. 0.75 m deep
WS_TIE_DEPTH = 0.0625                                                              # ties sit this far inside / outside the hinge


def ws_boxes():
    """[(name, lo (3,) fp32, hi (3,) fp32, dyadic)]: the box of three different sides about every offset (on the 1/64 m grid, so
    centre and half widths are exact in fp32) and one box of arbitrary fp32 bounds, whose centre and half widths round"""
    out = []
    for O in OFFSETS + [FAR_OFFSET]:
        c = dyadic_offset(O)
        lo, hi = c - WS_HALF, c + WS_HALF
        assert is_f32(lo).all() and is_f32(hi).all()
        out.append((f"O={tuple(float(v) for v in c)}", lo.astype(np.float32), hi.astype(np.float32), True))
    out.append(("rounded", np.array([2.1, -0.3, -0.7], np.float32), np.array([4.3, 2.3, 2.4], np.float32), False))
    return out


def ws_step(lo, hi):
    """the ladder step of a box: the coordinate's ulp, or the bounds' where centre or half width round (see ws_rows)"""
    lo64, hi64 = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    return "coordinate" if is_f32(0.5 * (lo64 + hi64)).all() and is_f32(0.5 * (hi64 - lo64)).all() else "bounds"


def ws_host_centre(lo, hi):
    """the host's h.ws_c, h.ws_h (csrc/trk_capi.hip): 0.5f * (min + max), 0.5f * (max - min) in fp32"""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    return np.float32(0.5) * (lo + hi), np.float32(0.5) * (hi - lo)


def ws_rows(lo, hi, margins=WS_MARGINS, seed=0, step="coordinate"):
    """The moving link's points for one box -> dict(p (n, 3) fp32, slot (n,) which collision link moves, kind (n,) one of 'ladder',
    'tie2', 'tie3', 'centre', 'zero', 'random', k (n,) the ladder rung, face (n,) 0..5 = [x-min, y-min, z-min, x-max, y-max, z-max]).
      ladder: per face and link, signed distance to the face = margin + k ulp of that coordinate (of the margin where the coordinate
              is the smaller of the two: the finest step that coordinate AND distance hold exactly), the other coordinates mid-box
              (step="bounds", for a box whose centre rounds: k ulp of the larger of the coordinate and the axis's two bounds);
      tie2:   two faces of different axes at the same distance (all 12 mixed pairs), WS_TIE_DEPTH inside and outside the hinge;
      tie3:   the eight corners likewise;
      centre: the centre of the shortest axis (its two faces tie), alone and with the other coordinates off-centre;
      zero:   -0.0 and +0.0 for p - c on the shortest axis (a box whose centre is 0 there);
      random: points in the box grown by 0.5 m."""
    lo64, hi64 = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    c, h = 0.5 * (lo64 + hi64), 0.5 * (hi64 - lo64)
    K = len(margins)
    P, S, KIND, KK, F = [], [], [], [], []

    def add(p, slot, kind, k=0, face=-1):
        P.append(np.asarray(p, np.float64).astype(np.float32)); S.append(slot); KIND.append(kind); KK.append(k); F.append(face)

    for face in range(6):
        a = face % 3
        for slot in range(K):
            mg = float(margins[slot])
            x0 = np.float32(lo64[a] + mg if face < 3 else hi64[a] - mg)
            assert x0 != 0                      # a coordinate of 0 has no ulp to climb by
            for k in LADDER_K:
                # further from the face = larger signed distance: +k moves inwards
                big = np.float32(max(abs(x0), mg) if step == "coordinate" else max(abs(x0), abs(lo64[a]), abs(hi64[a])))
                x = float(x0) + (k if face < 3 else -k) * float(np.spacing(np.abs(big)))
                p = c.copy(); p[a] = x
                add(p, slot, "ladder", k, face)
    n = 0
    for a, b in ((0, 1), (0, 2), (1, 2)):
        for sa in (-1, 1):
            for sb in (-1, 1):
                for side in (-1, 1):
                    slot = n % K; n += 1
                    s = float(margins[slot]) + side * WS_TIE_DEPTH
                    p = c.copy(); p[a] = c[a] + sa * (h[a] - s); p[b] = c[b] + sb * (h[b] - s)
                    add(p, slot, "tie2", face=(a if sa < 0 else a + 3))
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                for side in (-1, 1):
                    slot = n % K; n += 1
                    s = float(margins[slot]) + side * WS_TIE_DEPTH
                    add(c + np.array([sx, sy, sz]) * (h - s), slot, "tie3")
    a0 = int(np.argmin(h))
    for slot in range(K):
        add(c, slot, "centre")
        p = c + np.array([0.0, 0.25, -0.125]); p[a0] = c[a0]
        add(p, slot, "centre")
    if c[a0] == 0.0:
        for z in (-0.0, 0.0):
            for slot in range(K):
                p = c + np.array([0.0, 0.25, -0.125]); p[a0] = z
                add(p, slot, "zero")
    rng = np.random.default_rng(seed)
    for i in range(64):
        add(rng.uniform(lo64 - 0.5, hi64 + 0.5), i % K, "random")
    return dict(p=np.array(P, np.float32), slot=np.array(S), kind=np.array(KIND), k=np.array(KK), face=np.array(F))


def ws_positions(rows, lo, hi, obj_links, n_links=11):
    """(n, n_links, 3) fp32: the row's collision link at its point, the other collision links parked deep inside the box (WS_PARK,
    exact for a dyadic box), every other column at the box's centre"""
    lo64, hi64 = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    c = 0.5 * (lo64 + hi64)
    n = len(rows["p"])
    pos = np.tile(c.astype(np.float32), (n, n_links, 1))
    for l, li in enumerate(obj_links):
        pos[:, li, :] = (c + WS_PARK[l]).astype(np.float32)
    pos[np.arange(n), np.asarray(obj_links)[rows["slot"]], :] = rows["p"]
    return pos


def ws_planes64(p, lo, hi, margin):
    """margin - signed distance of the six planes [p - min ; max - p] in fp64: (n, 6)"""
    p = np.asarray(p, np.float32).astype(np.float64).reshape(-1, 3)
    lo64, hi64 = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    return np.asarray(margin, np.float64).reshape(-1, 1) - np.concatenate([p - lo64, hi64 - p], -1)


PLANE_ROWS = np.concatenate([-np.eye(3), np.eye(3)])           # d (margin - sd_k) / dp of the six planes


def ws_term64(p, lo, hi, margin, clamp):
    """the fp64 plane form (distance_fields.py:326-332), first maximum wins -> (value (n,), gradient (n, 3), hinge value (n,))"""
    v6 = ws_planes64(p, lo, hi, margin)
    k = np.argmax(v6, axis=1)
    v = v6[np.arange(len(v6)), k]
    g = PLANE_ROWS[k].copy()
    if clamp:
        g[~(v > 0)] = 0.0
        return np.maximum(v, 0.0), g, v
    return v.copy(), g, v


def ws_candidates64(p, lo, hi, margin, band):
    """The planes within `band` (n,) of the maximum of margin - sd_k: (mask (n, 6), their gradient rows (6, 3)).  At a tie every
    plane of the mask is a valid subgradient; the kernel's row must be one of them."""
    v6 = ws_planes64(p, lo, hi, margin)
    return v6 >= v6.max(axis=1, keepdims=True) - np.asarray(band, np.float64).reshape(-1, 1), PLANE_ROWS


def ws_rows_match_any(got, mask, scale=1.0):
    """rows of `got` (n, 3) that equal scale * the one-hot row of some plane of `mask` (n, 6), exactly"""
    got = np.asarray(got, np.float64).reshape(-1, 3)
    eq = (got[:, None, :] == scale * PLANE_ROWS[None]).all(-1)
    return (eq & mask).any(-1)


def ws_bound(p, lo, hi, margin):
    """|ws_cost_point - fp64 plane form| per point (n,), before the clamp -- the derivation of the module's docstring"""
    p = np.asarray(p, np.float32).astype(np.float64).reshape(-1, 3)
    lo64, hi64 = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    c32, h32 = (v.astype(np.float64) for v in ws_host_centre(lo, hi))
    e_c, e_h = np.abs(c32 - 0.5 * (lo64 + hi64)), np.abs(h32 - 0.5 * (hi64 - lo64))
    # a rounding whose exact result is representable is no rounding: on the dyadic boxes the whole chain is exact.  Once a step has
    # rounded, the later ones are counted at half an ulp whatever their exact value
    d = p - c32
    r1 = ~is_f32(d)
    m = h32 - np.abs(d)
    r2 = r1 | ~is_f32(m)
    per_axis = e_c + e_h + np.where(r1, 0.5 * u32(np.abs(d) + 0.5 * u32(d)), 0.0) + np.where(r2, 0.5 * u32(np.abs(m) + u32(m)), 0.0)
    mm = m.min(-1)                          # min_k over intervals m_k +- e_k: only the axes that can be the minimum count
    e = np.maximum(mm - (m - per_axis).min(-1), (m + per_axis).min(-1) - mm)
    v = np.asarray(margin, np.float64).reshape(-1) - mm
    return e + np.where((e > 0) | ~is_f32(v), 0.5 * u32(np.abs(v) + e), 0.0)


def row_sum_bound(terms, bounds):
    """a row's cost = the sum of its K terms (n, K), each within bounds (n, K): the terms' bounds plus K roundings of the running sum"""
    s = np.abs(terms).sum(-1) + bounds.sum(-1)
    return bounds.sum(-1) + terms.shape[1] * 0.5 * u32(s)


def ws_rule32(p, lo, hi, margin, clamp, scale=1.0):
    """ws_cost_point restated in numpy fp32, operation by operation: margin - min_k (h_k - |p_k - c_k|), the first arg-min axis wins,
    the sign is copysign(scale, p_k - c_k) -> (value (n,) fp32, gradient (n, 3) fp32)"""
    p = np.asarray(p, np.float32).reshape(-1, 3)
    c, h = ws_host_centre(lo, hi)
    d = p - c
    m3 = h - np.abs(d)
    m = np.minimum(np.minimum(m3[:, 0], m3[:, 1]), m3[:, 2])
    e0 = m3[:, 0] == m
    e1 = (m3[:, 1] == m) & ~e0
    e2 = ~(e0 | e1)
    v = np.asarray(margin, np.float32).reshape(-1) - m
    sc = np.full(len(p), scale, np.float32)
    if clamp:
        sc = np.where(v > 0, sc, np.float32(0.0))
    g = np.stack([np.where(e, np.copysign(sc, d[:, k]), np.float32(0.0)) for k, e in enumerate((e0, e1, e2))], -1).astype(np.float32)
    return (np.maximum(v, np.float32(0.0)) if clamp else v).astype(np.float32), g


def ws_hit32(pos, lo, hi, margin):
    """the booleans' plane form in fp32, exactly as collision_links / spec_collision_links evaluate it: any over links (n, K, 3) and
    the six planes of p - min < margin, max - p < margin; margin (K,) or a scalar"""
    pos = np.asarray(pos, np.float32)
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    mg = np.broadcast_to(np.asarray(margin, np.float32), pos.shape[:2])[..., None]
    return ((pos - lo < mg) | (hi - pos < mg)).any(axis=(1, 2))


def ws_spec(lo, hi, clamp, margins=WS_MARGINS):
    """the Panda template's collision links with one margin each, a workspace box and nothing else"""
    from torch_robotics_amd._abi import FIELD_WS
    spec = CostModelSpec(n_links_in=11)
    spec.obj_link_idx = gold("panda_robot")["obj_link_idxs"]
    spec.obj_link_margin = np.asarray(margins, np.float32)
    spec.ws_min, spec.ws_max = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    spec.clamp_fields = FIELD_WS if clamp else 0
    spec.validate()
    return spec


def ws_case(lo, hi, clamp):
    """One box, every row: (rows, positions (n, 11, 3), per-link fp64 terms (n, K), hinge values (n, K), bounds (n, K), the fp64
    gradient (n, 11, 3) with the oracle's first-plane rule)"""
    obj = gold("panda_robot")["obj_link_idxs"]
    rows = ws_rows(lo, hi, step=ws_step(lo, hi))
    pos = ws_positions(rows, lo, hi, obj)
    n, K = len(pos), len(obj)
    val, hinge, bnd = np.zeros((n, K)), np.zeros((n, K)), np.zeros((n, K))
    grad = np.zeros((n, 11, 3))
    for l, li in enumerate(obj):
        val[:, l], g, hinge[:, l] = ws_term64(pos[:, li], lo, hi, np.full(n, WS_MARGINS[l]), clamp)
        grad[:, li] += g
        bnd[:, l] = ws_bound(pos[:, li], lo, hi, np.full(n, WS_MARGINS[l]))
    return rows, pos, val, hinge, bnd, grad


# ---------------------------------------------------------------------------------------------------------------------------
# self pairs
# ---------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf restated: the product of two fp32 numbers is exact in fp64, the sum rounds to fp64 and then to fp32"""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def pair_norm32(pa, pb):
    """sqrtf(fma(dx, dx, fma(dy, dy, dz * dz))) of d = pa - pb in fp32: what both boolean kernels compare with the margin"""
    d = np.asarray(pa, np.float32) - np.asarray(pb, np.float32)
    return np.sqrt(fma32(d[..., 0], d[..., 0], fma32(d[..., 1], d[..., 1], d[..., 2] * d[..., 2])))


def grid_margins(n, lo=0.1, hi=0.3):
    """np.linspace(lo, hi, n) moved onto the 2^-12 m grid: distinct margins that a coordinate out to 2048 m can be off by exactly"""
    m = np.round(np.linspace(lo, hi, n) * 4096.0) / 4096.0
    assert len(np.unique(m)) == n
    return m.astype(np.float32)


def template_self_tables():
    """the Panda template's self-collision tables as the golden recorded them: (self_link_idx, self_pairs into it, pairs as links (P, 2))"""
    g = gold("panda_robot")
    idx, pairs = g["self_link_idxs"].astype(np.int32), g["self_pairs"].astype(np.int32)
    return idx, pairs, idx[pairs]


# a free table for the table-driven kernel: a pair and its reverse, a Pythagorean margin, a zero margin, and columns 9 and 10, which
# every row gives identical positions; column 8 is in no pair
FREE_LINKS = np.array([0, 1, 2, 3, 4, 5, 6, 7, 9, 10], np.int32)
FREE_PAIR_LINKS = np.array([[4, 1], [1, 4], [5, 2], [7, 3], [6, 0], [9, 10]], np.int32)
FREE_MARGINS = np.array([0.125, 0.25, 0.1875, 0.3125, 0.0, 0.0625], np.float32)
FREE_COINCIDENT = 5                     # the pair of columns 9 and 10


def self_spec(link_idx, pairs, margins, clamp):
    from torch_robotics_amd._abi import FIELD_SELF
    spec = CostModelSpec(n_links_in=11)
    spec.self_link_idx = np.asarray(link_idx, np.int32)
    spec.self_pairs = np.asarray(pairs, np.int32)
    spec.self_margin = np.asarray(margins, np.float32)
    spec.clamp_fields = FIELD_SELF if clamp else 0
    spec.validate()
    return spec


def free_self_spec(clamp):
    where = {int(l): i for i, l in enumerate(FREE_LINKS)}
    return self_spec(FREE_LINKS, [[where[int(a)], where[int(b)]] for a, b in FREE_PAIR_LINKS], FREE_MARGINS, clamp)


def self_case(table):
    """(self_link_idx, self_pairs into it, pairs as link columns (P, 2), margins (P,), columns kept identical) of the two tables:
    'template' -- the Panda template's pairs, which the generated kernels bake, with distinct margins and one margin of 0 --, and
    'free' -- FREE_PAIR_LINKS, for the table-driven kernels only"""
    if table == "template":
        idx, pairs, pl = template_self_tables()
        mg = grid_margins(len(pairs))
        mg[0] = 0.0
        return idx, pairs, pl, mg, ()
    spec = free_self_spec(True)
    return spec.self_link_idx, spec.self_pairs, FREE_PAIR_LINKS, FREE_MARGINS, ((9, 10),)


def self_tested(pl, same):
    """the pairs that get rows of their own: all but the columns kept identical"""
    return [i for i in range(len(pl)) if tuple(int(v) for v in pl[i]) not in same]


def self_parked(O, n_links=11):
    """(n_links, 3) fp64: link j at O + (j % 4, j // 4, 0): every pair at least 1 m apart, z = O_z for all"""
    j = np.arange(n_links)
    return dyadic_offset(O) + np.stack([j % 4, j // 4, 0 * j], -1).astype(np.float64)


def self_rows(pair_links, margins, O, same=()):
    """Positions (n, 11, 3) fp32 for the pairs (P, 2) of link columns with `margins` (P,) about offset O, every other link parked.
    -> dict(pos, pair (n,), kind (n,) of 'ladder', 'zero', 'subnormal', 'pyth', k (n,), sep (n,) the fp64 separation built).
      ladder:    pair i at distance margin_i + k * step along z and along x, k in PAIR_K, moving a about b and b about a; step is the
                 larger of the margin's ulp and the moved coordinate's (the finest separation both ends can hold exactly);
      zero:      the two columns at the same point;
      subnormal: TINY (about 1e-20 m) apart (squared distance below the smallest normal float), where the coordinate is 0;
      pyth:      (0.1875, 0.25, 0) + k * step along x: distance 0.3125 exactly at k = 0.
    same: pairs of columns (a, b) whose positions are made identical in every row (b follows a)."""
    park = self_parked(O)
    rows, PI, KIND, KK, SEP = [], [], [], [], []

    def add(mover, anchor, sep, pi, kind, k=0):
        pos = park.copy()
        pos[mover] = pos[anchor] + np.asarray(sep, np.float64)
        rows.append(pos); PI.append(pi); KIND.append(kind); KK.append(k); SEP.append(float(np.linalg.norm(sep)))

    for pi, (a, b) in enumerate(np.asarray(pair_links)):
        mg = float(margins[pi])
        for mover, anchor in ((a, b), (b, a)):
            if mg > 0:
                for axis in (2, 0):
                    for sgn in (1.0, -1.0):
                        step = max(float(u32(mg)), float(u32(abs(park[anchor, axis]) + mg)))
                        for k in PAIR_K:
                            e = np.zeros(3); e[axis] = sgn * (mg + k * step)
                            add(mover, anchor, e, pi, "ladder", k)
                stepx = float(u32(abs(park[anchor, 0]) + 0.1875))
                for k in (-4, -1, 0, 1, 4):
                    add(mover, anchor, (0.1875 + k * stepx, 0.25, 0.0), pi, "pyth", k)
            add(mover, anchor, (0.0, 0.0, 0.0), pi, "zero")
            if park[anchor, 2] == 0.0:
                add(mover, anchor, (0.0, 0.0, TINY), pi, "subnormal")
    pos = np.array(rows)
    for a, b in same:
        pos[:, b, :] = pos[:, a, :]
    return dict(pos=pos.astype(np.float32), exact=is_f32(pos).all(), pair=np.array(PI), kind=np.array(KIND), k=np.array(KK), sep=np.array(SEP))


def pair_terms64(pos, pair_links, margins):
    """per pair in fp64: (hinge value margin - ||pa - pb|| (n, P), norm (n, P), d = pa - pb (n, P, 3))"""
    p = np.asarray(pos, np.float32).astype(np.float64)
    pl = np.asarray(pair_links)
    d = p[:, pl[:, 0], :] - p[:, pl[:, 1], :]
    nrm = np.linalg.norm(d, axis=-1)
    return np.asarray(margins, np.float32).astype(np.float64)[None] - nrm, nrm, d


def pair_bound(v, nrm, d):
    """|kernel's margin - norm - fp64| per pair -- the derivation of the module's docstring (the subtraction pa - pb is counted at
    half an ulp of its result per axis where that result is not exact)"""
    p32 = np.asarray(d, np.float64)
    e_d = np.where(is_f32(p32), 0.0, 0.5 * u32(p32)).sum(-1)
    e = e_d + 4.5 * 2.0 ** -24 * nrm + np.where(nrm * nrm < FLT_MIN, nrm, 0.0)       # a subnormal squared distance counts as 0
    return e + 0.5 * u32(np.abs(v) + e)


def pair_grad64(pos, pair_links, on):
    """the fp64 gradient (n, 11, 3) of the pairs that `on` (n, P) switches on: minus the unit vector of pa - pb on a, plus on b,
    nothing at distance 0"""
    p = np.asarray(pos, np.float32).astype(np.float64)
    pl = np.asarray(pair_links)
    d = p[:, pl[:, 0], :] - p[:, pl[:, 1], :]
    nrm = np.linalg.norm(d, axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = np.where(((nrm > 0) & on)[..., None], d / nrm[..., None], 0.0)
    g = np.zeros(p.shape, np.float64)
    for i, (a, b) in enumerate(pl):
        g[:, a, :] -= unit[:, i, :]
        g[:, b, :] += unit[:, i, :]
    return g


def self_cost64(pos, pair_links, margins, clamp):
    """the fp64 self-pair field (distance_fields.py:194-208): (cost (n,), gradient (n, 11, 3))"""
    v, nrm, d = pair_terms64(pos, pair_links, margins)
    on = (v > 0) if clamp else np.ones_like(v, bool)
    return np.where(on, v, 0.0).sum(-1), pair_grad64(pos, pair_links, on)


# ---------------------------------------------------------------------------------------------------------------------------
# end effector
# ---------------------------------------------------------------------------------------------------------------------------
EE_WEIGHTS = [(1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (0.0, 0.0), (2.0, 0.5)]
EE_NS = (1, 255, 256, 257)
EE_KINDS = ("on_target", "pos_equal", "rot_equal", "pi_x", "pi_y", "pi_z", "one_ulp", "subnormal")


def _quat_rot(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _pose(R, t):
    H = np.eye(4)
    H[:3, :3], H[:3, 3] = R, t
    return H.astype(np.float32)


EXACT_ROTS = [np.eye(3), np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([[0.0, 0, 1], [0, -1, 0], [1, 0, 0]]),
              np.array([[-1.0, 0, 0], [0, 0, 1], [0, 1, 0]])]


def ee_target(seed=0, exact_rot=False):
    """a target pose whose y coordinate is 0, so that a pose TINY from it exists in fp32.  exact_rot: a rotation with entries in
    {0, +-1}, whose trace against itself is 3 exactly in fp32 (a general fp32 rotation's is 3 within a few roundings)"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-0.8, 0.8, 3)
    t[1] = 0.0
    R = _quat_rot(rng.standard_normal(4))
    return _pose(EXACT_ROTS[seed % len(EXACT_ROTS)] if exact_rot else R, t)


def ee_rows(n, seed, per_sample, exact_rot=False):
    """Poses (n, 4, 4) fp32, their targets (n, 4, 4) fp32 (one shared target unless per_sample) and the kind of each row: the edge
    rows of EE_KINDS in turn at rows 0, 1, .. and again at the END of the batch (the last lanes of the last block), 'random' between.
    exact_rot: the shared target (per_sample: the target of every 'on_target' row) has an exact rotation, see ee_target."""
    rng = np.random.default_rng(seed)
    shared = ee_target(seed, exact_rot)
    H, T, kind = [], [], []
    edge_at = {i: EE_KINDS[i % len(EE_KINDS)] for i in range(min(n, 2 * len(EE_KINDS)))}
    for j in range(min(n, len(EE_KINDS))):
        edge_at[n - 1 - j] = EE_KINDS[j]
    for i in range(n):
        k = edge_at.get(i, "random")
        Ht = ee_target(1000 + seed * 7919 + i, exact_rot and k == "on_target") if per_sample else shared
        Rt, tt = Ht[:3, :3].astype(np.float64), Ht[:3, 3].astype(np.float64)
        R, t = _quat_rot(rng.standard_normal(4)), tt + rng.uniform(-0.5, 0.5, 3)
        if k == "on_target":
            R, t = Rt, tt
        elif k == "pos_equal":
            t = tt
        elif k == "rot_equal":
            R = Rt
        elif k in ("pi_x", "pi_y", "pi_z"):
            s = -np.ones(3); s["xyz".index(k[-1])] = 1.0
            R = Rt * s[None, :]                     # Rt diag(s): a turn by pi about that axis of the target frame, trace(R^T Rt) = -1
        elif k == "one_ulp":
            R, t = Rt, tt.copy()
            t[2] = float(np.nextafter(np.float32(tt[2]), np.float32(np.inf)))
        elif k == "subnormal":
            R, t = Rt, tt.copy()
            t[1] = TINY
        H.append(_pose(R, t)); T.append(Ht); kind.append(k)
    H, T = np.array(H, np.float32), np.array(T, np.float32)
    on = np.array([k in ("on_target", "pos_equal", "one_ulp", "subnormal", "rot_equal") for k in kind])
    # rows that share the target's rotation or translation do so bit for bit
    for i in np.flatnonzero(on):
        if kind[i] in ("on_target", "rot_equal", "one_ulp", "subnormal"):
            H[i, :3, :3] = T[i, :3, :3]
        if kind[i] in ("on_target", "pos_equal"):
            H[i, :3, 3] = T[i, :3, 3]
    return H, T, np.array(kind)


def ee_spec(w_pos, w_rot, square, target):
    spec = CostModelSpec(n_links_in=11)
    spec.ee_link, spec.ee_target = 10, np.asarray(target, np.float32).reshape(4, 4)
    spec.ee_w_pos, spec.ee_w_rot, spec.ee_square = float(w_pos), float(w_rot), bool(square)
    spec.validate()
    return spec


def ee_bound(H, T, w_pos, w_rot, square):
    """|ee_cost_eval - fp64| per sample: the trace is nine fmas of products of rotation entries (partial sums <= 3: 9 * 2^-23 with the
    half-ulp of each of them), 1 - (tr - 1) / 2 two more roundings of a number <= 2; the norm as for a self pair (4.5 * 2^-24 of it);
    two fmas into d and, with `square`, d * d: one rounding each"""
    H, T = np.asarray(H, np.float64), np.asarray(T, np.float64)
    tr = (H[:, :3, :3] * T[:, :3, :3]).sum((1, 2))
    nrm = np.linalg.norm(H[:, :3, 3] - T[:, :3, 3], axis=-1)
    dp = H[:, :3, 3] - T[:, :3, 3]
    e_d = np.where(is_f32(dp), 0.0, 0.5 * u32(dp)).sum(-1)
    d = (w_rot * (1 - (tr - 1) * 0.5) if w_rot > 0 else 0.0) + (w_pos * nrm if w_pos > 0 else 0.0)
    e = (w_rot * 11 * 2.0 ** -23 if w_rot > 0 else 0.0) + (w_pos * (e_d + 4.5 * 2.0 ** -24 * nrm + np.where(nrm * nrm < FLT_MIN, nrm, 0.0)) if w_pos > 0 else 0.0) + 2 * 2.0 ** -24 * np.abs(d)
    return (2 * np.abs(d) * e + e * e + 2.0 ** -24 * d * d) if square else e


# ---------------------------------------------------------------------------------------------------------------------------
# the same edges through the fused kernels: the positions are FK outputs, so the configurations are fixed and the box moves
# ---------------------------------------------------------------------------------------------------------------------------
TOL_H = 2e-6                                   # the project's bound on an fp32 position: TOL_H * max(1, |p|)
ROLLOUT_N = 65                                 # one full wavefront plus one row
ROLLOUT_DELTAS = (0.0, 1e-7, -1e-7, 1e-5, -1e-5, 1e-4, -1e-4, 1e-3, -1e-3)
ROLLOUT_WEIGHTS = ((0.0, 0.0, 1.0, 0.0), (1.0, 1.0, 1.0, 1.0))
# three collision links per robot, both arms of the dual Panda (not link2 of an arm: its origin does not move with q)
ROLLOUT_SLOTS = {"panda": (1, 2, 4), "dual_panda": (1, 6, 9)}
FAR = 8.0                                      # the faces that are not under test lie this far from the robot's base


def rollout_robot(ident, seed=17):
    """(KinModel, template, q (ROLLOUT_N, D) fp32 within 90 % of the joint ranges) of a robot with an ahead-of-time unit"""
    from torch_robotics_amd import codegen
    kin, tmpl = codegen.template_for(ident)
    mov = kin.dof_idx >= 0
    o = np.argsort(kin.dof_idx[mov])
    lo, hi = np.asarray(kin.lower[mov], np.float64)[o], np.asarray(kin.upper[mov], np.float64)[o]
    mid, half = 0.5 * (lo + hi), 0.45 * (hi - lo)
    q = np.random.default_rng(seed).uniform(mid - half, mid + half, (ROLLOUT_N, len(lo))).astype(np.float32)
    return kin, tmpl, q


def rollout_spec(kin, tmpl, lo, hi, ee_targets=None, ee_kw=None):
    """The template's whole objective -- its collision links with distinct margins on one sphere and in the workspace box [lo, hi]
    (clamped: the hinge is what moves with the box), its self pairs with distinct margins, its tracked links -- so that the generated
    unit serves every weight tuple"""
    from torch_robotics_amd._abi import FIELD_WS
    from torch_robotics_amd.costmodel import make_object, sphere_prims
    K = len(tmpl.obj_links)
    spec = CostModelSpec(n_links_in=kin.n_links)
    spec.obj_link_idx = np.asarray(tmpl.obj_links, np.int32)
    spec.obj_link_margin = np.linspace(0.08, 0.14, K).astype(np.float32)
    spec.objects = [make_object(sphere_prims(np.array([[0.45, 0.35, 0.8]]), np.float32(0.05)))]
    spec.ws_min, spec.ws_max = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    spec.clamp_fields = FIELD_WS
    sl = sorted({a for p in tmpl.self_pairs for a in p})
    spec.self_link_idx = np.asarray(sl, np.int32)
    spec.self_pairs = np.asarray([(sl.index(a), sl.index(b)) for a, b in tmpl.self_pairs], np.int32).reshape(-1, 2)
    spec.self_margin = np.linspace(0.04, 0.07, len(tmpl.self_pairs)).astype(np.float32)
    Ht = np.eye(4, dtype=np.float32)
    Ht[:3, 3] = (0.4, 0.2, 0.5)
    spec.ee_link, spec.ee_target = tmpl.ee_link, Ht if ee_targets is None else np.asarray(ee_targets[0], np.float32)
    if tmpl.ee2_link >= 0:
        Ht2 = Ht.copy()
        Ht2[:3, 3] = (0.4, -0.3, 0.5)
        spec.ee2_link, spec.ee2_target = tmpl.ee2_link, Ht2 if ee_targets is None else np.asarray(ee_targets[1], np.float32)
    for k, v in (ee_kw or {}).items():
        setattr(spec, k, v)
    spec.validate()
    return spec


def far_box(pos):
    """a box whose every face is FAR from the positions' centre (fp32)"""
    c = np.round(np.asarray(pos, np.float64).reshape(-1, 3).mean(0) * 16.0) / 16.0
    return (c - FAR).astype(np.float32), (c + FAR).astype(np.float32)


def rollout_boxes(pos, ident):
    """The boxes of one robot from its kernel's own fp32 positions (n, L, 3): for three collision links, a sample each, every one
    of the six faces and every delta of ROLLOUT_DELTAS, the box whose face lies at that link's coordinate -+ (margin + delta) -- the
    link's hinge value is -delta up to the face's own rounding -- and whose other faces stay metres away.
    -> [dict(lo, hi, sample, slot, face, delta)]"""
    from torch_robotics_amd import codegen
    _, tmpl = codegen.template_for(ident)
    K = len(tmpl.obj_links)
    margins = np.linspace(0.08, 0.14, K).astype(np.float32)
    lo0, hi0 = far_box(pos)
    out = []
    for j, slot in enumerate(ROLLOUT_SLOTS[ident]):
        for face in range(6):
            a = face % 3
            obj = np.asarray(tmpl.obj_links)
            for s in (np.arange(len(pos)) + 7 + 11 * j + 5 * face) % len(pos):
                # the first sample whose face no OTHER (sample, link) comes near for any delta: one in-band pair at the most
                p = float(pos[s, obj[slot], a])
                face_at = p - float(margins[slot]) if face < 3 else p + float(margins[slot])
                sd = (pos[:, obj, a].astype(np.float64) - face_at) * (1.0 if face < 3 else -1.0)
                v = margins[None].astype(np.float64) - sd
                v[s, slot] = np.inf
                if np.abs(v).min() > 2e-3:
                    break
            else:
                raise AssertionError("no sample has this face to itself")
            for delta in ROLLOUT_DELTAS:
                lo, hi = lo0.copy(), hi0.copy()
                if face < 3:
                    lo[a] = np.float32(p - (float(margins[slot]) + delta))
                else:
                    hi[a] = np.float32(p + (float(margins[slot]) + delta))
                out.append(dict(lo=lo, hi=hi, sample=s, slot=slot, face=face, delta=delta))
    return out


def rollout_hinges64(pos64, obj_links, margins, lo, hi):
    """per (sample, collision link): the fp64 hinge value margin - nearest plane distance (n, K), the band 2 TOL_H max(1, |p|) (n, K)
    and the plane distances (n, K, 6)"""
    p = np.asarray(pos64, np.float64)[:, np.asarray(obj_links), :]
    sd = np.concatenate([p - np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64) - p], -1)
    v = np.asarray(margins, np.float32).astype(np.float64)[None] - sd.min(-1)
    return v, 2 * TOL_H * np.maximum(1.0, np.abs(p).max(-1)), sd


def moved_face(box, amount):
    """the box with its face under test moved INWARDS by `amount` (outwards if negative)"""
    lo, hi = box["lo"].astype(np.float64), box["hi"].astype(np.float64)
    a = box["face"] % 3
    if box["face"] < 3:
        lo[a] += amount
    else:
        hi[a] -= amount
    return lo.astype(np.float32), hi.astype(np.float32)


def rollout_tied_pairs(pos64, obj_links, margins, lo, hi):
    """(n, K) bool: the (sample, link) pairs whose two nearest planes lie within twice the band of each other"""
    v, band, sd = rollout_hinges64(pos64, obj_links, margins, lo, hi)
    two = np.sort(sd, -1)[..., :2]
    return (two[..., 1] - two[..., 0]) <= 2 * band


def rollout_tie_box(pos, ident):
    """A box symmetric in x and y about one (sample, link) of the kernel's positions, half that link's margin away on either side (z
    far): four planes tie as far as fp32 bounds allow.  -> (box, the four boxes that move ONE of the tied faces in by four bands --
    that plane then wins by more than the band --, sample, slot)"""
    from torch_robotics_amd import codegen
    _, tmpl = codegen.template_for(ident)
    K = len(tmpl.obj_links)
    margins = np.linspace(0.08, 0.14, K).astype(np.float32)
    slot = ROLLOUT_SLOTS[ident][1]
    li = tmpl.obj_links[slot]
    lo0, hi0 = far_box(pos)
    for s in (np.arange(len(pos)) + 3) % len(pos):
        w = 0.5 * float(margins[slot])
        lo, hi = lo0.copy(), hi0.copy()
        for a in (0, 1):
            lo[a], hi[a] = np.float32(float(pos[s, li, a]) - w), np.float32(float(pos[s, li, a]) + w)
        tied = rollout_tied_pairs(pos.astype(np.float64), tmpl.obj_links, margins, lo, hi)
        v, band, _ = rollout_hinges64(pos.astype(np.float64), tmpl.obj_links, margins, lo, hi)
        if tied.sum() == 1 and tied[s, slot] and (np.abs(v) > 1e-3).all():
            break
    else:
        raise AssertionError("no sample gives a clean tie")
    box = dict(lo=lo, hi=hi, sample=int(s), slot=slot, face=-1, delta=0.0)
    amount = 4.0 * float(band[s, slot])
    cand = []
    for a in (0, 1):
        l2, h2 = lo.copy(), hi.copy(); l2[a] = np.float32(float(lo[a]) + amount); cand.append((l2, h2))
        l2, h2 = lo.copy(), hi.copy(); h2[a] = np.float32(float(hi[a]) - amount); cand.append((l2, h2))
    return box, cand, int(s), slot


COINCIDENT_PAIRS = np.array([[1, 2], [5, 6], [8, 9], [4, 1], [5, 0]], np.int32)        # the Panda's shared origins, two template pairs
COINCIDENT_MARGINS = np.array([0.0625, 0.09375, 0.125, 0.05, 0.07], np.float32)


def coincident_specs(clamp):
    """(the cost model with the five pairs, the one with the two template pairs alone, pairs as links, margins)"""
    def make(pl, mg):
        links = sorted({int(v) for v in pl.reshape(-1)})
        return self_spec(links, [[links.index(int(a)), links.index(int(b))] for a, b in pl], mg, clamp)
    return make(COINCIDENT_PAIRS, COINCIDENT_MARGINS), make(COINCIDENT_PAIRS[3:], COINCIDENT_MARGINS[3:]), COINCIDENT_PAIRS, COINCIDENT_MARGINS
