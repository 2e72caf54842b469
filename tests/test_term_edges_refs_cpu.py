"""The inputs and fp64 references of tests/test_gpu_term_edges.py, checked on the CPU: the builders produce the coverage the GPU test
demands, the dyadic constructions are exact, the references agree with oracle/ off ties, the oracle's choice at a tie is a member of
the candidate set, and ws_cost_point's rule restated in numpy fp32 stays within the derived bound and inside the candidate sets --
with a different plane than the oracle's at exact ties, which is accepted (both are subgradients)."""
import numpy as np
import pytest

import term_edges_helpers as T
from helpers import gold, model
from oracle.oracle import Oracle
from torch_robotics_amd._abi import FIELD_SELF, FIELD_WS

TIE_KINDS = ("tie2", "tie3", "centre", "zero")
BOXES = T.ws_boxes()


def test_offsets_are_the_edge_tests():
    import test_gpu_edges
    assert T.OFFSETS == test_gpu_edges.OFFSETS
    assert len(BOXES) == len(T.OFFSETS) + 2 and np.abs(np.asarray(T.FAR_OFFSET)).max() >= 300.0


@pytest.mark.parametrize("name,lo,hi,dyadic", BOXES, ids=[b[0] for b in BOXES])
def test_ws_rows_cover_faces_hinges_and_ties(name, lo, hi, dyadic):
    rows, pos, val, hinge, bnd, _ = T.ws_case(lo, hi, True)
    n = len(pos)
    r = np.arange(n)
    hv, hb = hinge[r, rows["slot"]], bnd[r, rows["slot"]]
    lad = rows["kind"] == "ladder"
    decided = np.abs(hv) > hb
    # three different sides, every face, either side of the hinge: at least 8 decided rows within 64 ulp of it
    assert len(set((np.asarray(hi, np.float64) - np.asarray(lo, np.float64)).tolist())) == 3
    for face in range(6):
        f = lad & (rows["face"] == face)
        assert (f & decided & (hv > 0)).sum() >= 8 and (f & decided & (hv < 0)).sum() >= 8, (name, face)
        assert (f & (rows["k"] == 0)).sum() == len(T.WS_MARGINS)
        # the ladder's nearest plane is the face it was built for, by a wide gap
        v6 = T.ws_planes64(rows["p"][f], lo, hi, T.WS_MARGINS[rows["slot"][f]])
        assert (np.argmax(v6, 1) == face).all() and (np.sort(v6, 1)[:, -1] - np.sort(v6, 1)[:, -2] > 0.1).all()
    for kind in ("tie2", "tie3", "centre") + (("zero",) if name == BOXES[0][0] else ()):
        assert (rows["kind"] == kind).sum() >= 8, (name, kind)
    assert (rows["kind"] == "tie2").sum() == 24
    # the rows that the either-side rule may serve are the lowest rungs (|k| <= 4: p - c rounds where p - min does not) and no
    # others; the rows with more than one candidate plane are constructed ties and no others
    in_band = ~decided
    assert (in_band <= (lad & (np.abs(rows["k"]) <= 4))).all(), (name, np.flatnonzero(in_band & ~(lad & (np.abs(rows["k"]) <= 4))))
    assert (lad & (rows["k"] == 0) <= in_band).all() or not dyadic
    mask, _ = T.ws_candidates64(rows["p"], lo, hi, T.WS_MARGINS[rows["slot"]], 2 * hb)
    multi = mask.sum(1) > 1
    assert (multi <= np.isin(rows["kind"], TIE_KINDS)).all(), name
    if dyadic:
        assert (lad & (rows["k"] == 0) <= (hv == 0)).all()
        assert multi[np.isin(rows["kind"], TIE_KINDS)].all()
        assert (mask[rows["kind"] == "tie2"].sum(1) == 2).all() and (mask[rows["kind"] == "tie3"].sum(1) == 3).all()
        # exact: the fp32 distance to the nearest plane equals the fp64 one, bit for bit, for every link of every constructed row (the
        # planes that do not decide may round: 2 m minus a 24-bit coordinate); centre and half width too
        built = rows["kind"] != "random"
        p32 = pos[built][:, gold("panda_robot")["obj_link_idxs"], :]
        d32 = np.concatenate([p32 - np.asarray(lo, np.float32), np.asarray(hi, np.float32) - p32], -1)
        d64 = np.concatenate([p32.astype(np.float64) - np.asarray(lo, np.float64), np.asarray(hi, np.float64) - p32.astype(np.float64)], -1)
        assert np.array_equal(d32.min(-1).astype(np.float64), d64.min(-1)), name
        c32, h32 = T.ws_host_centre(lo, hi)
        assert np.array_equal(c32.astype(np.float64), 0.5 * (np.asarray(lo, np.float64) + np.asarray(hi, np.float64)))
        assert np.array_equal(h32.astype(np.float64), 0.5 * (np.asarray(hi, np.float64) - np.asarray(lo, np.float64)))
    # the derived bound stays below the project's cost tolerance
    for clamp in (True, False):
        _, _, val, _, bnd, _ = T.ws_case(lo, hi, clamp)
        rb = T.row_sum_bound(val, bnd)
        assert (rb <= T.TOL_C * np.maximum(1.0, np.abs(val.sum(1)))).all(), (name, float(rb.max()))


@pytest.mark.parametrize("name,lo,hi,dyadic", BOXES, ids=[b[0] for b in BOXES])
@pytest.mark.parametrize("clamp", [True, False])
def test_ws_reference_agrees_with_the_oracle(name, lo, hi, dyadic, clamp):
    rows, pos, val, hinge, bnd, grad = T.ws_case(lo, hi, clamp)
    orc = Oracle(model("panda_arm_no_gripper"), T.ws_spec(lo, hi, clamp))
    c64, g64 = orc.cost_fields(FIELD_WS, pos.astype(np.float64), prec="f64")
    assert np.abs(c64 - val.sum(1)).max() <= 1e-12 * max(1.0, np.abs(c64).max())
    assert np.array_equal(g64, grad)                      # the same first-maximum rule: equal at ties too
    # at a tie the oracle's plane is one of the candidates -- and it is the FIRST of [x-min, y-min, z-min, x-max, y-max, z-max]
    obj = gold("panda_robot")["obj_link_idxs"]
    r = np.arange(len(pos))
    hb = bnd[r, rows["slot"]]
    mask, _ = T.ws_candidates64(rows["p"], lo, hi, T.WS_MARGINS[rows["slot"]], 2 * hb)
    live = (hinge[r, rows["slot"]] > hb) | (not clamp)
    got = g64[r, obj[rows["slot"]]]
    assert T.ws_rows_match_any(got[live], mask[live]).all()
    if dyadic:
        tie = np.isin(rows["kind"], TIE_KINDS) & live
        first = np.argmax(mask, 1)
        assert np.array_equal(got[tie], T.PLANE_ROWS[first[tie]])
    # the boolean of the oracle in fp32 is the fp32 plane form
    b32 = Oracle(model("panda_arm_no_gripper"), T.ws_spec(lo, hi, clamp)).collision_fields(FIELD_WS, pos, prec="f32")
    assert np.array_equal(b32, T.ws_hit32(pos[:, obj], lo, hi, T.WS_MARGINS))


@pytest.mark.parametrize("name,lo,hi,dyadic", BOXES, ids=[b[0] for b in BOXES])
def test_ws_kernel_rule_in_numpy(name, lo, hi, dyadic):
    """margin - min_k (h_k - |p_k - c_k|) in fp32: within the derived bound of the plane form, its gradient one of the candidate
    planes; at exact ties it picks another plane than the oracle (the first arg-min AXIS, the side by the sign of p - c)"""
    differs = 0
    for clamp in (True, False):
        rows, pos, val, hinge, bnd, grad = T.ws_case(lo, hi, clamp)
        r = np.arange(len(pos))
        mg = T.WS_MARGINS[rows["slot"]]
        v32, g32 = T.ws_rule32(rows["p"], lo, hi, mg, clamp)
        hv, hb = hinge[r, rows["slot"]], bnd[r, rows["slot"]]
        ref = val[r, rows["slot"]]
        err = np.abs(v32.astype(np.float64) - ref)
        assert (err <= hb).all(), (name, clamp, float(err.max()), float(hb[np.argmax(err)]))
        mask, _ = T.ws_candidates64(rows["p"], lo, hi, mg, 2 * hb)
        live = (hv > hb) | (not clamp)
        dead = clamp & (hv < -hb)
        assert T.ws_rows_match_any(g32[live], mask[live]).all(), name
        assert (g32[dead] == 0).all()
        gref = grad[r, gold("panda_robot")["obj_link_idxs"][rows["slot"]]]
        single = live & (mask.sum(1) == 1)
        assert np.array_equal(g32[single].astype(np.float64), gref[single])
        differs += int((g32[live].astype(np.float64) != gref[live]).any(-1).sum())
        if name == BOXES[0][0]:
            assert err[rows["kind"] != "random"].max() == 0.0      # about the origin the rewritten formula has nothing to round
    if dyadic:
        assert differs > 0                             # the kernel's tie rule is not the oracle's, and is accepted


def test_ws_issue_examples():
    """the two points of the issue in [-1, 1]^3: the oracle takes y-min / z-min, the kernel's rule x-max"""
    lo, hi = -np.ones(3, np.float32), np.ones(3, np.float32)
    p = np.array([[0.75, -0.75, 0.0], [0.875, 0.3, -0.875]], np.float32)
    _, g64, _ = T.ws_term64(p, lo, hi, np.full(2, 0.5), False)
    _, g32 = T.ws_rule32(p, lo, hi, np.full(2, 0.5, np.float32), False)
    assert np.array_equal(g64, [[0, -1, 0], [0, 0, -1]]) and np.array_equal(g32, [[1, 0, 0], [1, 0, 0]])
    mask, _ = T.ws_candidates64(p, lo, hi, np.full(2, 0.5), np.full(2, 1e-7))
    assert T.ws_rows_match_any(g64, mask).all() and T.ws_rows_match_any(g32, mask).all() and (mask.sum(1) == 2).all()
    wrong = np.array([[0, 0, 1.0], [0, 1.0, 0]])
    assert not T.ws_rows_match_any(wrong, mask).any()


SELF_CASES = [("template", O) for O in T.OFFSETS + [T.FAR_OFFSET]] + [("free", O) for O in T.OFFSETS + [T.FAR_OFFSET]]


@pytest.mark.parametrize("table,O", SELF_CASES, ids=[f"{t}-{O[0]:g}" for t, O in SELF_CASES])
def test_self_rows_and_reference(table, O):
    idx, pairs, pl, mg, same = T.self_case(table)
    tested = [i for i in range(len(pl)) if tuple(pl[i]) not in same]
    rows = T.self_rows(pl[tested], mg[tested], O, same=same)
    pos = rows["pos"]
    assert rows["exact"]                                  # every position representable: the separations are what was built
    v, nrm, d = T.pair_terms64(pos, pl, mg)
    b = T.pair_bound(v, nrm, d)
    pi = np.asarray(tested)[rows["pair"]]
    r = np.arange(len(pos))
    assert np.abs(nrm[r, pi] - rows["sep"]).max() <= 1e-15 * 4
    same_links = np.array([[set(map(int, pl[i])) == set(map(int, pl[j])) for j in range(len(pl))] for i in range(len(pl))])
    others = ~same_links[pi]                              # a pair and its reverse are at their edge together
    others[:, [i for i in range(len(pl)) if tuple(map(int, pl[i])) in same]] = False
    assert (v[others] < -0.25).all()                       # every parked pair is far behind the clamp
    hv, hb = v[r, pi], b[r, pi]
    lad = rows["kind"] == "ladder"
    for p in np.unique(pi):
        if mg[p] == 0:
            assert not (lad & (pi == p)).any() and ((rows["kind"] == "zero") & (pi == p)).any()
            continue
        m = lad & (pi == p)
        assert (m & (hv > hb)).sum() >= 8 and (m & (hv < -hb)).sum() >= 8 and (m & (rows["k"] == 0)).sum() >= 8
        assert (hv[m & (rows["k"] == 0)] == 0).all()
    in_band = np.abs(hv) <= hb
    # the either-side rule can serve the rungs within the 1-ulp rsq's reach (|k| <= 4) and a zero margin's zero distance, nothing else
    assert (in_band <= ((lad | (rows["kind"] == "pyth")) & (np.abs(rows["k"]) <= 4)) | ((rows["kind"] != "ladder") & (mg[pi] == 0))).all()
    assert (nrm[r, pi][rows["kind"] == "zero"] == 0).all()
    if tuple(O) == (0.0, 0.0, 0.0):
        sub = rows["kind"] == "subnormal"
        assert sub.sum() >= 2 and ((nrm[r, pi][sub] ** 2 < T.FLT_MIN) & (nrm[r, pi][sub] > 0)).all()
    # the fp64 reference and the oracle agree, clamped and not; the fp32 boolean is the oracle's fp32 one
    for clamp in (True, False):
        spec = T.self_spec(idx, pairs, mg, clamp)
        orc = Oracle(model("panda_arm_no_gripper"), spec)
        c64, g64 = orc.cost_fields(FIELD_SELF, pos.astype(np.float64), prec="f64")
        cr, gr = T.self_cost64(pos, pl, mg, clamp)
        assert np.abs(c64 - cr).max() <= 1e-13 * max(1.0, np.abs(cr).max()) and np.abs(g64 - gr).max() <= 1e-13
    hit32 = (T.pair_norm32(pos[:, pl[:, 0]], pos[:, pl[:, 1]]) < mg[None]).any(1)
    hit64 = (v > 0).any(1)
    decided = (np.abs(v) > b).all(1)
    assert np.array_equal(hit32[decided], hit64[decided]) and decided.sum() > 0.5 * len(pos)


@pytest.mark.parametrize("per_sample", [False, True])
def test_ee_rows(per_sample):
    for n in T.EE_NS:
        H, Tg, kind = T.ee_rows(n, 3, per_sample)
        assert H.shape == (n, 4, 4) and H.dtype == np.float32
        if n >= 255:
            for k in T.EE_KINDS:
                assert (kind == k).sum() >= 2 and kind[n - 1 - T.EE_KINDS.index(k)] == k
            assert (kind == "random").sum() >= 200
        assert len(T.ee_rows(n, 3, per_sample, exact_rot=True)[0]) == n
        i = np.flatnonzero(kind == "on_target")
        assert np.array_equal(H[i], Tg[i])
        R, Rt = H[:, :3, :3].astype(np.float64), Tg[:, :3, :3].astype(np.float64)
        tr = (R * Rt).sum((1, 2))
        assert np.abs(tr[np.isin(kind, ("pi_x", "pi_y", "pi_z"))] + 1.0).max(initial=0.0) < 1e-6
        dp = (H[:, :3, 3].astype(np.float64) - Tg[:, :3, 3].astype(np.float64))
        n2 = (dp * dp).sum(-1)
        assert ((n2[kind == "subnormal"] > 0) & (n2[kind == "subnormal"] < T.FLT_MIN)).all()
        assert ((np.abs(dp[kind == "one_ulp"]) > 0).sum(-1) == 1).all() and (n2[np.isin(kind, ("on_target", "pos_equal"))] == 0).all()
        for w_pos, w_rot in T.EE_WEIGHTS:
            for square in (True, False):
                orc = Oracle(model("panda_arm_no_gripper"), T.ee_spec(w_pos, w_rot, square, Tg[0]))
                c, g = orc.ee_cost(H.astype(np.float64), Tg.astype(np.float64) if per_sample else None, prec="f64")
                assert np.isfinite(c).all() and np.isfinite(g).all() and (g[:, 3, :] == 0).all()
                if square:
                    assert (np.abs(g[kind == "on_target"]) < 1e-6).all()
                assert (T.ee_bound(H, Tg, w_pos, w_rot, square) <= 5 * T.TOL_C * np.maximum(1.0, np.abs(c))).all()


@pytest.mark.parametrize("ident", ["panda", "dual_panda"])
def test_rollout_boxes_on_the_oracles_fp32_positions(ident):
    """part 3's boxes, built on the oracle's fp32 FK as a stand-in for the kernel's positions: every face and three links, at most
    one in-band pair per sample, exactly one for delta 0 and +-1e-7 and none from |delta| = 1e-5 on; the tie box ties one pair only"""
    kin, tmpl, q = T.rollout_robot(ident)
    assert q.shape == (T.ROLLOUT_N, kin.n_dofs)
    pos = Oracle(kin).fk(q, prec="f32")[:, :, :3, 3]
    pos64 = Oracle(kin).fk(q.astype(np.float64), prec="f64")[:, :, :3, 3]
    assert (np.abs(pos - pos64) <= T.TOL_H * np.maximum(1.0, np.abs(pos64))).all()
    boxes = T.rollout_boxes(pos, ident)
    spec = T.rollout_spec(kin, tmpl, *T.far_box(pos))
    assert len(boxes) == 3 * 6 * len(T.ROLLOUT_DELTAS) and len(np.unique(spec.obj_link_margin)) == len(tmpl.obj_links)
    assert {b["face"] for b in boxes} == set(range(6)) and len({b["slot"] for b in boxes}) == 3
    assert sorted({abs(d) for d in T.ROLLOUT_DELTAS}) == [0.0, 1e-7, 1e-5, 1e-4, 1e-3]
    for b in boxes:
        v, band, sd = T.rollout_hinges64(pos64, tmpl.obj_links, spec.obj_link_margin, b["lo"], b["hi"])
        inb = np.abs(v) <= band
        assert inb.sum(1).max() <= 1
        assert inb.sum() == (1 if abs(b["delta"]) < 1e-5 else 0) and (not inb.any() or inb[b["sample"], b["slot"]]), b
        # the other faces stay metres away
        other = np.ones(6, bool); other[b["face"]] = False
        assert sd[..., other].min() > 5.0
        # moving the face by twice the band decides the pair either way
        for sgn in (1.0, -1.0):
            v2, _, _ = T.rollout_hinges64(pos64, tmpl.obj_links, spec.obj_link_margin, *T.moved_face(b, sgn * 2 * band.max()))
            assert (np.abs(v2) > 0.9 * band)[inb].all() and (np.sign(v2[inb]) == sgn).all()
    box, cand, s, slot = T.rollout_tie_box(pos, ident)
    tied = T.rollout_tied_pairs(pos64, tmpl.obj_links, spec.obj_link_margin, box["lo"], box["hi"])
    assert tied.sum() == 1 and tied[s, slot] and len(cand) == 4
    for lo, hi in cand:
        assert not T.rollout_tied_pairs(pos64, tmpl.obj_links, spec.obj_link_margin, lo, hi).any()


def test_coincident_origins_in_the_oracle():
    """the Panda's links 1/2, 5/6, 8/9 share an origin in fp64 for every q: the pairs contribute their margin, no gradient"""
    kin, tmpl, q = T.rollout_robot("panda")
    for clamp in (False, True):
        spec, spec_rest, pl, mg = T.coincident_specs(clamp)
        pos, c, g = Oracle(kin, spec).rollout(q.astype(np.float64), (1, 0, 0, 0), "f64")
        _, c2, g2 = Oracle(kin, spec_rest).rollout(q.astype(np.float64), (1, 0, 0, 0), "f64")
        assert all(np.array_equal(pos[:, a], pos[:, b]) for a, b in pl[:3])
        assert np.abs(c - c2 - float(mg[:3].astype(np.float64).sum())).max() < 1e-12 and np.array_equal(g, g2)
