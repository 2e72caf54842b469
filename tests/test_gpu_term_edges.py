"""The workspace, self-pair and end-effector terms per sample at their hinges, ties and zeros, against the fp64 plane / norm / SE(3)
forms, on the generated kernels and on the table-driven ones (tests/term_edges_helpers.py builds the inputs and derives the bounds;
tests/test_term_edges_refs_cpu.py checks both on the CPU).

Every check is per sample and asserts how many rows it judged by which rule: a row is DECIDED unless its fp64 hinge value lies
within the derived bound of zero (then cost and gradient of either side of the clamp are accepted) or it was built on a tie of
planes (then any tied plane's gradient row is accepted).  The booleans are held bit for bit to their own fp32 expression.

Which family serves a call: `cm.enable_specialized` / `h.enable_specialized`; the cost models of the generated runs hold the template's
link and pair tables only (the units take no others).  `ops.last_dispatch()` is asserted for the rollouts -- the entries on given
positions do not record it.  The end-effector gradient with `square` and pose == target is exactly 0 only where the trace of R^T R
is exactly 3 in fp32 (rotation entries in {0, +-1}: asserted exactly); a general fp32 rotation's trace is 3 within its roundings and
the gradient is held to that bound instead."""
import numpy as np
import pytest
import torch

import term_edges_helpers as T
from helpers import GRAD_ATOL, GRAD_RTOL, gold, model
from oracle.oracle import Oracle
from torch_robotics_amd import ops
from torch_robotics_amd._abi import FIELD_SELF, FIELD_WS

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TIE_KINDS = ("tie2", "tie3", "centre", "zero")
BOXES = T.ws_boxes()
FAMILIES = (("generated", True), ("table-driven", False))


def _poison(shape):
    """NaNs where the next allocation of this shape will most likely land (the entries allocate their outputs themselves)"""
    t = torch.full(tuple(shape), float("nan"), device=DEV, dtype=torch.float32)
    torch.cuda.synchronize()
    del t


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("name,lo,hi,dyadic", BOXES, ids=[b[0] for b in BOXES])
def test_ws_cost_and_boolean_on_given_positions(name, lo, hi, dyadic):
    """ops.cost_fields / ops.collision_fields with FIELD_WS on a box of three different sides, about every offset: the six faces'
    ladders, the ties of two and three faces, the centre, signed zeros"""
    obj = gold("panda_robot")["obj_link_idxs"]
    K = len(obj)
    summary = {}
    for clamp in (True, False):
        rows, pos, val, hinge, bnd, g64 = T.ws_case(lo, hi, clamp)
        n = len(pos)
        r = np.arange(n)
        band = clamp & (np.abs(hinge) <= bnd)                           # (n, K): terms on the hinge, either side accepted
        assert (band.any(1) <= ((rows["kind"] == "ladder") & (np.abs(rows["k"]) <= 4))).all()
        assert band.sum(1).max() <= 1 and (not clamp or 0 < band.any(1).sum() <= 6 * K * 7)
        live = (hinge > bnd) | (not clamp)                                   # decided and in front of the clamp: a one-hot row
        dead = clamp & (hinge < -bnd)
        masks = np.stack([T.ws_candidates64(pos[:, li], lo, hi, np.full(n, T.WS_MARGINS[l]), 2 * bnd[:, l])[0] for l, li in enumerate(obj)], 1)
        multi = masks.sum(-1) > 1                                       # (n, K)
        built = np.isin(rows["kind"], TIE_KINDS)
        assert not multi[~built].any() and (not dyadic or multi[built, rows["slot"][built]].all())
        row_bound = T.row_sum_bound(val, bnd) + np.where(band, np.abs(hinge), 0.0).sum(1)
        assert (T.row_sum_bound(val, bnd) <= T.TOL_C * np.maximum(1.0, np.abs(val.sum(1)))).all()
        cm = ops.CostHandle(T.ws_spec(lo, hi, clamp), DEV)
        pt = torch.as_tensor(pos, device=DEV)
        for family, generated in FAMILIES:
            cm.enable_specialized(generated)
            what = f"{name} clamp={clamp} {family}"
            _poison(pos.shape)
            cost, g = ops.cost_fields(cm, FIELD_WS, pt, want_grad=True)
            hit = _np(ops.collision_fields(cm, FIELD_WS, pt))
            hit_o = _np(ops.collision_fields(cm, FIELD_WS, pt, margin=0.1875))
            torch.cuda.synchronize()
            cost, g = _np(cost).astype(np.float64), _np(g).astype(np.float64)
            assert np.isfinite(cost).all() and np.isfinite(g).all(), what
            # cost: the fp64 plane form within the derived bound, row by row
            err = np.abs(cost - val.sum(1))
            ulp = T.u32(np.maximum(np.abs(pos[:, obj]).max((1, 2)), max(np.abs(lo).max(), np.abs(hi).max())))
            assert (err <= row_bound).all(), (what, int(np.argmax(err - row_bound)), float(err.max()), rows["kind"][np.argmax(err - row_bound)])
            # gradient: columns that are no collision link get exactly 0; a decided link its one-hot row, exactly; a tie any tied
            # plane's; a term on the hinge either its row or 0
            other = np.setdiff1d(np.arange(11), obj)
            assert (g[:, other] == 0).all(), what
            judged = {"decided": 0, "tie": 0, "band": 0}
            for l, li in enumerate(obj):
                gl = g[:, li]
                one = live[:, l] & ~multi[:, l]
                assert np.array_equal(gl[one], g64[one][:, li]), (what, l)
                assert (gl[dead[:, l]] == 0).all(), (what, l)
                tie = live[:, l] & multi[:, l]
                assert T.ws_rows_match_any(gl[tie], masks[tie, l]).all(), (what, l, "a plane that is not tied")
                b = band[:, l]
                assert (T.ws_rows_match_any(gl[b], masks[b, l]) | (gl[b] == 0).all(-1)).all(), (what, l)
                judged["decided"] += int(one.sum() + dead[:, l].sum()); judged["tie"] += int(tie.sum()); judged["band"] += int(b.sum())
            assert judged["band"] == int(band.sum()) and sum(judged.values()) == n * K, (what, judged)
            assert judged["tie"] <= int(built.sum()) and judged["band"] <= int(((rows["kind"] == "ladder") & (np.abs(rows["k"]) <= 4)).sum())
            # booleans: bit-equal to the fp32 plane form, with the links' own margins and with an override
            assert np.array_equal(hit, T.ws_hit32(pos[:, obj], lo, hi, T.WS_MARGINS)), what
            assert np.array_equal(hit_o, T.ws_hit32(pos[:, obj], lo, hi, np.float32(0.1875))), what
            lad0 = (rows["kind"] == "ladder") & (rows["k"] == 0)
            if dyadic:                    # the rung on the margin is no hit, the rung below it is one
                assert hit[(rows["kind"] == "ladder") & (rows["k"] == -1)].all() and not hit[lad0].any(), what
            # hinge against boolean: they may disagree only where the fp64 hinge value lies within the bound
            gap = 0.0
            if clamp:
                dis = (cost > 0) != hit
                hv, hb = hinge[r, rows["slot"]], bnd[r, rows["slot"]]
                assert (np.abs(hv[dis]) <= hb[dis]).all(), (what, float(np.abs(hv[dis]).max()))
                gap = float(np.abs(hv[dis]).max(initial=0.0))
            summary[(clamp, family)] = dict(cost_err_ulp=float((err / ulp).max()), bound_ulp=float((row_bound / ulp).max()),
                                            hinge_vs_boolean=gap, **judged)
    for k, v in summary.items():
        print(f"workspace {name} clamp={k[0]} {k[1]}: worst cost error {v['cost_err_ulp']:.3g} ulp (bound {v['bound_ulp']:.3g}), hinge against "
              f"boolean {v['hinge_vs_boolean']:.3g} m, rows x links decided {v['decided']}, tie {v['tie']}, in band {v['band']}")


SELF_CASES = [(t, O) for t in ("template", "free") for O in T.OFFSETS + [T.FAR_OFFSET]]


@pytest.mark.parametrize("table,O", SELF_CASES, ids=[f"{t}-{O[0]:g}" for t, O in SELF_CASES])
def test_self_pairs_on_given_positions(table, O):
    """ops.cost_fields / ops.collision_fields with FIELD_SELF: distance ladders about every pair's margin in both orders, distance
    exactly 0 (also with a margin of 0), a subnormal squared distance, columns that no pair names"""
    idx, pairs, pl, mg, same = T.self_case(table)
    tested = T.self_tested(pl, same)
    rows = T.self_rows(pl[tested], mg[tested], O, same=same)
    pos = rows["pos"]
    n, P = len(pos), len(pl)
    r = np.arange(n)
    pi = np.asarray(tested)[rows["pair"]]
    v, nrm, d = T.pair_terms64(pos, pl, mg)
    b = T.pair_bound(v, nrm, d)
    sub = rows["kind"] == "subnormal"
    zero = rows["kind"] == "zero"
    untouched = np.setdiff1d(np.arange(11), np.unique(pl))
    assert len(untouched) >= 1 and (sub.sum() >= 2) == (tuple(O) == (0.0, 0.0, 0.0))
    pt = torch.as_tensor(pos, device=DEV)
    hit32 = lambda m: (T.pair_norm32(pos[:, pl[:, 0]], pos[:, pl[:, 1]]) < np.asarray(m, np.float32)).any(1)
    summary = {}
    for clamp in (True, False):
        band = clamp & (np.abs(v) <= b)                                  # (n, P)
        assert band.sum(1).max() <= 1
        ok_band = ((np.isin(rows["kind"], ("ladder", "pyth")) & (np.abs(rows["k"]) <= 4)) | (mg[pi] == 0) | sub)
        assert (band.any(1) <= ok_band).all()
        on = (v > b) | (not clamp)
        terms = np.where(on, v, 0.0)
        # a pair on its hinge, or one whose squared distance is subnormal (taken for 0: norm 0, no gradient), may be on or off
        tiny = (nrm > 0) & (nrm * nrm < T.FLT_MIN)
        on64 = (v > 0) | (not clamp)
        g_on, g_alt = T.pair_grad64(pos, pl, on64), T.pair_grad64(pos, pl, on64 & ~(band | tiny))
        row_bound = T.row_sum_bound(terms, np.where(on | band, b, 0.0)) + np.where(band, np.abs(v), 0.0).sum(1)
        spec = T.self_spec(idx, pairs, mg, clamp)
        cm = ops.CostHandle(spec, DEV)
        for family, generated in FAMILIES:
            if generated and table != "template":
                continue                                                  # the generated units take the template's tables only
            cm.enable_specialized(generated)
            what = f"{table} O={O} clamp={clamp} {family}"
            _poison(pos.shape)
            cost, g = ops.cost_fields(cm, FIELD_SELF, pt, want_grad=True)
            hit = _np(ops.collision_fields(cm, FIELD_SELF, pt))
            hit_o = _np(ops.collision_fields(cm, FIELD_SELF, pt, margin=0.1875))
            hit_0 = _np(ops.collision_fields(cm, FIELD_SELF, pt, margin=0.0))
            torch.cuda.synchronize()
            c32, g32 = _np(cost), _np(g)
            cost, g = c32.astype(np.float64), g32.astype(np.float64)
            # finite everywhere -- the subnormal squared distance included --, untouched columns exactly 0
            assert np.isfinite(cost).all() and np.isfinite(g).all(), (what, np.flatnonzero(~np.isfinite(cost))[:8], rows["kind"][~np.isfinite(cost)][:8])
            assert (g[:, untouched] == 0).all(), what
            err = np.abs(cost - np.where(on, v, 0.0).sum(1))
            assert (err <= row_bound).all(), (what, int(np.argmax(err - row_bound)), float(err.max()), rows["kind"][np.argmax(err - row_bound)])
            # gradient: the fp64 unit vectors element by element; a row with a pair on its hinge may have that pair on or off
            tol = GRAD_RTOL * np.abs(g_on) + GRAD_ATOL * max(1.0, float(np.abs(g_on).max()))
            close = (np.abs(g - g_on) <= tol).all((1, 2))
            dec = ~(band | tiny).any(1)
            assert close[dec].all(), (what, np.flatnonzero(dec & ~close)[:8])
            alt = (np.abs(g - g_alt) <= GRAD_RTOL * np.abs(g_alt) + GRAD_ATOL * max(1.0, float(np.abs(g_on).max()))).all((1, 2))
            assert (close | alt)[~dec].all(), (what, np.flatnonzero(~dec & ~close & ~alt)[:8], rows["kind"][~dec & ~close & ~alt][:8])
            assert (~dec).sum() <= ok_band.sum()
            # -g on a, +g on b, bit for bit, wherever the two columns serve this pair (and its reverse) alone: under the clamp
            if clamp:
                a_col, b_col = pl[pi, 0], pl[pi, 1]
                assert np.array_equal(g32[r, a_col], -g32[r, b_col]), what
                # distance exactly 0: the pair contributes its margin exactly and no gradient
                z = zero & ~band.any(1)
                expect = np.where((nrm == 0) & (v > 0), mg[None].astype(np.float64), 0.0).sum(1)
                assert np.array_equal(cost[z], expect[z]) and (g[z][:, np.unique(pl[pi[z]])] == 0).all(), what
            # booleans: bit-equal to sqrtf(fma(dx, dx, fma(dy, dy, dz * dz))) < margin in fp32
            assert np.array_equal(hit, hit32(mg[None])), what
            assert np.array_equal(hit_o, hit32(np.float32(0.1875))), what
            assert not hit_0.any(), what                                  # nothing is nearer than 0, a distance of exactly 0 included
            summary[(clamp, family)] = (float((err / np.maximum(T.u32(np.abs(v).max(1)), 2.0 ** -30)).max()), int(dec.sum()), int((~dec).sum()))
        # sizes: the first n rows alone give the same bits as the first n rows of the whole batch
        for family, generated in FAMILIES:
            if generated and table != "template":
                continue
            cm.enable_specialized(generated)
            full_c, full_g = ops.cost_fields(cm, FIELD_SELF, pt, want_grad=True)
            for m in (1, 63, 64, 65):
                _poison((m, 11, 3))
                c_m, g_m = ops.cost_fields(cm, FIELD_SELF, pt[:m].contiguous(), want_grad=True)
                assert torch.equal(c_m, full_c[:m]) and torch.equal(g_m, full_g[:m]), (table, O, family, m)
                assert torch.equal(ops.collision_fields(cm, FIELD_SELF, pt[:m].contiguous()), ops.collision_fields(cm, FIELD_SELF, pt)[:m])
    for k, (e, nd, nb) in summary.items():
        print(f"self pairs {table} O={O} clamp={k[0]} {k[1]}: worst cost error {e:.3g} ulp of the largest term, rows decided {nd}, in band {nb}")


@pytest.mark.parametrize("square", [True, False])
@pytest.mark.parametrize("w_pos,w_rot", T.EE_WEIGHTS)
def test_ee_cost_guards_shapes_and_targets(w_pos, w_rot, square):
    """ops.ee_cost (k_ee_cost): every guard of ee_cost_eval (w_rot > 0, w_pos > 0, n2 > 0, the hard zero of rs, square), one block and
    a ragged second one, contiguous and strided poses, shared / per-sample / the cost model's own target"""
    m = model("panda_arm_no_gripper")
    worst = 0.0
    for target_mode, exact_rot in (("shared", False), ("shared", True), ("per_sample", True), ("own", False)):
        for n in T.EE_NS:
            H, Tg, kind = T.ee_rows(n, 5, target_mode == "per_sample", exact_rot)
            spec = T.ee_spec(w_pos, w_rot, square, Tg[0])
            cm, orc = ops.CostHandle(spec, DEV), Oracle(m, spec)
            tgt = {"shared": torch.as_tensor(Tg[0], device=DEV), "per_sample": torch.as_tensor(Tg, device=DEV), "own": None}[target_mode]
            c64, g64 = orc.ee_cost(H.astype(np.float64), Tg.astype(np.float64) if target_mode == "per_sample" else None, prec="f64")
            bound = T.ee_bound(H, Tg, w_pos, w_rot, square)
            sub = kind == "subnormal"
            n2_zero = np.isin(kind, ("on_target", "pos_equal"))
            if n >= 255:
                assert all((kind == k).sum() >= 2 for k in T.EE_KINDS)
            for layout in ("contiguous", "strided"):
                what = f"w=({w_pos}, {w_rot}) square={square} target={target_mode} exact_rot={exact_rot} n={n} {layout}"
                if layout == "contiguous":
                    Hv = torch.as_tensor(H, device=DEV)
                else:
                    Hall = torch.randn((n, 3, 4, 4), device=DEV)
                    Hall[:, -1] = torch.as_tensor(H, device=DEV)
                    Hv = Hall[:, -1]
                    assert not Hv.is_contiguous() or n == 1
                _poison((n, 4, 4))
                cost, gH = ops.ee_cost(cm, Hv, tgt, want_grad=True)
                torch.cuda.synchronize()
                cost, gH = _np(cost).astype(np.float64), _np(gH).astype(np.float64)
                assert np.isfinite(cost).all() and np.isfinite(gH).all(), (what, kind[~np.isfinite(cost)])
                assert (gH[:, 3, :] == 0).all(), what                      # the bottom row comes back 0 from a poisoned buffer
                err = np.abs(cost - c64)
                assert (err <= bound).all(), (what, int(np.argmax(err - bound)), kind[np.argmax(err - bound)], float(err.max()))
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                tol = GRAD_RTOL * np.abs(g64) + GRAD_ATOL * np.maximum(1.0, np.abs(g64).max((1, 2), keepdims=True))
                close = np.abs(gH - g64) <= tol
                assert close[~sub].all(), (what, kind[~close.all((1, 2))])
                # the subnormal squared distance: the rotation block as usual, the translation gradient the unit vector or 0
                assert close[sub][:, :3, :3].all() and (close[sub][:, :3, 3].all(-1) | (gH[sub][:, :3, 3] == 0).all(-1)).all(), what
                if w_pos == 0:
                    assert (gH[:, :3, 3] == 0).all(), what
                if w_rot == 0:
                    assert (gH[:, :3, :3] == 0).all(), what
                assert (gH[n2_zero][:, :3, 3] == 0).all(), what
                on = kind == "on_target"
                if square and (exact_rot or w_rot == 0):
                    assert (gH[on] == 0).all(), what                       # d is exactly 0: trace 3, norm 0
                elif square:
                    assert (np.abs(gH[on]) <= 2 * w_rot * 11 * 2.0 ** -23 * 0.5 * w_rot).all(), what
            if w_pos == 0:
                # the position does not enter: any other translation -- a huge one included -- leaves the cost bit for bit as it was
                H2 = H.copy()
                H2[:, :3, 3] += np.random.default_rng(n).uniform(-1, 1, (n, 3)).astype(np.float32)
                H2[0, :3, 3] = np.float32(1e30)
                c1 = ops.ee_cost(cm, torch.as_tensor(H, device=DEV), tgt)
                c2 = ops.ee_cost(cm, torch.as_tensor(H2, device=DEV), tgt)
                assert torch.equal(c1, c2), f"w=({w_pos}, {w_rot}) square={square}: the cost moves with t"
    print(f"ee_cost w=({w_pos}, {w_rot}) square={square}: worst cost error {worst:.3g} of the derived bound")


# ---------------------------------------------------------------------------------------------------------------------------
# the same edges through the fused kernels
# ---------------------------------------------------------------------------------------------------------------------------
ROLLOUT_CASES = [("panda", True, "rollout"), ("panda", False, "rollout"), ("dual_panda", True, "rollout"),
                 ("dual_panda", True, "gp0"), ("dual_panda", True, "gp1")]
GP_WEIGHTS = ((0.0, 0.0, 1.0, 0.0), (0.0, 1.0, 1.0, 1.0))       # no self weight: the arm-per-lane schedule serves these


TOL_C_FUSED = 1e-5       # tests/test_gpu_parity.py's TOL_C, the constant of `rel_err(cost) < TOL_C` for the fused kernels


def _tol_c(c64):
    """Per sample: TOL_C_FUSED * max(1, |cost|).  The cost of a fused launch is a sum of some twenty terms of slope 1 in positions that
    are themselves good to TOL_H = 2e-6 max(1, |p|): 2e-6 per sample cannot be derived for it, and the fp32 oracle itself misses
    2e-6 max(1, |cost|) on these inputs (1.005 of it; the kernels: 1.85 to 2.98 of it, worst on the dual Panda).  The figure
    against 2e-6 is printed."""
    return TOL_C_FUSED * np.maximum(1.0, np.abs(c64))


def _rows_close(g, ref, rows, floor):
    """grad_close row by row (whole-row relative error below 1e-4 and the element-wise bound), silently, with the absolute floor
    of the whole launch: `floor` = its largest gradient entry"""
    out = []
    for i in rows:
        d = np.abs(g[i] - ref[i])
        out.append(bool(d.max() < 1e-4 * max(1e-30, np.abs(ref[i]).max(), 0.05 * floor) and (d <= GRAD_RTOL * np.abs(ref[i]) + GRAD_ATOL * floor).all()))
    return np.array(out, bool)


def _setup(ident, generated):
    kin, tmpl, q = T.rollout_robot(ident)
    h = ops.ModelHandle(kin)
    h.enable_specialized(generated)
    qt = torch.as_tensor(q, device=DEV)
    spec0 = T.rollout_spec(kin, tmpl, np.full(3, -T.FAR, np.float32), np.full(3, T.FAR, np.float32))
    pos, _, _ = ops.rollout_cost_grad(h, ops.CostHandle(spec0, DEV), (0, 0, 0, 0), qt)      # the kernel's own fp32 positions
    assert ops.last_dispatch() == ("generated" if generated else "table-driven")
    pos = _np(pos)
    q64 = q.astype(np.float64)
    pos64, _, _ = Oracle(kin, spec0).rollout(q64, (0, 0, 0, 0), "f64")
    assert (np.abs(pos - pos64) <= T.TOL_H * np.maximum(1.0, np.abs(pos64))).all()
    return kin, tmpl, q, qt, q64, h, pos, pos64


def _runner(mode, h, qt):
    if mode == "rollout":
        def run(cm, w):
            _, c, g = ops.rollout_cost_grad(h, cm, w, qt, want_pos=False)
            return _np(c).astype(np.float64).reshape(-1), _np(g).astype(np.float64).reshape(len(qt), -1)
        return run
    import os
    q3 = qt.reshape(5, 13, -1).contiguous()
    qd = torch.zeros_like(q3)

    def run_gp(cm, w):
        os.environ["TRK_GP_ARM_LANES"] = mode[-1]
        try:
            _, c, g, gqd = ops.rollout_gp_cost_grad(h, cm, w, q3, qd, 0.1, 0.3, 0.0, want_pos=False)
        finally:
            os.environ.pop("TRK_GP_ARM_LANES", None)
        assert (gqd == 0).all()                                           # the prior's weight is 0
        return _np(c).astype(np.float64).reshape(-1), _np(g).astype(np.float64).reshape(len(qt), -1)
    return run_gp


@pytest.mark.parametrize("ident,generated,mode", ROLLOUT_CASES, ids=[f"{i}-{'generated' if g else 'table'}-{m}" for i, g, m in ROLLOUT_CASES])
def test_ws_hinge_through_the_fused_kernels(ident, generated, mode):
    """rollout_cost_grad / rollout_collision / rollout_gp_cost_grad (either schedule of the dual Panda) on 65 fixed configurations and
    one box per (link, face, delta): the face lies at the kernel's own coordinate of that link -+ (margin + delta).  Every sample of every
    launch is held to the fp64 oracle; a sample with a link in the band 2 TOL_H max(1, |p|) of its hinge to the oracle's row with the
    face moved in or out by twice the band."""
    from helpers import grad_close
    kin, tmpl, q, qt, q64, h, pos, pos64 = _setup(ident, generated)
    run = _runner(mode, h, qt)
    served = "generated" if generated else "table-driven"
    boxes = T.rollout_boxes(pos, ident)
    assert len(boxes) == 3 * 6 * len(T.ROLLOUT_DELTAS) and len({b["face"] for b in boxes}) == 6 and len({b["slot"] for b in boxes}) == 3
    n_either = n_band = n_decided = 0
    worst_c = worst_b = 0.0
    for box in boxes:
        spec = T.rollout_spec(kin, tmpl, box["lo"], box["hi"])
        cm, orc = ops.CostHandle(spec, DEV), Oracle(kin, spec)
        v, band, sd = T.rollout_hinges64(pos64, tmpl.obj_links, spec.obj_link_margin, box["lo"], box["hi"])
        inb = np.abs(v) <= band
        assert inb.sum(1).max() <= 1, box                                 # at most one in-band pair per sample
        assert not inb.any() or abs(box["delta"]) < 1e-5, box
        assert inb[box["sample"], box["slot"]] == (abs(box["delta"]) < 1e-5), box
        rows = inb.any(1)
        n_band += int(inb.sum())
        sides = None
        for w in (T.ROLLOUT_WEIGHTS if mode == "rollout" else GP_WEIGHTS):
            c, g = run(cm, w)
            assert ops.last_dispatch() == served, (box, w, ops.last_dispatch())
            _, c64, g64 = orc.rollout(q64, w, "f64", want_pos=False)
            err = np.abs(c - c64)
            floor = float(np.abs(g64).max())
            assert np.isfinite(c).all() and np.isfinite(g).all()
            assert (err[~rows] <= _tol_c(c64)[~rows]).all(), (box, w, float((err / _tol_c(c64))[~rows].max()))
            assert grad_close(g[~rows], g64[~rows], scale=floor / max(1e-30, float(np.abs(g64[~rows]).max()))), (box, w)
            worst_c = max(worst_c, float((err / (T.TOL_C * np.maximum(1.0, np.abs(c64))))[~rows].max()))
            n_decided += int((~rows).sum())
            if rows.any():
                # either side of the clamp: the cost is continuous (the in-band term is at most the band), the gradient is the
                # oracle's with the face moved in (the term on) or out (off) by twice the band
                amount = 2.0 * float(band[inb].max())
                sides = [Oracle(kin, T.rollout_spec(kin, tmpl, *T.moved_face(box, s * amount))).rollout(q64, w, "f64", want_pos=False)[2] for s in (1.0, -1.0)]
                i = np.flatnonzero(rows)
                slack = w[2] * np.abs(v[inb])
                assert (err[i] <= _tol_c(c64)[i] + slack).all(), (box, w)
                assert (_rows_close(g, sides[0], i, floor) | _rows_close(g, sides[1], i, floor)).all(), (box, w, "neither side of the hinge")
                assert not np.array_equal(sides[0][i], sides[1][i])      # the two sides do differ: the check can tell them apart
                n_either += len(i)
        if mode == "rollout":
            hit = _np(ops.rollout_collision(h, cm, FIELD_WS, qt))
            assert ops.last_dispatch() == served
            mg = spec.obj_link_margin.astype(np.float64)[None, :, None]
            decided = (np.abs(sd - mg) > band[..., None]).all((1, 2))
            assert decided.sum() >= len(q) - 1 and np.array_equal(hit[decided], (sd < mg).any((1, 2))[decided]), box
            worst_b = max(worst_b, float(np.abs(sd - mg).min((1, 2))[~decided].max(initial=0.0)))
    n_w = 2
    assert n_band == 3 * 6 * 3 and n_either == n_w * n_band, (n_band, n_either)     # delta 0 and +-1e-7, one pair each; no more rows than that
    print(f"fused workspace hinge {ident} {served} {mode}: {len(boxes)} boxes, samples decided {n_decided}, judged either side {n_either} "
          f"(fp64 in-band pairs {n_band} x {n_w} weight tuples), worst decided cost error {worst_c:.3g} of 2e-6 max(1, |cost|), booleans undecided within {worst_b:.3g} m")


@pytest.mark.parametrize("ident,generated,mode", ROLLOUT_CASES, ids=[f"{i}-{'generated' if g else 'table'}-{m}" for i, g, m in ROLLOUT_CASES])
def test_ws_tie_through_the_fused_kernels(ident, generated, mode):
    """a box symmetric about one sample's link position in x and y, half the link's margin wide: four planes tie (as far as fp32
    bounds allow).  That sample's gradient must be the oracle's for SOME tied plane made the winner by twice the band."""
    kin, tmpl, q, qt, q64, h, pos, pos64 = _setup(ident, generated)
    run = _runner(mode, h, qt)
    box0, cand, s, slot = T.rollout_tie_box(pos, ident)
    spec = T.rollout_spec(kin, tmpl, box0["lo"], box0["hi"])
    cm, orc = ops.CostHandle(spec, DEV), Oracle(kin, spec)
    tied = T.rollout_tied_pairs(pos64, tmpl.obj_links, spec.obj_link_margin, box0["lo"], box0["hi"])
    assert tied[s, slot] and tied.sum() == 1
    rest = np.arange(len(q)) != s
    for w in (T.ROLLOUT_WEIGHTS if mode == "rollout" else GP_WEIGHTS):
        c, g = run(cm, w)
        _, c64, g64 = orc.rollout(q64, w, "f64", want_pos=False)
        floor = float(np.abs(g64).max())
        assert (np.abs(c - c64) <= _tol_c(c64)).all(), w
        assert _rows_close(g, g64, np.flatnonzero(rest), floor).all(), w
        refs = [Oracle(kin, T.rollout_spec(kin, tmpl, lo, hi)).rollout(q64, w, "f64", want_pos=False)[2] for lo, hi in cand]
        assert len({tuple(np.round(r[s], 6)) for r in refs}) == 4            # four different rows: the planes are told apart
        assert any(_rows_close(g, r, [s], floor)[0] for r in refs), (w, "the gradient of a plane that is not tied")


@pytest.mark.parametrize("clamp", [False, True])
def test_coincident_self_pairs_through_the_table_driven_rollout(clamp):
    """The Panda's links 1/2, 5/6 and 8/9 share an origin for every q: as self pairs (a user's table; with two of the template's) they
    contribute their margin and no gradient"""
    from helpers import grad_close
    kin, tmpl, q = T.rollout_robot("panda")
    h = ops.ModelHandle(kin)
    h.enable_specialized(False)
    qt, q64 = torch.as_tensor(q, device=DEV), q.astype(np.float64)
    spec, spec_rest, pl, mg = T.coincident_specs(clamp)
    pos, c, g = ops.rollout_cost_grad(h, ops.CostHandle(spec, DEV), (1, 0, 0, 0), qt)
    assert ops.last_dispatch() == "table-driven"
    pos, c, g = _np(pos), _np(c).astype(np.float64), _np(g).astype(np.float64)
    same = [bool(np.array_equal(pos[:, a], pos[:, b])) for a, b in pl[:3]]
    _, c_rest, g_rest = Oracle(kin, spec_rest).rollout(q64, (1, 0, 0, 0), "f64")
    sep = np.stack([np.linalg.norm(pos[:, a].astype(np.float64) - pos[:, b].astype(np.float64), axis=-1) for a, b in pl[:3]], -1)
    expect = c_rest + (mg[:3].astype(np.float64)[None] - sep).sum(-1)          # the oracle's value at the kernel's own separation
    print(f"coincident self pairs clamp={clamp}: columns bit-equal {same}, largest separation {sep.max():.3g} m")
    assert np.isfinite(c).all() and np.isfinite(g).all()
    assert (np.abs(c - expect) <= _tol_c(expect)).all()
    assert all(same) and (sep == 0).all()              # the walk adds the zero offset exactly: the margins come back exactly
    assert grad_close(g, g_rest)                       # and the pairs add nothing to the gradient


@pytest.mark.parametrize("ident,generated", [("panda", True), ("panda", False), ("dual_panda", True)])
def test_ee_on_target_through_the_fused_kernels(ident, generated):
    """the target(s) set to ops.fk's pose of one sample: with `square` that sample has no cost and no gradient; without it (position
    only) its gradient is a unit direction through the Jacobian or zero, nothing larger; every other sample is the oracle's"""
    from helpers import grad_close
    kin, tmpl, q, qt, q64, h, pos, pos64 = _setup(ident, generated)
    s = 20
    Hs = _np(ops.fk(h, qt)).reshape(len(q), kin.n_links, 4, 4)[s]
    links = [tmpl.ee_link] + ([tmpl.ee2_link] if tmpl.ee2_link >= 0 else [])
    targets = [Hs[l] for l in links] + [np.eye(4, dtype=np.float32)]
    rest = np.arange(len(q)) != s
    lo, hi = T.far_box(pos)
    w = (0.0, 0.0, 0.0, 1.0)
    for square, kw in ((True, dict(ee_square=True, ee_w_pos=1.0, ee_w_rot=1.0)), (False, dict(ee_square=False, ee_w_pos=1.0, ee_w_rot=0.0))):
        spec = T.rollout_spec(kin, tmpl, lo, hi, ee_targets=targets, ee_kw=kw)
        _, c, g = ops.rollout_cost_grad(h, ops.CostHandle(spec, DEV), w, qt, want_pos=False)
        assert ops.last_dispatch() == ("generated" if generated else "table-driven")
        c, g = _np(c).astype(np.float64), _np(g).astype(np.float64)
        _, c64, g64 = Oracle(kin, spec).rollout(q64, w, "f64", want_pos=False)
        assert np.isfinite(c).all() and np.isfinite(g).all()
        assert (np.abs(c - c64)[rest] <= _tol_c(c64)[rest]).all() and grad_close(g[rest], g64[rest]), square
        if square:
            assert c[s] < 1e-9 and np.abs(g[s]).max() <= 1e-4 * np.abs(g).max(), (c[s], np.abs(g[s]).max())
        else:
            smax = sum(float(np.linalg.svd(Oracle(kin).jacobian(q64[s:s + 1], None, l, "f64")[2][0], compute_uv=False)[0]) for l in links)
            assert np.linalg.norm(g[s]) <= kw["ee_w_pos"] * smax * (1 + 1e-4), (np.linalg.norm(g[s]), smax)
            assert c[s] <= 1e-6
