"""The inputs of tests/test_gpu_ik_edges.py, proved on the CPU: on exactly the batches the GPU test draws (tests/ik_helpers.py) the fp32
oracle stays within ONE QUARTER of every bound the kernels are held to, on all rows -- so a kernel that misses a bound is wrong, not
unlucky --, the share of elements the Adam comparison may skip stays under its cap, and every family holds the edge it is there for."""
import numpy as np
import pytest

import ik_helpers as ik
from helpers import ROLLOUT_BASES

QUARTER = 0.25


@pytest.fixture(scope="module")
def orc_of(oracle_lib):
    cache = {}

    def get(u, base="identity", clamp=True):
        key = (tuple(u), base, clamp)
        if key not in cache:
            kin, _tmpl, link = ik.unit(*u)
            if ROLLOUT_BASES[base] is not None:
                kin.set_base_pose(np.asarray(ROLLOUT_BASES[base], np.float32))
            if not clamp:
                kin = ik.without_stateful_clamp(kin)
            cache[key] = (oracle_lib.Oracle(kin), kin, link)
        return cache[key]
    return get


@pytest.mark.parametrize("u", ik.UNITS, ids=ik.unit_id)
def test_gauss_newton_fp32_oracle_keeps_a_quarter_of_every_bound(orc_of, u):
    worst = {}
    for base in ROLLOUT_BASES:
        orc, kin, link = orc_of(u, base)
        for n in ik.NS:
            for name, q0, Ht, lo, hi, pairs in ik.gn_cases(orc, kin, link, ik.unit_seed(u), n):
                for tgt in ((Ht, Ht[0]) if name == "F1" else (Ht,)):
                    for pair in pairs:
                        q64, e64 = ik.oracle_gn_step(orc, link, tgt, lo, hi, q0, pair, "f64")
                        q32, e32 = ik.oracle_gn_step(orc, link, tgt, lo, hi, q0, pair, "f32")
                        xq, xe = ik.gn_q_excess(q32, q64, q0), ik.gn_err_excess(name, e32, e64)
                        key = (name, pair)
                        worst[key] = np.maximum(worst.get(key, (0.0, 0.0)), (xq, xe))
                        assert xq <= QUARTER and xe < QUARTER, (base, n, name, pair, xq, xe)
    for key, (xq, xe) in worst.items():
        print(f"{ik.unit_id(u)} {key}: fp32 oracle uses {xq:.3f} of the q bound, {xe:.3f} of the err bound")


def test_at_a_half_turn_the_rotation_vector_sign_is_undecided(orc_of):
    """theta = pi exactly: fp32 and fp64 pick the sign of the rotation vector by rounding, and the steps differ by radians.  Nobody
    may `fix` the GPU test into comparing q there: it asserts finiteness, the limits and err only."""
    for u in ik.UNITS:
        orc, kin, link = orc_of(u)
        lo, hi = ik.limits(kin)
        q0, Ht, _ = ik.f2_rotation(orc, kin, link, ik.unit_seed(u) + 7, 2048, theta=np.pi)
        q64, e64 = ik.oracle_gn_step(orc, link, Ht, lo, hi, q0, ik.GN_PAIRS[0], "f64")
        q32, e32 = ik.oracle_gn_step(orc, link, Ht, lo, hi, q0, ik.GN_PAIRS[0], "f32")
        bad = (np.abs(q32 - q64) > ik.GN_Q_ATOL + ik.GN_Q_RTOL * np.abs(q64 - q0)).any(-1)
        print(f"{ik.unit_id(u)}: at pi {int(bad.sum())} of 2048 rows disagree, by up to {np.abs(q32 - q64).max():.2f} rad")
        assert bad.mean() > 0.10
        assert ik.gn_err_excess("F2", e32, e64) < QUARTER          # the distance itself is continuous there


@pytest.mark.parametrize("u", ik.UNITS, ids=ik.unit_id)
def test_adam_fp32_oracle_keeps_a_quarter_of_every_bound(orc_of, u):
    share, worst = {}, {}
    for base in ROLLOUT_BASES:
        orc, kin, link = orc_of(u, base)
        for n in ik.NS:
            for name, q0, Ht, lo, hi in ik.adam_cases(orc, kin, link, ik.unit_seed(u), n):
                q, m, v = q0, np.zeros_like(q0), np.zeros_like(q0)
                for it in range(ik.ADAM_STEPS):
                    r64, g64 = ik.oracle_adam_step(orc, link, Ht, lo, hi, q, m, v, it + 1, "f64")
                    r32, g32 = ik.oracle_adam_step(orc, link, Ht, lo, hi, q, m, v, it + 1, "f32")
                    # the fp32 oracle forms 1 - beta2 in fp32 (1 - 0.999f = 0.99998713e-3, 1.29e-5 off) where torch.optim.Adam and the
                    # kernels round 0.001 once: its v carries that constant's error, which is none of fp32 arithmetic's.  v's stand-in is
                    # the same update of the fp32 oracle's own gradient with the constants rounded once.
                    r32["v"] = np.float32(0.999) * v + np.float32(0.001) * g32 * g32
                    fig = ik.adam_compare(r32, r64, g64, q, lo, hi, 0.1, 300.0, scale=QUARTER, what=(base, n, name, it))
                    np.testing.assert_array_equal(r32["valid"], r64["valid"])
                    ex, nz = share.get(name, (0, 0))
                    share[name] = (ex + int(ik.adam_excluded(g64).sum()), nz + int((g64 != 0).sum()))
                    worst[name] = {k: max(fig[k], worst.get(name, {}).get(k, 0.0)) for k in ("loss", "q", "m", "v")}
                    q, m, v = (r64[k].astype(np.float32) for k in ("q", "m", "v"))      # both precisions go on from the same fp32 state
    for name, (ex, nz) in share.items():
        print(f"{ik.unit_id(u)} {name}: excluded {ex} of {nz} elements with a gradient ({ex / nz:.4f}); fp32 oracle worst {worst[name]}")
        assert ex <= ik.ADAM_EXCLUDED_CAP * nz, (name, ex, nz)


@pytest.mark.parametrize("u", ik.UNITS, ids=ik.unit_id)
def test_every_family_holds_its_edge(orc_of, u):
    orc, kin, link = orc_of(u)
    seed, n, D = ik.unit_seed(u), 130, kin.n_dofs
    lo, hi = ik.limits(kin)
    # F3: the step ends on a limit
    q0, Ht = ik.f3_on_limits(orc, kin, link, seed + 3, n)
    q64, _ = ik.oracle_gn_step(orc, link, Ht, lo, hi, q0, ik.GN_PAIRS[0], "f64")
    on = (q64 == lo.astype(np.float64)) | (q64 == hi.astype(np.float64))
    assert on.mean() >= 0.15, on.mean()
    assert ik.f3_edge_rows(kin, n) == 2 * D and not ik.inside(q0[:2 * D], lo, hi).any() and ik.inside(q0[2 * D:], lo, hi).all()
    assert (q0[2 * D:] == lo).any() and (q0[2 * D:] == hi).any()
    # F4: the stateful clamp changes the pose
    q4, _ = ik.f4_outside(orc, kin, link, seed + 4, n)
    free = orc_of(u, clamp=False)[0]
    moved = np.abs(ik.stateful_pose64(orc, link, q4) - ik.stateful_pose64(free, link, q4)).max((1, 2)) > 1e-3
    assert moved.mean() >= 0.20, moved.mean()
    wlo, whi = ik.wide_limits(kin)
    # (the UR10's joints range over 4 pi: some of its displaced elements leave even the box widened by 10, the others' never do)
    assert (ik.inside(q4, wlo, whi).all() or u[0] == "ur10") and ik.inside(q4, wlo, whi).mean() > 0.5 and not ik.inside(q4, lo, hi).all()
    # F5: a pinned joint of the chain
    q5, _, lo5, hi5 = ik.f5_pinned(orc, kin, link, seed + 5, n)
    pinned = np.flatnonzero(lo5 == hi5)
    assert len(pinned) == 1 and pinned[0] in ik.chain_dofs(kin, link) and (q5[:, pinned[0]] == lo5[pinned[0]]).all()
    # the Jacobian's columns: the file-order rule, not ancestry
    chain, cols = ik.chain_dofs(kin, link), ik.column_dofs(kin, link)
    q1, H1 = ik.f1_random(orc, kin, link, seed + 1, n)
    q64, _ = ik.oracle_gn_step(orc, link, H1, lo, hi, q1, ik.GN_PAIRS[0], "f64")
    step = q64 - q1.astype(np.float64)
    lin, ang = orc.jacobian(q1.astype(np.float64), None, link, "f64")[2:4]
    extra = [d for d in cols if d not in chain]
    none = [d for d in range(D) if d not in cols]
    expect = {("panda_arm_hand", None): ([7, 8], []), ("panda_arm_hand", "panda_rightfinger"): ([7], []),
              ("panda_arm_hand", "panda_leftfinger"): ([], [8]), ("panda", "panda_link4"): ([], [4, 5, 6])}
    if tuple(u) in expect:
        assert (extra, none) == expect[tuple(u)], (extra, none)
    for d in extra:                                     # a non-ancestor's column is there and moves its joint
        assert np.abs(ang[:, :, d]).max(1).min() > 0.5 and (np.abs(step[:, d]) > 1e-6).mean() > 0.5, d
    for d in none:                                      # no column: the step is exactly zero
        assert (lin[:, :, d] == 0).all() and (ang[:, :, d] == 0).all() and (step[:, d] == 0.0).all(), d


@pytest.mark.parametrize("u", ik.UNITS, ids=ik.unit_id)
def test_hinge_of_the_one_ulp_rows_fp32_oracle_keeps_a_quarter(orc_of, u):
    orc, kin, link = orc_of(u)
    lo, hi = ik.limits(kin, ik.ADAM_SHRINK)
    q0, Ht = ik.f3_on_limits(orc, kin, link, ik.unit_seed(u) + 3, 63, lo, hi)
    z = np.zeros_like(q0)

    def loss_of(prec):
        return lambda lo_, hi_, w: ik.oracle_adam_step(orc, link, Ht, lo_, hi_, q0, z, z, 1, prec, lr=0.0, w_jl=w)[0]["loss"]
    x = ik.hinge_excess(loss_of("f32"), kin, q0, lo, hi, loss_of("f64"))
    print(f"{ik.unit_id(u)}: fp32 oracle uses {x:.4f} of the hinge bound")
    assert x < QUARTER
