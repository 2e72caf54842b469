"""The generated IK kernels off the Panda's happy path: k_ikgn (trk_ik_gn_steps) and k_ik (trk_ik_steps) of the bundled units of four
robots (6, 7 and 9 DOF) and of three run-time units whose tracked link has non-ancestor or missing Jacobian columns, against the fp64
oracle on the input families of tests/ik_helpers.py -- other unit shapes, the file-order column rule, rotations up to a half turn and
down to zero, starts on / one ulp outside / far outside the limits, the stateful walk's URDF clamp, a pinned joint, a zero residual --
and at the edges of rows and buffers.  tests/test_ik_edges_cpu.py proves on the CPU that the fp32 oracle alone keeps a quarter of every
bound used here, on these very batches.

Measured on an MI355X over all units, families, batch sizes and both base poses (kernel / fp32 oracle alone): Gauss-Newton q 0.072 /
0.10 of 1e-4 + 5e-3 |dq|, err 0.022 / 0.021 of 2e-5; Adam loss 2.5e-7 / 2.2e-7 (bound 1e-4), q 1.1e-6 / 1.0e-6 (2e-4), m 4.6e-7 /
5.3e-7 and v 9.3e-7 / 6.9e-7 (1e-5 of the largest entry); the one-ulp hinge 0.0024 / 0.0024 of 1e-4; at most 0.69 % of the elements
with a gradient are left out of the Adam q comparison (cap 1 %).

Mutants these tests were shown to fail on (none committed): the Jacobian's non-ancestor columns dropped -- the step tests on
panda_arm_hand; the rotation vector's sign pick moved to w < -0.5 -- the step tests on every unit; `q >= lower` made strict in `valid`
-- both valid tests on every unit.  Replacing the stateful walk's angles by the stateless ones is NOT a mutant on these four robots
(both clamp every joint: the emitted kernel only gains an unused mask); an oracle without the clamp misses F4 by three orders of
magnitude.  Dropping the `min(base + lane, n - 1)` target clamp changes what idle lanes read, not any row's value."""
import numpy as np
import pytest
import torch

import ik_helpers as ik
from helpers import ROLLOUT_BASES, rel_err
from torch_robotics_amd import jit

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7777.0
ROW_UNITS = [("panda_arm_hand", None), ("ur10", None)]          # the row and buffer tests: D = 9 (two-wavefront launch bound) and D = 6


@pytest.fixture(scope="module")
def ops():
    from torch_robotics_amd import ops as _ops
    return _ops


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def ctx(ops, oracle_lib):
    """(handle, oracle, KinModel, link) of a unit at a base pose; a run-time unit is compiled (or found in the cache) on first use.  Every
    handle is shown to be served by the generated kernels before anything is compared on it."""
    cache = {}

    def get(u, base="identity"):
        key = (tuple(u), base)
        if key not in cache:
            kin, tmpl, link = ik.unit(*u)
            if u[1] is not None:
                jit.specialize(kin, tmpl.obj_links, (), ee_link=link)
            if ROLLOUT_BASES[base] is not None:
                kin.set_base_pose(np.asarray(ROLLOUT_BASES[base], np.float32))
            h, orc = ops.ModelHandle(kin), oracle_lib.Oracle(kin)
            assert h.specialized, u
            lo, hi = ik.limits(kin)
            q0, Ht = ik.f1_random(orc, kin, link, 99, 130)
            a = adam(ops, h, link, Ht, lo, hi, q0)
            h.enable_specialized(False)
            b = adam(ops, h, link, Ht, lo, hi, q0)
            with pytest.raises(Exception, match="no generated unit"):
                gn(ops, h, link, Ht, lo, hi, q0, ik.GN_PAIRS[0])
            h.enable_specialized(True)
            assert not (np.array_equal(a["q"], b["q"]) and np.array_equal(a["m"], b["m"]) and np.array_equal(a["loss"], b["loss"])), \
                f"{u}: trk_ik_steps did not take the generated kernel"
            gn(ops, h, link, Ht, lo, hi, q0, ik.GN_PAIRS[0])           # (raises when no unit tracks the link)
            cache[key] = (h, orc, kin, link)
        return cache[key]
    return get


def gn(ops, h, link, Ht, lo, hi, q0, pair, K=1, se3_eps=0.1):
    """ops.ik_gn_steps on copies -> dict(q, err, valid) as numpy"""
    n = len(q0)
    q, err, valid = dev(q0).clone(), torch.empty(n, device=DEV), torch.empty(n, device=DEV, dtype=torch.uint8)
    ops.ik_gn_steps(h, link, dev(Ht), dev(lo), dev(hi), q, K, damping=pair[0], lm_gain=pair[1], step_scale=pair[2], se3_eps=se3_eps,
                    err=err, valid=valid)
    return dict(q=host(q), err=host(err), valid=host(valid).astype(bool))


def adam(ops, h, link, Ht, lo, hi, q0, m0=None, v0=None, step=1, K=None, lr=ik.ADAM_LR, w_jl=300.0, se3_eps=0.1):
    """ops.ik_step (K None) or ops.ik_steps on copies -> dict(q, m, v, loss, valid) as numpy"""
    n = len(q0)
    q = dev(q0).clone()
    m, v = (torch.zeros_like(q) if a is None else dev(a).clone() for a in (m0, v0))
    loss, valid = torch.empty(n, device=DEV), torch.empty(n, device=DEV, dtype=torch.uint8)
    kw = dict(lr=lr, w_joint_limits=w_jl, se3_eps=se3_eps, loss=loss, valid=valid)
    if K is None:
        ops.ik_step(h, link, dev(Ht), dev(lo), dev(hi), q, m, v, step, **kw)
    else:
        ops.ik_steps(h, link, dev(Ht), dev(lo), dev(hi), q, m, v, step, K, **kw)
    return dict(q=host(q), m=host(m), v=host(v), loss=host(loss), valid=host(valid).astype(bool))


def same_bits(a, b, keys=None, rows=None):
    for k in (keys or a.keys()):
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y, err_msg=k)


@pytest.mark.parametrize("u", ik.UNITS, ids=ik.unit_id)
def test_both_ik_entry_points_take_the_generated_kernels(ctx, u):
    """What `ctx` asserts, under a name of its own: trk_ik_steps on a link that only a run-time unit tracks used to fall back to the
    table-driven kernel without a word (it looked at the model's first unit alone); trk_ik_gn_steps found the unit."""
    for base in ROLLOUT_BASES:
        ctx(u, base)


# ---------------------------------------------------------------------------------------------------------------------------
# Gauss-Newton
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u", ik.UNITS, ids=ik.unit_id)
def test_gauss_newton_step_vs_fp64_oracle(ops, ctx, u):
    """F1 - F6, one step, both kernels (_bi / _bg), every parameter pair, per-sample targets and (F1) a single one; a DOF without a
    Jacobian column comes back bit-identical when it is inside the limits"""
    worst = {}
    for base in ROLLOUT_BASES:
        h, orc, kin, link = ctx(u, base)
        none = [d for d in range(kin.n_dofs) if d not in ik.column_dofs(kin, link)]
        for n in ik.NS:
            for name, q0, Ht, lo, hi, pairs in ik.gn_cases(orc, kin, link, ik.unit_seed(u), n):
                for tgt in ((Ht, Ht[0]) if name == "F1" else (Ht,)):
                    for pair in pairs:
                        q64, e64 = ik.oracle_gn_step(orc, link, tgt, lo, hi, q0, pair, "f64")
                        r = gn(ops, h, link, tgt, lo, hi, q0, pair)
                        xq, xe = ik.gn_q_excess(r["q"], q64, q0), ik.gn_err_excess(name, r["err"], e64)
                        worst[name] = np.maximum(worst.get(name, (0.0, 0.0)), (xq, xe))
                        assert xq <= 1.0 and xe < 1.0, (base, n, name, pair, tgt.ndim, xq, xe)
                        assert np.isfinite(r["q"]).all() and (r["q"] >= lo).all() and (r["q"] <= hi).all()
                        for d in none:
                            keep = (q0[:, d] >= lo[d]) & (q0[:, d] <= hi[d])
                            np.testing.assert_array_equal(r["q"][keep, d].view(np.uint32), q0[keep, d].view(np.uint32))
    print(f"{ik.unit_id(u)}: share of the (q, err) bound used, per family: " + ", ".join(f"{k} ({a:.3f}, {b:.3f})" for k, (a, b) in worst.items()))


@pytest.mark.parametrize("u", ik.UNITS, ids=ik.unit_id)
def test_gauss_newton_at_a_half_turn(ops, ctx, u):
    """theta = pi exactly: the rotation vector's sign is undecided (the CPU test shows fp32 and fp64 disagree by radians), so only:
    every output finite and inside the limits, err the oracle's (it is continuous there)"""
    h, orc, kin, link = ctx(u)
    lo, hi = ik.limits(kin)
    for n in ik.NS:
        q0, Ht, _ = ik.f2_rotation(orc, kin, link, ik.unit_seed(u) + 7, n, theta=np.pi)
        for pair in ik.GN_ALL_PAIRS:
            _, e64 = ik.oracle_gn_step(orc, link, Ht, lo, hi, q0, pair, "f64")
            r = gn(ops, h, link, Ht, lo, hi, q0, pair)
            assert np.isfinite(r["q"]).all() and np.isfinite(r["err"]).all() and (r["q"] >= lo).all() and (r["q"] <= hi).all()
            assert rel_err(r["err"], e64) < ik.GN_ERR_RTOL


@pytest.mark.parametrize("u", ik.UNITS, ids=ik.unit_id)
def test_gauss_newton_six_successive_steps(ops, ctx, u):
    """six single steps on F1, the oracle re-fed the kernel's own q each step"""
    h, orc, kin, link = ctx(u)
    lo, hi = ik.limits(kin)
    for n in ik.NS:
        q, Ht = ik.f1_random(orc, kin, link, ik.unit_seed(u) + 8, n)
        for it in range(6):
            q64, e64 = ik.oracle_gn_step(orc, link, Ht, lo, hi, q, ik.GN_PAIRS[0], "f64")
            r = gn(ops, h, link, Ht, lo, hi, q, ik.GN_PAIRS[0])
            assert ik.gn_q_excess(r["q"], q64, q) <= 1.0 and rel_err(r["err"], e64) < ik.GN_ERR_RTOL, (n, it)
            sure = np.abs(e64 - 0.1) > ik.VALID_BAND
            np.testing.assert_array_equal(r["valid"][sure], ((e64 < 0.1) & ik.inside(q, lo, hi))[sure])
            q = r["q"]


@pytest.mark.parametrize("u", ik.UNITS, ids=ik.unit_id)
def test_gauss_newton_valid_is_decided_by_the_limits_alone(ops, ctx, u):
    """se3_eps = 100: a row on a limit is valid, a row one ulp outside is not; every row as numpy decides it"""
    h, orc, kin, link = ctx(u)
    lo, hi = ik.limits(kin)
    for n in ik.NS:
        q0, Ht = ik.f3_on_limits(orc, kin, link, ik.unit_seed(u) + 3, n)
        r = gn(ops, h, link, Ht, lo, hi, q0, ik.GN_PAIRS[0], se3_eps=100.0)
        np.testing.assert_array_equal(r["valid"], ik.inside(q0, lo, hi))
        k = ik.f3_edge_rows(kin, n)
        assert not r["valid"][:k].any() and r["valid"][k:].all()


@pytest.mark.parametrize("u,Ks", [(("panda_arm_hand", None), (3, 17)), (("panda_arm_hand", "panda_rightfinger"), (3, 17)), (("ur10", None), (3,))],
                         ids=lambda x: ik.unit_id(x) if isinstance(x[0], str) else None)
def test_gauss_newton_k_steps_in_one_launch_equal_k_launches(ops, ctx, u, Ks):
    h, orc, kin, link = ctx(u)
    lo, hi = ik.limits(kin)
    q0, Ht = ik.f1_random(orc, kin, link, ik.unit_seed(u) + 9, 130)
    for K in Ks:
        q, first = q0, None
        for it in range(K):
            r = gn(ops, h, link, Ht, lo, hi, q, ik.GN_PAIRS[0])
            first, q = (r if it == 0 else first), r["q"]
        one = gn(ops, h, link, Ht, lo, hi, q0, ik.GN_PAIRS[0], K=K)
        same_bits(dict(q=q, err=first["err"], valid=first["valid"]), one)


# ---------------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u", ik.UNITS, ids=ik.unit_id)
def test_adam_steps_vs_fp64_oracle(ops, ctx, u):
    """F1, F3, F4: three steps from zero moments, the oracle fed the kernel's q, m, v after each; loss, valid, q (outside the capped
    exclusion set), m, v.  An element whose oracle gradient is exactly zero and that lies inside the limits keeps its bits, m = v = 0."""
    worst, zeros = {}, 0
    for base in ROLLOUT_BASES:
        h, orc, kin, link = ctx(u, base)
        for n in ik.NS:
            for name, q0, Ht, lo, hi in ik.adam_cases(orc, kin, link, ik.unit_seed(u), n):
                q, m, v = q0, np.zeros_like(q0), np.zeros_like(q0)
                for it in range(ik.ADAM_STEPS):
                    r64, g64 = ik.oracle_adam_step(orc, link, Ht, lo, hi, q, m, v, it + 1, "f64")
                    r = adam(ops, h, link, Ht, lo, hi, q, m, v, step=it + 1)
                    fig = ik.adam_compare(r, r64, g64, q, lo, hi, 0.1, 300.0, what=(base, n, name, it))
                    worst[name] = {k: max(fig[k], worst.get(name, {}).get(k, 0.0)) for k in ("loss", "q", "m", "v")}
                    # no gradient, no hinge and no momentum from an earlier step's hinge: nothing may move (the finger DOFs off the
                    # tracked chain; in F4 also the DOFs the stateless walk clamps, whose gradient the clamp kills)
                    still = (g64 == 0.0) & (q >= lo) & (q <= hi) & (m == 0.0) & (v == 0.0)
                    zeros += int(still.sum())
                    np.testing.assert_array_equal(r["q"][still].view(np.uint32), q[still].view(np.uint32), err_msg=f"{base} {n} {name} {it}")
                    assert (r["m"][still] == 0).all() and (r["v"][still] == 0).all(), (base, n, name, it)
                    q, m, v = r["q"], r["m"], r["v"]
    assert zeros > 0 or len(ik.chain_dofs(kin, link)) == kin.n_dofs
    print(f"{ik.unit_id(u)}: worst against the fp64 oracle {worst}; {zeros} elements without a gradient kept their bits")


@pytest.mark.parametrize("u", ik.UNITS, ids=ik.unit_id)
def test_adam_valid_is_decided_by_the_limits_alone(ops, ctx, u):
    h, orc, kin, link = ctx(u)
    lo, hi = ik.limits(kin, ik.ADAM_SHRINK)
    for n in ik.NS:
        q0, Ht = ik.f3_on_limits(orc, kin, link, ik.unit_seed(u) + 3, n, lo, hi)
        r = adam(ops, h, link, Ht, lo, hi, q0, se3_eps=100.0)
        np.testing.assert_array_equal(r["valid"], ik.inside(q0, lo, hi))
        assert not r["valid"][:ik.f3_edge_rows(kin, n)].any() and (n == 1 or r["valid"].any())


@pytest.mark.parametrize("u", ik.UNITS, ids=ik.unit_id)
def test_adam_hinge_one_ulp_outside_and_on_the_limit(ops, ctx, u):
    """One ulp outside a limit the hinge is w_jl e^2, the oracle's value (each row at the weight that makes it visible in fp32:
    ik_helpers.hinge_rows); exactly on a limit it is exactly zero -- the loss has the bits of the loss with every limit widened by 1.0."""
    h, orc, kin, link = ctx(u)
    lo, hi = ik.limits(kin, ik.ADAM_SHRINK)
    q0, Ht = ik.f3_on_limits(orc, kin, link, ik.unit_seed(u) + 3, 63, lo, hi)
    z = np.zeros_like(q0)
    x = ik.hinge_excess(lambda lo_, hi_, w: adam(ops, h, link, Ht, lo_, hi_, q0, lr=0.0, w_jl=w)["loss"], kin, q0, lo, hi,
                        lambda lo_, hi_, w: ik.oracle_adam_step(orc, link, Ht, lo_, hi_, q0, z, z, 1, "f64", lr=0.0, w_jl=w)[0]["loss"])
    print(f"{ik.unit_id(u)}: the hinge of the one-ulp rows uses {x:.4f} of its bound")
    assert x < 1.0
    for n in ik.NS[1:]:
        q0, Ht = ik.f3_on_limits(orc, kin, link, ik.unit_seed(u) + 3, n, lo, hi)
        on = ik.inside(q0, lo, hi) & ((q0 == lo) | (q0 == hi)).any(-1)
        assert on.sum() >= 8
        a = adam(ops, h, link, Ht, lo, hi, q0, lr=0.0)
        b = adam(ops, h, link, Ht, lo - np.float32(1.0), hi + np.float32(1.0), q0, lr=0.0)
        same_bits(a, b, keys=("loss",), rows=on)


@pytest.mark.parametrize("u", ik.UNITS, ids=ik.unit_id)
def test_adam_lr_zero_only_evaluates(ops, ctx, u):
    h, orc, kin, link = ctx(u)
    for n in ik.NS:
        for name, q0, Ht, lo, hi in ik.adam_cases(orc, kin, link, ik.unit_seed(u), n):
            rng = np.random.default_rng(5)
            m0, v0 = rng.normal(size=q0.shape).astype(np.float32), rng.random(q0.shape).astype(np.float32)
            first = adam(ops, h, link, Ht, lo, hi, q0)
            r = adam(ops, h, link, Ht, lo, hi, q0, m0, v0, step=4, lr=0.0)
            same_bits(r, dict(q=q0, m=m0, v=v0, loss=first["loss"], valid=first["valid"]))


@pytest.mark.parametrize("u", ROW_UNITS, ids=ik.unit_id)
def test_adam_k_steps_in_one_call_equal_single_steps(ops, ctx, u):
    """K = 40 spans two launches of at most 32"""
    h, orc, kin, link = ctx(u)
    lo, hi = ik.limits(kin, ik.ADAM_SHRINK)
    q0, Ht = ik.f1_random(orc, kin, link, ik.unit_seed(u) + 9, 130)
    for K in (5, 40):
        r, first = dict(q=q0, m=None, v=None), None
        for it in range(K):
            r = adam(ops, h, link, Ht, lo, hi, r["q"], r["m"], r["v"], step=it + 1)
            first = r if it == 0 else first
        one = adam(ops, h, link, Ht, lo, hi, q0, K=K)
        same_bits(dict(q=r["q"], m=r["m"], v=r["v"], loss=first["loss"], valid=first["valid"]), one)


@pytest.mark.parametrize("u", [("ur10", None), ("panda_arm_hand", None), ("panda_arm_hand", "panda_rightfinger")], ids=ik.unit_id)
def test_adam_generated_equals_table_driven(ops, ctx, u):
    """one step on F1, the bounds and the exclusion set of the oracle comparison: the table-driven kernel on a prismatic chain"""
    for base in ROLLOUT_BASES:
        h, orc, kin, link = ctx(u, base)
        lo, hi = ik.limits(kin, ik.ADAM_SHRINK)
        for n in ik.NS:
            q0, Ht = ik.f1_random(orc, kin, link, ik.unit_seed(u) + 1, n)
            _, g64 = ik.oracle_adam_step(orc, link, Ht, lo, hi, q0, np.zeros_like(q0), np.zeros_like(q0), 1, "f64")
            a = adam(ops, h, link, Ht, lo, hi, q0)
            h.enable_specialized(False)
            try:
                b = adam(ops, h, link, Ht, lo, hi, q0)
            finally:
                h.enable_specialized(True)
            ik.adam_compare(a, {k: (x.astype(np.float64) if x.dtype == np.float32 else x) for k, x in b.items()}, g64, q0, lo, hi, 0.1, 300.0, what=(base, n))


# ---------------------------------------------------------------------------------------------------------------------------
# rows and buffers, both kernels
# ---------------------------------------------------------------------------------------------------------------------------
def _in_sentinels(n_elems, dtype=torch.float32, off=1):
    """(view of n_elems at an offset that is 4-byte but not 16-byte aligned, the whole buffer)"""
    off = off if dtype == torch.float32 else 4
    buf = torch.full((n_elems + 16,), SENTINEL if dtype == torch.float32 else 0xA5, device=DEV, dtype=dtype)
    view = buf[off:off + n_elems]
    assert view.data_ptr() % 4 == 0 and view.data_ptr() % 16 != 0
    return view, buf, off


def _untouched(buf, off, n_elems):
    s = buf[0].item()
    return bool((buf[:off] == s).all()) and bool((buf[off + n_elems:] == s).all())


@pytest.mark.parametrize("u", ROW_UNITS, ids=ik.unit_id)
def test_unaligned_buffers_between_sentinels(ops, ctx, u):
    h, orc, kin, link = ctx(u)
    D = kin.n_dofs
    lo, hi = ik.limits(kin, ik.ADAM_SHRINK)
    for n in ik.NS:
        q0, Ht = ik.f1_random(orc, kin, link, ik.unit_seed(u) + 10, n)
        bufs = {k: _in_sentinels(n * D) for k in ("q", "m", "v")}
        bufs["loss"], bufs["valid"], bufs["Ht"] = _in_sentinels(n), _in_sentinels(n, torch.uint8), _in_sentinels(n * 16)
        t = {k: b[0] for k, b in bufs.items()}
        q, m, v, Hd = t["q"].view(n, D), t["m"].view(n, D), t["v"].view(n, D), t["Ht"].view(n, 4, 4)
        Hd.copy_(dev(Ht))
        # Gauss-Newton
        q.copy_(dev(q0))
        ops.ik_gn_steps(h, link, Hd, dev(lo), dev(hi), q, 2, err=t["loss"], valid=t["valid"])
        ref = gn(ops, h, link, Ht, lo, hi, q0, ik.GN_PAIRS[0], K=2)
        same_bits(dict(q=host(q), err=host(t["loss"]), valid=host(t["valid"]).astype(bool)), ref)
        # Adam
        q.copy_(dev(q0)); m.zero_(); v.zero_()
        ops.ik_steps(h, link, Hd, dev(lo), dev(hi), q, m, v, 1, 2, lr=ik.ADAM_LR, loss=t["loss"], valid=t["valid"])
        ref = adam(ops, h, link, Ht, lo, hi, q0, K=2)
        same_bits(dict(q=host(q), m=host(m), v=host(v), loss=host(t["loss"]), valid=host(t["valid"]).astype(bool)), ref)
        for k, (view, buf, off) in bufs.items():
            assert _untouched(buf, off, view.numel()), (n, k)


@pytest.mark.parametrize("u", ROW_UNITS, ids=ik.unit_id)
def test_a_non_finite_row_stays_in_its_row(ops, ctx, u):
    """a row of NaN, and a row holding an inf, at the edges of the wavefronts: every other row has the bits of the clean run"""
    h, orc, kin, link = ctx(u)
    n, D = 130, kin.n_dofs
    lo, hi = ik.limits(kin, ik.ADAM_SHRINK)
    q0, Ht = ik.f1_random(orc, kin, link, ik.unit_seed(u) + 11, n)
    clean_gn, clean_adam = gn(ops, h, link, Ht, lo, hi, q0, ik.GN_PAIRS[0], K=2), adam(ops, h, link, Ht, lo, hi, q0, K=2)
    for pos in (0, 63, 64, n - 1):
        for kind in ("nan", "inf"):
            qb = q0.copy()
            if kind == "nan":
                qb[pos] = np.nan
            else:
                qb[pos, pos % D] = np.inf
            others = np.arange(n) != pos
            r = gn(ops, h, link, Ht, lo, hi, qb, ik.GN_PAIRS[0], K=2)
            same_bits(r, clean_gn, rows=others)
            assert not r["valid"][pos], ("gn", pos, kind)
            r = adam(ops, h, link, Ht, lo, hi, qb, K=2)
            same_bits(r, clean_adam, rows=others)
            assert not r["valid"][pos], ("adam", pos, kind)


@pytest.mark.parametrize("u", ROW_UNITS, ids=ik.unit_id)
def test_per_sample_targets_in_the_tail_wavefront(ops, ctx, u):
    """the last row of a ragged batch reads ITS target: the same bits as a batch of one on that row with that target"""
    h, orc, kin, link = ctx(u)
    lo, hi = ik.limits(kin, ik.ADAM_SHRINK)
    for n in (65, 130):
        q0, Ht = ik.f1_random(orc, kin, link, ik.unit_seed(u) + 12, n)
        assert len(np.unique(Ht.reshape(n, -1), axis=0)) == n
        last = slice(n - 1, n)
        a, b = gn(ops, h, link, Ht, lo, hi, q0, ik.GN_PAIRS[0], K=2), gn(ops, h, link, Ht[last], lo, hi, q0[last], ik.GN_PAIRS[0], K=2)
        same_bits({k: x[last] for k, x in a.items()}, b)
        a, b = adam(ops, h, link, Ht, lo, hi, q0, K=2), adam(ops, h, link, Ht[last], lo, hi, q0[last], K=2)
        same_bits({k: x[last] for k, x in a.items()}, b)
