"""trk_pack_sums (k_pack_partial / k_pack_finish), trk_reduce_sum (k_reduce_sum / k_reduce_sum_wide) and trk_scale_rows (k_scale_rows)
held to the bit.  All three are sums or single products, so the inputs (tests/sums_helpers.py, checked on their own by
tests/test_sums_refs_cpu.py) are chosen so that the correct fp32 result does not depend on the association order: an int64 reference,
compared as bit patterns -- no tolerance that a dropped, doubled or misplaced element could hide in.

  1  trk_pack_sums on position-coded integers: ten shapes at the slice, tile and unit-width boundaries, fp32 and fp16 gradients, three
     loss scales, traj_cost absent and given, the 16-byte and the scalar unit path on the same numbers (views 4 / 2 bytes off a 16-byte
     boundary), scratch filled with NaN and with zeros, sentinels around scratch and packed, inputs unmodified, replay
  2  ops.PackedSums against the raw call at D = 6 and D = 14
  3  trk_pack_sums on real-valued columns, each on its own scale: a per-column bound from the documented association order
  4  trk_reduce_sum at the boundaries of its two kernels and of the wide kernel's three loops, aligned and one float in
  5  trk_scale_rows: raw ABI and ops.scale_rows, fp32 and fp16 (ties, subnormals, negative zero), one scale and one per row, in place,
     offset views, sentinels
  6  the three autograd routes of the fused rollout (ctypes Function, torch.ops.trk.rollout_cost_grad, native trk::rollout) under five
     upstream gradients, against gq x gcost rounded as the kernel rounds it, and against one another"""
import faulthandler
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import helpers as hp
import sums_helpers as sh
import test_gpu_arm_traj_terms as tt
from torch_robotics_amd import _lib, custom_ops, jit, ops  # noqa: F401  (custom_ops registers torch.ops.trk.*)
from torch_robotics_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S = 1234.0                     # the sentinel: exact in fp16 as well
TORCH_OF = {np.dtype(np.float32): torch.float32, np.dtype(np.float16): torch.float16}
FILE_TIME_LIMIT_S = 300        # the whole file runs in seconds


@pytest.fixture(scope="module", autouse=True)
def file_time_limit():
    """A launch that never returns ends the process with a traceback of every thread instead of holding the GPU."""
    faulthandler.dump_traceback_later(FILE_TIME_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def host(t):
    return t.detach().cpu().numpy()


class Placed:
    """A device array `off` bytes past a 16-byte boundary, with 16 bytes of sentinels in front of it and behind it.  a: the numpy array
    to place, or (shape, dtype, fill) of an output."""

    def __init__(self, a, off=0):
        if isinstance(a, tuple):
            shape, dtype, fill = a
            src = None
        else:
            shape, dtype, fill, src = a.shape, TORCH_OF[a.dtype], None, a
        item = torch.empty(0, dtype=dtype).element_size()
        assert off % item == 0 and 0 <= off < 16
        n = int(np.prod(shape))
        self.lead, self.n = (16 + off) // item, n
        self.buf = torch.full((self.lead + n + 16 // item,), S, dtype=dtype, device=DEV)
        self.v = self.buf[self.lead:self.lead + n].view(*shape)
        if src is not None:
            self.v.copy_(dev(src))
        else:
            self.v.fill_(fill)
        assert self.v.data_ptr() % 16 == off and self.v.is_contiguous()

    def guards_intact(self):
        return bool((self.buf[:self.lead] == S).all() and (self.buf[self.lead + self.n:] == S).all())


def same_bits(t, a):
    """device tensor t == numpy array a as bit patterns"""
    return np.array_equal(sh.bits(host(t)), sh.bits(np.asarray(a)))


# 1 -----------------------------------------------------------------------------------------------------------------------------------
def pack_raw(cost, gq, gs, block, traj, B, H, D, scratch, packed):
    rc = lib().trk_pack_sums(cost.data_ptr(), gq.data_ptr(), int(gq.dtype == torch.float16), float(gs), block.data_ptr(),
                             None if traj is None else traj.data_ptr(), B, H, D, scratch.data_ptr(), packed.data_ptr(), stream())
    assert rc == 0, lib().trk_last_error()


def scratch_floats(H, D):
    nbytes = int(lib().trk_pack_sums_scratch_bytes(H, D))
    assert nbytes >= 4 * 128 * (H + H * D) and nbytes % 4 == 0            # the partial rows of the 128-slice cap at least
    return nbytes // 4


@pytest.mark.parametrize("shape", sh.PACK_SHAPES, ids=str)
def test_pack_sums_of_coded_inputs_to_the_bit(shape):
    B, H, D = shape
    inp = sh.pack_inputs(B, H, D)
    size, nfl = 1 + H + H * D, scratch_floats(H, D)
    cost_np, g32_np = sh.as_f32(inp["cost"], sh.COST_UNIT), sh.as_f32(inp["gq"], sh.GQ_UNIT)
    block, traj = dev(sh.as_f32(inp["block"], sh.BLOCK_UNIT)), dev(sh.as_f32(inp["traj"], sh.TRAJ_UNIT))
    block0, traj0 = block.clone(), traj.clone()
    for f16 in (False, True):
        g_np = g32_np.astype(np.float16) if f16 else g32_np
        first = {}
        for off in (0, 4):                            # off = 4: no array is 16-byte aligned -> scalar units even where H % 4 == 0
            cost, gq = Placed(cost_np, off), Placed(g_np, off // 2 if f16 else off)
            for gs in (sh.PACK_GRAD_SCALES if f16 else (1.0,)):
                for tc in (None, traj):
                    what = (shape, "fp16" if f16 else "fp32", gs, tc is not None, off)
                    ref = sh.packed_reference(inp, tc is not None, gs)
                    scr = Placed(((nfl,), torch.float32, float("nan")), off)
                    out = Placed(((size,), torch.float32, S))
                    pack_raw(cost.v, gq.v, gs, block, tc, B, H, D, scr.v, out.v)
                    got = host(out.v).copy()
                    print(what, "packed[:3]", got[:3], "reference", ref[:3])
                    assert np.isfinite(got).all(), what
                    bad = np.flatnonzero(sh.bits(got) != sh.bits(ref))
                    assert len(bad) == 0, (what, "first wrong entries", bad[:8], got[bad[:8]], ref[bad[:8]])
                    assert scr.guards_intact() and out.guards_intact(), what
                    pack_raw(cost.v, gq.v, gs, block, tc, B, H, D, scr.v, out.v)          # replay: same packed, same scratch
                    assert same_bits(out.v, got), what
                    scr.v.zero_()                                                         # nothing is carried in the scratch
                    out.v.fill_(S)
                    pack_raw(cost.v, gq.v, gs, block, tc, B, H, D, scr.v, out.v)
                    assert same_bits(out.v, got) and scr.guards_intact() and out.guards_intact(), what
                    first.setdefault((gs, tc is None), got)
                    assert np.array_equal(sh.bits(first[(gs, tc is None)]), sh.bits(got)), what      # both unit widths: the same bits
            assert same_bits(cost.v, cost_np) and same_bits(gq.v, g_np) and cost.guards_intact() and gq.guards_intact()
    assert torch.equal(block, block0) and torch.equal(traj, traj0)


# 2 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(7, 3, 6), (1031, 64, 14)], ids=str)
def test_packed_sums_wrapper_is_the_raw_call(shape):
    B, H, D = shape
    inp = sh.pack_inputs(B, H, D)
    block, traj = dev(sh.as_f32(inp["block"], sh.BLOCK_UNIT)), dev(sh.as_f32(inp["traj"], sh.TRAJ_UNIT))
    for f16, gs in ((False, 1.0), (True, 2.0 ** -6)):
        g_np = sh.as_f32(inp["gq"], sh.GQ_UNIT).astype(np.float16 if f16 else np.float32)
        plan = SimpleNamespace(B=B, H=H, cost=dev(sh.as_f32(inp["cost"], sh.COST_UNIT)), gq=dev(g_np), grad_scale=gs, device=DEV)
        for tc in (None, traj):
            pk = ops.PackedSums(plan, block, tc)
            assert (pk.B, pk.H, pk.D, pk.size) == (B, H, D, 1 + H + H * D)
            out = torch.full((pk.size,), S, device=DEV)
            pk.pack(out)
            raw = torch.full((pk.size,), S, device=DEV)
            scr = torch.full((scratch_floats(H, D),), float("nan"), device=DEV)
            pack_raw(plan.cost, plan.gq, gs, block, tc, B, H, D, scr, raw)
            assert same_bits(out, host(raw)) and same_bits(out, sh.packed_reference(inp, tc is not None, gs)), (shape, f16, tc is not None)
            pk._scratch.fill_(float("nan"))                # what the wrapper's scratch holds between calls does not matter
            out.fill_(S)
            pk.pack(out)
            assert same_bits(out, host(raw)), (shape, f16, tc is not None)


# 3 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("shape", sh.REAL_SHAPES, ids=str)
def test_pack_sums_real_valued_columns_each_on_its_own_scale(shape, f16):
    """Columns scaled by 2^(j % 31 - 20): each is held to depth(B) roundings of ITS OWN sum of magnitudes (sums_helpers.pack_bound), not
    to a bound taken from the largest column."""
    B, H, D = shape
    gs = 2.0 ** -6 if f16 else 1.0
    cost_np, g_np = sh.real_inputs(B, H, D, f16)
    block = dev(sh.as_f32(sh.coded_block_sums(sh.n_blocks(B * H)), sh.BLOCK_UNIT))
    cost, gq = dev(cost_np), dev(g_np)
    out = torch.full((1 + H + H * D,), S, device=DEV)
    scr = torch.full((scratch_floats(H, D),), float("nan"), device=DEV)
    pack_raw(cost, gq, gs, block, None, B, H, D, scr, out)
    got = host(out).astype(np.float64)
    x = np.concatenate([cost_np.astype(np.float64), g_np.astype(np.float64).reshape(B, -1) / gs], 1)       # the stored values, unscaled
    ref = x.sum(0)
    bound = sh.pack_bound(np.abs(x).sum(0), ref, B)
    err = np.abs(got[1:] - ref)
    k = int(np.argmax(err / bound))
    print(f"{shape} fp16={f16}: worst |got - ref| / bound {err[k] / bound[k]:.3f} at column {k} (|ref| {abs(ref[k]):.3g})")
    assert np.isfinite(got).all() and (err <= bound).all(), (shape, f16, k, got[1 + k], ref[k], bound[k])
    assert same_bits(out[:1], sh.as_f32([sh.coded_block_sums(sh.n_blocks(B * H)).sum()], sh.BLOCK_UNIT))


# 4 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sh.REDUCE_NS)
def test_reduce_sum_to_the_bit(n):
    x_np = sh.as_f32(sh.coded_reduce(n), 1.0)
    ref = np.float32(sh.coded_reduce(n).sum())
    for off in (0, 4):                                # one float in: the wide kernel adds everything in its scalar loop
        x = Placed(x_np, off)
        out = torch.full((3,), S, device=DEV)
        for trip in range(2):
            rc = lib().trk_reduce_sum(x.v.data_ptr(), n, out[1:].data_ptr(), stream())
            assert rc == 0, lib().trk_last_error()
            got = host(out)
            assert got[0] == S and got[2] == S, (n, off)
            assert sh.bits(got[1:2])[0] == sh.bits(np.array([ref]))[0], (n, off, trip, float(got[1]), float(ref))
            out[1] = S                                # `out` is overwritten, not accumulated into
        assert same_bits(x.v, x_np) and x.guards_intact(), (n, off)
    assert same_bits(ops.reduce_sum(dev(x_np)), np.array([ref])), n


# 5 -----------------------------------------------------------------------------------------------------------------------------------
def scale_raw(g, s, stride, n, dim, out):
    rc = lib().trk_scale_rows(g.data_ptr(), s.data_ptr(), stride, n, dim, int(g.dtype == torch.float16), out.data_ptr(), stream())
    assert rc == 0, lib().trk_last_error()


@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("n,dim", sh.SCALE_SHAPES)
def test_scale_rows_to_the_bit(n, dim, f16):
    io = torch.float16 if f16 else torch.float32
    for one in (False, True):                         # scale_stride 1: one value per row; 0: ONE value
        g_np, s_np = sh.scale_inputs(n, dim, f16, one_scale=one)
        ref = sh.scale_reference(g_np, s_np)
        for off in (0, 2 if f16 else 4):
            what = (n, dim, f16, one, off)
            g, s = Placed(g_np, off), Placed(s_np, 4 if off else 0)
            out = Placed(((n, dim), io, S), off)
            scale_raw(g.v, s.v, 0 if one else 1, n, dim, out.v)
            bad = np.flatnonzero(sh.bits(host(out.v)).reshape(-1) != sh.bits(ref).reshape(-1))
            assert len(bad) == 0, (what, bad[:8], host(out.v).reshape(-1)[bad[:8]], ref.reshape(-1)[bad[:8]])
            assert out.guards_intact() and same_bits(g.v, g_np) and same_bits(s.v, s_np) and g.guards_intact() and s.guards_intact(), what
            scale_raw(g.v, s.v, 0 if one else 1, n, dim, g.v)                             # out == g
            assert same_bits(g.v, ref) and g.guards_intact() and same_bits(s.v, s_np), what
        # the Python wrapper: a scale shaped like g's rows; one value arrives expanded (every stride 0), as .sum().backward() hands it down
        gd = dev(g_np)
        sd = dev(s_np).expand(n) if one else dev(s_np)
        assert not one or n == 1 or not any(sd.stride())
        got = ops.scale_rows(gd, sd)
        assert got.dtype == io and got.shape == gd.shape and same_bits(got, ref) and same_bits(gd, g_np), (n, dim, f16, one)
        if dim > 1 and n > 1:                         # leading dimensions are rows too
            r2 = n // 2 * 2
            got = ops.scale_rows(gd[:r2].view(2, r2 // 2, dim), sd[:r2].reshape(2, r2 // 2))
            assert same_bits(got.view(r2, dim), ref[:r2]), (n, dim, f16, one)


# 6 -----------------------------------------------------------------------------------------------------------------------------------
W_ALL = (1.0, 1.0, 1.0, 1.0)
UPSTREAM = {
    "sum": lambda c, w: c.sum(),                                         # one expanded value: strides (0, 0)
    "row": lambda c, w: (c.sum(1) * w["b"]).sum(),                       # partially expanded: strides (1, 0)
    "dense": lambda c, w: (c * w["W"]).sum(),
    "transposed": lambda c, w: (c.t() * w["W2"].t()).sum(),              # comes down transposed: not contiguous
    "strided": lambda c, w: c[:, ::2].sum(),                             # zeros in every other column
}
_units = {}


def rollout_unit(name):
    """(ModelHandle, CostHandle, PointSetHandle or None, D) of a unit every build compiles"""
    if name not in _units:
        ps = None
        if name == "ur10":
            kin, spec = tt.unit_case("ur10", "spheres", False, "identity")
        elif name == "dual_panda":
            kin, spec, _ = hp.tree_cost_spec("dual_panda")
        elif name == "panda":
            kin = hp.model("panda_arm_no_gripper")
            spec = hp.panda_cost_spec(hp.gold("cost_spheres3d"), hp.gold("panda_robot"), ee_target=hp.gold("rollout_panda")["target"])
        else:
            kin, pl, po, spec = hp.grasp_panda_setup()
        assert name == "points" or jit.has_matching_unit(kin, spec)          # a bundled unit: nothing is compiled at run time
        h, cm = ops.ModelHandle(kin), ops.CostHandle(spec, DEV)
        if name == "points":
            ps = ops.PointSetHandle(h, pl, po, DEV)
        _units[name] = (h, cm, ps, kin.n_dofs)
    return _units[name]


def route_cost(route, q, h, cm, ps):
    if route == "ctypes":                             # the autograd Function over the ctypes calls
        return ops._Rollout.apply(q, ps.model if ps is not None else h, cm, W_ALL, ps, False)[0]
    if route == "dispatcher":                         # the Python-registered dispatcher op
        return torch.ops.trk.rollout_cost_grad(q, h.uid, cm.uid, list(W_ALL), False, ps.uid if ps is not None else 0)[0]
    native = _lib.torch_ops()                         # the C++ dispatcher op with its own autograd node
    assert native is not None, "libtrk_torch.so is part of the build"
    return native.rollout(q, h.ptr, cm.ptr, *W_ALL, False)[0]


@pytest.mark.parametrize("name,f16,shape", [("ur10", False, (3, 5)), ("ur10", False, (37, 9)), ("dual_panda", False, (3, 5)),
                                            ("dual_panda", False, (37, 9)), ("panda", True, (3, 5)), ("panda", True, (37, 9)),
                                            ("points", False, (37, 9))])
def test_backward_of_the_three_autograd_routes_to_the_bit(name, f16, shape):
    h, cm, ps, D = rollout_unit(name)
    B, H = shape
    rng = np.random.default_rng(100 * B + D)
    q_np = rng.uniform(-1.2, 1.2, (B, H, D)).astype(np.float16 if f16 else np.float32)
    gen = torch.Generator().manual_seed(B + D)
    w = dict(b=torch.rand(B, generator=gen).to(DEV) + 0.5, W=(torch.rand(B, H, generator=gen) - 0.5).to(DEV),
             W2=(torch.rand(H, B, generator=gen) - 0.5).to(DEV).t())
    if ps is None:
        gq = ops.rollout_cost_grad(h, cm, W_ALL, dev(q_np), want_pos=False)[2]
    else:
        gq = ops.rollout_points_cost_grad(ps, cm, W_ALL, dev(q_np), want_pos=False)[2].view(B, H, D)
    gq_np = host(gq)
    assert gq_np.dtype == q_np.dtype and np.isfinite(gq_np.astype(np.float64)).all() and (gq_np != 0).mean() > 0.5
    routes = ("ctypes", "dispatcher") + (("native",) if ps is None else ())        # a point-set rollout has no native op
    for up, f in UPSTREAM.items():
        c0 = torch.zeros(B, H, device=DEV, requires_grad=True)                     # the upstream gradient, formed by torch on the side
        f(c0, w).backward()
        ref = sh.scale_reference(gq_np, host(c0.grad).reshape(-1))
        if up == "strided":
            assert (host(c0.grad)[:, 1::2] == 0).all() and (ref.reshape(B, H, D)[:, 1::2] == 0).all()
        grads = {}
        for route in routes:
            q = dev(q_np).requires_grad_(True)
            cost = route_cost(route, q, h, cm, ps)
            seen = []
            cost.register_hook(lambda g: seen.append((tuple(g.stride()), g.is_contiguous())))
            f(cost, w).backward()
            strides, contiguous = seen[0]
            if up == "sum":
                assert not any(strides), (route, strides)
            elif up == "row":
                assert strides[1] == 0 and strides[0] != 0, (route, strides)
            elif up == "transposed":
                assert not contiguous, (route, strides)
            grads[route] = host(q.grad)
            assert grads[route].dtype == q_np.dtype and grads[route].shape == q_np.shape
            bad = np.flatnonzero(sh.bits(grads[route]).reshape(-1) != sh.bits(ref).reshape(-1))
            assert len(bad) == 0, (name, up, route, bad[:8], grads[route].reshape(-1)[bad[:8]], ref.reshape(-1)[bad[:8]])
        for route in routes[1:]:
            assert np.array_equal(sh.bits(grads[route]), sh.bits(grads[routes[0]])), (name, up, route)
