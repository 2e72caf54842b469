"""CPU-only checks of what tests/test_gpu_sums.py feeds trk_pack_sums, trk_reduce_sum and trk_scale_rows (tests/sums_helpers.py): the coded
inputs are exactly summable in fp32 in any order at every shape of the GPU tests, their reference notices a dropped row, a swapped pair
of columns and an H / D-transposed read, and an fp32 restatement of the association order include/trk.h documents stays within the
per-column bound the real-valued test applies.  No kernel is run here: this is about the inputs and the references."""
import numpy as np
import pytest

import sums_helpers as sh


@pytest.mark.parametrize("shape", sh.PACK_SHAPES, ids=str)
def test_coded_pack_inputs_are_exactly_summable(shape):
    B, H, D = shape
    inp = sh.pack_inputs(B, H, D)
    for a in inp.values():
        assert (a % 2 != 0).all() and (a != 0).all()                      # odd: no element can leave or join a sum unnoticed
    assert inp["cost"].shape == (B, H) and inp["gq"].shape == (B, H, D) and len(inp["block"]) == sh.n_blocks(B * H) and len(inp["traj"]) == B
    total, c, g = sh.pack_magnitudes(inp)
    print(f"{shape}: sum of magnitudes in units: packed[0] {total}, cost column {c}, gradient column {g} (limit {sh.EXACT_LIMIT})")
    assert max(total, c, g) < sh.EXACT_LIMIT
    # an fp16 gradient holds the coded values themselves (times GQ_UNIT): integers far below 2048, exact in fp16
    assert np.abs(inp["gq"]).max() <= 2048
    g16 = sh.as_f32(inp["gq"], sh.GQ_UNIT).astype(np.float16)
    assert np.array_equal(g16.astype(np.float64), inp["gq"] * sh.GQ_UNIT)
    for gs in sh.PACK_GRAD_SCALES:
        for with_traj in (False, True):
            ref = sh.packed_reference(inp, with_traj, gs)                  # asserts that the conversion to fp32 is exact
            assert ref.shape == (1 + H + H * D,) and np.isfinite(ref).all()
    # block_sums is not the block sums of cost: a kernel that summed `cost` for packed[0] would be caught
    assert sh.packed_units(inp, False)[0] * min(sh.BLOCK_UNIT, sh.TRAJ_UNIT) != inp["cost"].sum() * sh.COST_UNIT
    assert sh.packed_reference(inp, True)[0] != sh.packed_reference(inp, False)[0]


@pytest.mark.parametrize("shape", sh.PACK_SHAPES, ids=str)
def test_coded_pack_reference_notices_indexing_errors(shape):
    B, H, D = shape
    inp = sh.pack_inputs(B, H, D)
    ref = sh.packed_reference(inp, True)[1:]
    C = H + H * D
    # a dropped row: every column changes (every value is odd)
    short = dict(inp, cost=inp["cost"][:-1], gq=inp["gq"][:-1])
    if B > 1:
        assert (sh.packed_reference(short, True)[1:] != ref).all()
    else:
        assert (ref != 0).all()
    # a swapped pair of adjacent columns
    if C > 1:
        differ = float((ref[1:] != ref[:-1]).mean())
        print(f"{shape}: adjacent columns differ in {100 * differ:.1f} % of {C - 1} places")
        # Every pair differs at the seven shapes below B = 1024.  From there on whole periods of the 20-periodic gradient code cancel,
        # B mod 20 rows decide a column, and a few neighbours tie: 4 of 91 pairs at (1024, 4, 22), 63 of 959 at (1031, 64, 14), 127 of
        # 1919 at (1025, 128, 14) -- at least 93 % of the pairs differ at every shape.
        assert differ >= 0.9 and (B >= 1000 or differ == 1.0)
    # a gradient row read as (D, H) instead of (H, D)
    if H > 1 and D > 1:
        _, _, gt = sh.packed_units(inp, True, gq=inp["gq"].reshape(B, D, H).transpose(0, 2, 1))
        moved = float((gt != sh.packed_units(inp, True)[2]).mean())
        print(f"{shape}: the H / D-transposed read changes {100 * moved:.1f} % of the gradient columns")
        assert moved >= 0.8


@pytest.mark.parametrize("n", sh.REDUCE_NS)
def test_coded_reduce_inputs_are_exactly_summable(n):
    x = sh.coded_reduce(n)
    assert (x % 2 != 0).all() and np.abs(x).max() <= 7 and int(np.abs(x).sum()) < sh.EXACT_LIMIT
    ref = np.float32(x.sum())
    assert float(ref) == float(x.sum())
    if n > 1:                                                             # the last element and an element twice are both visible
        assert np.float32(x[:-1].sum()) != ref and np.float32(x.sum() + x[n // 2]) != ref
    # the alignment the wide kernel's loops are tested at: whole float4s, then 1 .. 3 floats of tail
    assert {m % 4 for m in sh.REDUCE_NS if m > 65536} == {0, 1, 3}


@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("shape", sh.REAL_SHAPES, ids=str)
def test_documented_association_order_meets_the_real_valued_bound(shape, f16):
    """Part 3's bound, derived from the depth of the documented order, holds for that order carried out in numpy fp32"""
    B, H, D = shape
    gs = 2.0 ** -6 if f16 else 1.0
    cost, gq = sh.real_inputs(B, H, D, f16)
    x = np.concatenate([cost, gq.reshape(B, -1).astype(np.float32)], 1)
    unscale = np.concatenate([np.ones(H), np.full(H * D, 1.0 / gs)])
    got = sh.pack_columns_f32(x) * unscale.astype(np.float32)
    ref = x.astype(np.float64).sum(0) * unscale
    bound = sh.pack_bound(np.abs(x.astype(np.float64)).sum(0) * unscale, ref, B)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{shape} fp16={f16}: depth {sh.pack_depth(B)}, worst |got - ref| / bound {float((err / bound).max()):.3f}")
    assert (bound > 0).all() and (err <= bound).all()
    # the columns are on their own scales: the bound of the smallest column is orders of magnitude below the largest one's
    assert bound.min() < 1e-6 * bound.max()


@pytest.mark.parametrize("B,slices,rows_per", [(1, 1, 1), (8, 1, 8), (9, 2, 5), (1023, 128, 8), (1024, 128, 8), (1025, 128, 9), (1031, 128, 9)])
def test_slice_arithmetic(B, slices, rows_per):
    assert sh.pack_slices(B) == (slices, rows_per)
    assert slices * rows_per >= B
    assert sh.pack_depth(B) == -(-rows_per // 8) + 3 + -(-slices // 8) + 8
    # on the coded inputs the restated order is exact as well: it gives the integer reference
    inp = sh.pack_inputs(B, 3, 2)
    x = np.concatenate([sh.as_f32(inp["cost"], sh.COST_UNIT), sh.as_f32(inp["gq"], sh.GQ_UNIT).reshape(B, -1)], 1)
    assert np.array_equal(sh.pack_columns_f32(x), sh.packed_reference(inp, True)[1:])


@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
def test_scale_rows_reference(f16):
    for n, dim in sh.SCALE_SHAPES:
        for one in (False, True):
            g, s = sh.scale_inputs(n, dim, f16, one_scale=one)
            ref = sh.scale_reference(g, s)
            assert ref.dtype == g.dtype and ref.shape == g.shape and np.isfinite(ref.astype(np.float64)).all()
            assert len(s) == (1 if one else n)
    if f16:
        got = {(gv, sv): sh.scale_reference(np.array([[gv]], np.float16), np.array([sv], np.float32))[0, 0] for gv, sv in sh.F16_SPECIALS}
        assert got[(683.0, 3.0)] == 2048 and got[(293.0, 7.0)] == 2052 and got[(-683.0, 3.0)] == -2048       # ties go to even
        sub = [v for v in got.values() if 0 < abs(float(v)) < 2.0 ** -14]
        assert len(sub) >= 2                                                                                  # fp16 subnormals
        assert got[(3.0 * 2.0 ** -14, 2.0 ** -11)] == np.float16(2.0 ** -23)                                 # 1.5 x 2^-24: a tie between subnormals
        zeros = [v for v in got.values() if float(v) == 0.0]
        assert len(zeros) >= 3 and all(np.signbit(v) for v in zeros)                                          # negative zeros, one by underflow
        g, s = sh.scale_inputs(37, 7, True)
        assert np.array_equal(sh.bits(sh.scale_reference(g, s))[:len(sh.F16_SPECIALS), 0], sh.bits(np.array(list(got.values()), np.float16)))
