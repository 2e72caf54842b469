"""Inputs and references of the packing (trk_pack_sums), reduction (trk_reduce_sum) and row-scaling (trk_scale_rows) tests
(tests/test_sums_refs_cpu.py, tests/test_gpu_sums.py).  numpy only: nothing here touches the library.

Every coded input is an ODD integer that is a function of its indices, times a power-of-two unit.  While the sum of the magnitudes of
a summed set stays below 2^24 units, every partial sum in ANY association order is an integer of fewer than 24 bits -- exact in fp32 --
so the correct fp32 result is the int64 sum converted once, and a test can ask for its bits.  No value is zero and every value is odd:
one dropped or doubled element changes its sum."""
import numpy as np

# (B, H, D): B = 1; 8 / 9 (one row slice becomes two); 1023 / 1024 / 1025 / 1031 (the 128-slice cap, then empty trailing slices);
# H = 1, 3, 5, 6, 65 (scalar units) and 4, 64, 128 (16-byte units); (8, 4, 15): 16 units; (129, 64, 7): 128 units = two full tiles;
# (9, 5, 12): 65 units = one in the second tile; D = 1, 6, 7, 12, 14, 15, 22
PACK_SHAPES = [(1, 1, 1), (7, 3, 6), (8, 4, 15), (9, 5, 12), (37, 6, 7), (129, 64, 7), (1023, 65, 1), (1024, 4, 22), (1025, 128, 14),
               (1031, 64, 14)]
REAL_SHAPES = [(37, 6, 7), (1025, 128, 14), (129, 64, 7)]          # the real-valued columns of part 3
PACK_GRAD_SCALES = (1.0, 2.0 ** -6, 8.0)                            # of an fp16 gradient: powers of two, 1 / scale and the product are exact
# 65536 is the last launch of the 256-thread kernel; 98304 floats = 24576 float4 = three trips of the eight-in-flight loop
REDUCE_NS = [1, 2, 255, 256, 257, 1000, 65535, 65536, 65537, 65540, 65543, 98304, 98305, 98307, 98304 + 4 * 1023 + 3, 1 << 20, (1 << 20) + 1]
SCALE_SHAPES = [(1, 1), (37, 7), (256, 1), (257, 3), (1000, 14), (4099, 22)]      # (n, dim): one thread per element, 256 per workgroup

# units: powers of two, one per array, so that no array is summed in the unit another one is read in
COST_UNIT, GQ_UNIT, BLOCK_UNIT, TRAJ_UNIT = 2.0 ** -3, 2.0 ** -5, 2.0 ** -2, 2.0 ** -1
EXACT_LIMIT = 1 << 24


def n_blocks(n_samples):
    """length of the rollout's cost_block_sums: one entry per 64 samples (include/trk.h)"""
    return (int(n_samples) + 63) // 64


def coded_gq(B, H, D):
    b, h, d = np.meshgrid(np.arange(B, dtype=np.int64), np.arange(H, dtype=np.int64), np.arange(D, dtype=np.int64), indexing="ij")
    return 2 * ((131 * b + 31 * h + 7 * d + 3) % 20) - 19


def coded_cost(B, H):
    b, h = np.meshgrid(np.arange(B, dtype=np.int64), np.arange(H, dtype=np.int64), indexing="ij")
    return 2 * ((17 * b + 5 * h + 1) % 16) - 15


def coded_block_sums(nb):
    """deliberately NOT the block sums of coded_cost: packed[0] must come from the array the call was given"""
    return 2 * ((7 * np.arange(nb, dtype=np.int64) + 2) % 2000) - 1999


def coded_traj_cost(B):
    return 2 * ((3 * np.arange(B, dtype=np.int64) + 1) % 500) - 499


def coded_reduce(n):
    """odd values in [-7, 7]"""
    return 2 * ((5 * np.arange(n, dtype=np.int64) + 3) % 8) - 7


def as_f32(units, unit):
    """integers times a power-of-two unit: exact"""
    return (np.asarray(units, np.int64).astype(np.float64) * unit).astype(np.float32)


def pack_inputs(B, H, D):
    """dict of the coded integer arrays of a shape: cost (B, H), gq (B, H, D), block (n_blocks(B H),), traj (B,)"""
    return dict(cost=coded_cost(B, H), gq=coded_gq(B, H, D), block=coded_block_sums(n_blocks(B * H)), traj=coded_traj_cost(B))


def packed_units(inp, with_traj, gq=None):
    """the int64 sums behind packed [1 + H + H D]: -> (total in units of min(BLOCK_UNIT, TRAJ_UNIT), cost columns in COST_UNIT,
    gradient columns in GQ_UNIT)"""
    u = min(BLOCK_UNIT, TRAJ_UNIT)
    total = int(inp["block"].sum()) * int(BLOCK_UNIT / u) + (int(inp["traj"].sum()) * int(TRAJ_UNIT / u) if with_traj else 0)
    g = inp["gq"] if gq is None else gq
    return total, inp["cost"].sum(0), g.sum(0).reshape(-1)


def packed_reference(inp, with_traj, grad_scale=1.0):
    """fp32 packed [1 + H + H D] of the coded inputs: each int64 sum converted to fp32 ONCE; the gradient columns hold grad_scale x the
    gradient and are divided by it (a power of two: exact)"""
    total, c, g = packed_units(inp, with_traj)
    u = min(BLOCK_UNIT, TRAJ_UNIT)
    out = np.concatenate([[total * u], c.astype(np.float64) * COST_UNIT, g.astype(np.float64) * GQ_UNIT / grad_scale])
    out32 = out.astype(np.float32)
    assert np.array_equal(out32.astype(np.float64), out)            # the conversion itself is exact
    return out32


def pack_magnitudes(inp):
    """the sum of magnitudes, in units, of every set that trk_pack_sums adds up: (total with traj_cost, largest cost column, largest
    gradient column) -- each must stay below EXACT_LIMIT"""
    u = min(BLOCK_UNIT, TRAJ_UNIT)
    total = int(np.abs(inp["block"]).sum()) * int(BLOCK_UNIT / u) + int(np.abs(inp["traj"]).sum()) * int(TRAJ_UNIT / u)
    return total, int(np.abs(inp["cost"]).sum(0).max()), int(np.abs(inp["gq"]).sum(0).max())


# ---------------------------------------------------------------------------------------------------------------------------
# the association order include/trk.h documents for trk_pack_sums, from B alone
# ---------------------------------------------------------------------------------------------------------------------------
def pack_slices(B):
    """(row slices, rows per slice): slices = min(128, ceil(B / 8)), rows_per = ceil(B / slices); beyond B = 1024 trailing slices are empty"""
    slices = max(1, min(128, (B + 7) // 8))
    return slices, (B + slices - 1) // slices


def pack_depth(B):
    """the most additions a column's value passes through: a row lane's rows of a slice in sequence (ceil(rows_per / 8)), the tree over
    the 8 row lanes (3), a group's slices in sequence (ceil(slices / 8)), the 8 groups in sequence (8)"""
    slices, rows_per = pack_slices(B)
    return (rows_per + 7) // 8 + 3 + (slices + 7) // 8 + 8


def pack_bound(abs_colsum, ref, B):
    """|got - ref| <= depth 2^-24 sum_b |x[b, col]| (1 + 2^-10) + 2^-24 |ref| per column: `depth` roundings of partial sums that never
    exceed the sum of magnitudes (the factor 1 + 2^-10 covers the second-order terms), and the rounding of the unscale product"""
    u = 2.0 ** -24
    return pack_depth(B) * u * np.asarray(abs_colsum, np.float64) * (1.0 + 2.0 ** -10) + u * np.abs(np.asarray(ref, np.float64))


def pack_columns_f32(x, unscale=1.0):
    """The documented association order restated in numpy fp32 on a matrix x (B, C): every slice's rows b0 + rl, b0 + rl + 8, ... in
    sequence per row lane rl, the eight lanes as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)); then the slices g per .. (g + 1) per - 1 in
    sequence per group g, the eight groups in sequence; the result times `unscale`.  -> (C,) fp32"""
    x = np.asarray(x, np.float32)
    B, C = x.shape
    slices, rows_per = pack_slices(B)
    partial = np.zeros((slices, C), np.float32)
    for s in range(slices):
        b0, b1 = s * rows_per, min(B, (s + 1) * rows_per)
        lane = np.zeros((8, C), np.float32)
        for rl in range(8):
            for b in range(b0 + rl, b1, 8):
                lane[rl] = lane[rl] + x[b]
        partial[s] = ((lane[0] + lane[1]) + (lane[2] + lane[3])) + ((lane[4] + lane[5]) + (lane[6] + lane[7]))
    per = (slices + 7) // 8
    tot = np.zeros(C, np.float32)
    for g in range(8):
        acc = np.zeros(C, np.float32)
        for p in range(g * per, min(slices, (g + 1) * per)):
            acc = acc + partial[p]
        tot = tot + acc
    return tot * np.float32(unscale)


def real_inputs(B, H, D, f16, seed=0):
    """Part 3: normal draws with column j of the C = H + H D columns scaled by 2^(j % 31 - 20) -> (cost (B, H) fp32, gq (B, H, D) fp32 or
    fp16 as STORED, i.e. rounded to the storage type)"""
    rng = np.random.default_rng(seed + 1000 * B + H)
    C = H + H * D
    x = rng.standard_normal((B, C)) * 2.0 ** (np.arange(C) % 31 - 20)
    cost = x[:, :H].astype(np.float32)
    gq = x[:, H:].reshape(B, H, D).astype(np.float16 if f16 else np.float32)
    return cost, gq


# ---------------------------------------------------------------------------------------------------------------------------
# trk_scale_rows
# ---------------------------------------------------------------------------------------------------------------------------
# (g, scale) whose fp16 product is decided by the rounding: two exact ties (2049 -> 2048, 2051 -> 2052: to even), results in the
# fp16 subnormal range (one of them a tie between two subnormals), an underflow to zero, and negative zeros
F16_SPECIALS = [(683.0, 3.0), (293.0, 7.0), (2.0 ** -10, 1.3 * 2.0 ** -10), (3.0 * 2.0 ** -14, 2.0 ** -11), (-2.0 ** -14, 2.0 ** -20),
                (-0.0, 5.0), (1.5, -0.0), (-683.0, 3.0)]


def scale_inputs(n, dim, f16, seed=0, one_scale=False):
    """g (n, dim) fp32 / fp16 and scale (n,) fp32 -- (1,) with one_scale -- for trk_scale_rows: seeded draws, every fp16 product well inside
    the fp16 range; in fp16 the first rows start with the constructed pairs of F16_SPECIALS (with one scale: those whose scale is 3)"""
    rng = np.random.default_rng(seed + 100 * n + dim)
    g = rng.standard_normal((n, dim)).astype(np.float16 if f16 else np.float32)
    s = (rng.uniform(0.25, 4.0, 1 if one_scale else n) * rng.choice([-1.0, 1.0], 1 if one_scale else n)).astype(np.float32)
    if f16:
        if one_scale:
            s[0] = 3.0
            for k, gv in enumerate([gv for gv, sv in F16_SPECIALS if sv == 3.0][:n * dim]):
                g.reshape(-1)[k] = gv
        else:
            for r, (gv, sv) in enumerate(F16_SPECIALS[:n]):
                g[r, 0], s[r] = gv, sv
    return g, s


def scale_reference(g, s):
    """What one fp32 multiply gives: the correctly rounded product (an fp64 product of two fp32 values is exact, so the conversion is the
    only rounding); fp16 rows are widened, multiplied in fp32 and rounded to fp16 once more.  s: (n,) or (1,) or shaped like g's rows."""
    g = np.asarray(g)
    s = np.broadcast_to(np.asarray(s, np.float32).reshape(-1), (g.size // g.shape[-1],)).reshape(g.shape[:-1] + (1,))
    if g.dtype == np.float16:
        return (g.astype(np.float32) * s).astype(np.float16)
    return (g.astype(np.float64) * s.astype(np.float64)).astype(np.float32)


def bits(a):
    """the bit patterns of an fp32 / fp16 array, for comparisons that tell -0 from +0"""
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int16)
