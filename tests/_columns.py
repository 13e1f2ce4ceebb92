"""Helpers of the column-filter tests (DESIGN.md §3 "Column filters") and a numpy restatement of the semantics: the value of a
row is zero-extended to u64, every comparison is unsigned 64-bit, a row is admitted iff its clauses -- combined by all / any --
hold, the base filter (if any) admits it and it is not deleted.  Python integers do the arithmetic, so 2^64 - 1 is exact."""
import numpy as np

U32, U64 = 4, 5  # schema/types.fbs
TOP = 2 ** 64 - 1
NP_OF = {U32: np.uint32, U64: np.uint64}
OPS = ["==", "!=", "<", "<=", ">", ">=", "between", "in", "not in"]
OP_CODE = {op: i for i, op in enumerate(OPS)}  # include/mvf_gpu.h MVFGPU_OP_*


def clause_mask(values, op, operand):
    """bool[n]: the clause over a column's values (uint32 / uint64 array)."""
    v = np.asarray(values).astype(np.uint64)
    u = np.uint64
    if op == "==":
        return v == u(operand)
    if op == "!=":
        return ~clause_mask(values, "==", operand)
    if op == "<":
        return v < u(operand)
    if op == "<=":
        return v <= u(operand)
    if op == ">":
        return v > u(operand)
    if op == ">=":
        return v >= u(operand)
    if op == "between":
        lo, hi = operand
        return (v >= u(lo)) & (v <= u(hi))  # a > b: nothing
    if op == "in":
        return np.isin(v, np.array(list(operand), dtype=np.uint64))  # no values: nothing
    if op == "not in":
        return ~clause_mask(values, "in", operand)
    raise ValueError(op)


def where_mask(clauses, any=False, base=None, dead=None):  # noqa: A002
    """bool[n] of [(values, op, operand), ...]: the rows a where-filter admits."""
    masks = [clause_mask(v, op, operand) for v, op, operand in clauses]
    m = np.logical_or.reduce(masks) if any else np.logical_and.reduce(masks)
    if base is not None:
        m = m & base
    if dead is not None:
        m = m & ~dead
    return m


def range_of(data_type, op, a, b=0):
    """(lo, hi, negate) of the host-side normalisation: lo <= v <= hi over the type's values, negated for "!="; an empty
    range is (1, 0)."""
    tmax = 2 ** 32 - 1 if data_type == U32 else TOP
    lo, hi = {"==": (a, a), "!=": (a, a), "<": (0, a - 1), "<=": (0, a), ">": (a + 1, TOP), ">=": (a, TOP), "between": (a, b)}[op]
    hi = min(hi, tmax)
    if lo > hi:  # "< 0" gives hi = -1, "> 2^64 - 1" gives lo = 2^64
        lo, hi = 1, 0
    return lo, hi, 1 if op == "!=" else 0


def edge_values(n, data_type, rng, lo=1000, hi=2000):
    """Column values in which every comparison with operands around lo .. hi has admitted and refused rows at both ends of
    every 32-row word: the first and last two rows of each word alternate between a value below `lo`, `lo` itself, a value
    inside, `hi` itself and a value above; the rest is random around the range."""
    v = rng.integers(lo - 300, hi + 300, n).astype(np.uint64)
    pattern = [lo - 1, lo, (lo + hi) // 2, hi, hi + 1]
    for w in range((n + 31) // 32):
        for j, r in enumerate((32 * w, 32 * w + 1, 32 * w + 30, 32 * w + 31)):
            if r < n:
                v[r] = pattern[(w + j) % 5] if j % 2 == 0 else pattern[(w + j + 2) % 5]
    return v.astype(NP_OF[data_type])


def odd_address(values):
    """The same values in a buffer that starts at an odd byte address: (keep-alive, address)."""
    raw = np.ascontiguousarray(values).view(np.uint8)
    buf = np.zeros(raw.size + 16, np.uint8)
    off = 1 if buf.ctypes.data % 2 == 0 else 2
    buf[off:off + raw.size] = raw
    assert (buf.ctypes.data + off) % 2 == 1
    return buf, buf.ctypes.data + off
