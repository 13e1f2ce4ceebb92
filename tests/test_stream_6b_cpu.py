"""The 6-bit shadow stream without a GPU: the shape rule that sends ONE Float32 query over the 6-bit shadow, the shadow's
layout through the library's host pack / unpack, and the proven bound restated in numpy (csrc/shadow_6b.hip,
csrc/query_16s.h): |approximate score - exact score| <= delta for EVERY row."""
import math

import numpy as np
import pytest

from metrovector_amd import gpu as G

SEED = 0x4D564631
L2, IP, COS = 0, 1, 2
F32, F16, I8 = 0, 1, 2


# ---- the shape rule ------------------------------------------------------------------------------------------------------

def test_which_shadow_a_single_query_streams_is_a_function_of_its_shape():
    for metric in (L2, IP, COS):
        assert G.stream_bits(10_000_000, 768, F32, metric, 1, 100) == 6   # the headline
    assert G.stream_bits(10_000_000, 768, F32, COS, 1, 1) == 6
    assert G.stream_bits(10_000_000, 768, F32, COS, 1, 204) == 8          # ~9 400 rows predicted inside the margin: more than half the capacity
    assert G.stream_bits(10_000_000, 1024, F32, COS, 1, 100) == 8         # ~9 100
    assert G.stream_bits(400_000, 768, F32, COS, 1, 100) == 8             # 1.2 GB: under the size threshold
    assert G.stream_bits(16_400, 8192, F32, COS, 1, 100) == 8             # 537 MB of long rows
    assert G.stream_bits(10_000_000, 768, F32, COS, 1, 205) == 0          # beyond the streamed selection's k
    assert G.stream_bits(100_000, 768, F32, COS, 1, 100) == 0             # under the int8 threshold too
    assert G.stream_bits(10_000_000, 768, F16, COS, 1, 100) == 0
    assert G.stream_bits(10_000_000, 768, I8, IP, 1, 100) == 0
    assert G.stream_bits(10_000_000, 768, F32, COS, 2, 100) == 0
    # the int8 rule is the older entry point's, unchanged
    for shape in ((10_000_000, 768, F32, COS, 1, 100), (400_000, 768, F32, COS, 1, 100), (10_000_000, 768, F16, COS, 1, 100)):
        assert (G.stream_bits(*shape) != 0) == (G.stream_rows(*shape) == 1)


# ---- the layout ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 63, 64, 65, 768, 1000])
def test_pack_unpack_round_trip(dim):
    rng = np.random.default_rng(dim)
    rows = 131  # two whole tiles and three rows
    codes = rng.integers(-31, 32, (rows, dim), dtype=np.int8)
    codes[0], codes[1], codes[-1] = -31, 31, 0
    shadow = G.shadow6_pack(codes)
    units = (dim + 63) // 64
    assert shadow.size == G.shadow6_bytes(rows, dim) == 3 * units * 3072  # ceil(131 / 64) tiles of `units` x 3 KiB
    assert (G.shadow6_unpack(shadow, rows, dim) == codes).all()
    # the layout itself: plane p of unit u of the tile's 64 rows is one KiB, row r at byte 16 r; every code a non-negative 6-bit value
    tiles = shadow.reshape(3, units, 3, 64, 16)
    r, e = 70, min(dim - 1, 5)
    assert tiles[r // 64, e // 64, (e % 64) // 16, r % 64, e % 16] & 63 == int(codes[r, e]) + 32
    if dim > 48:
        y = int(codes[r, 48]) + 32  # element 48 of unit 0: the top two bits of byte 0 of the three planes
        assert [int(tiles[1, 0, p, r % 64, 0]) >> 6 for p in range(3)] == [y & 3, (y >> 2) & 3, (y >> 4) & 3]
    assert (tiles[2, :, :, 3:, :] == 0).all()  # the rows behind the last one


def test_pack_refuses_codes_outside_six_bits():
    from metrovector_amd.errors import MvfError
    with pytest.raises(MvfError):
        G.shadow6_pack(np.full((2, 8), 32, np.int8))


# ---- the bound -------------------------------------------------------------------------------------------------------------

def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _shadow6(x):
    """shadow_6b_kernel: codes, s_r and the four corpus-wide maxima, in f32 as the kernel evaluates them."""
    sr = _f32(np.abs(x).max(axis=1) / np.float32(31))
    t = _f32(x / sr[:, None])
    q = np.clip(np.rint(t), -31, 31).astype(np.float32)
    e = _f32(t - q)
    ex = _f32(np.sqrt(_f32((e * e).sum(1))) * np.float32(1.0005) + np.float32(1e-3))
    xa = _f32(np.sqrt(_f32((q * q).sum(1))) * np.float32(1.0005) + ex)
    xn = _f32(np.sqrt(_f32((x * x).sum(1))))
    a, b = _f32(sr * xa), _f32(sr * ex)
    stats = [a.max(), b.max(), _f32(a / xn * np.float32(1.000001)).max(), _f32(b / xn * np.float32(1.000001)).max()]
    return q.astype(np.int64), sr, [np.float32(s) for s in stats], xn


def _query16(q):
    """prep_query_16s: Q = 128 hi + lo, s_q, |Q|, |eq|."""
    sq = np.float32(np.abs(q).max() / np.float32(16256))
    t = _f32(q / sq)
    Q = np.clip(np.rint(t), -16256, 16256).astype(np.float32)
    e = _f32(t - Q)
    Qi = Q.astype(np.int64)
    lo = ((Qi + 64) & 127) - 64
    hi = (Qi - lo) >> 7
    assert (np.abs(hi) <= 127).all() and (lo >= -64).all() and (lo <= 63).all() and (128 * hi + lo == Qi).all()
    eq = np.float32(np.sqrt(np.float32((e * e).sum())) * np.float32(1.0005) + np.float32(1e-3))
    qqn = np.float32(np.sqrt(np.float32((Q * Q).sum())) * np.float32(1.0005))
    return lo, hi, sq, qqn, eq


@pytest.mark.parametrize("dim", [64, 768])
def test_the_bound_holds_for_every_row(oracle, dim):
    n = 20_000
    x = np.ascontiguousarray(oracle.synth_rows(SEED, 0, n, dim, F32)).astype(np.float32)
    queries = oracle.synth_queries(SEED + 1, 4, dim, F32).astype(np.float32).copy()
    queries[3] = x[17]  # a stored row as the query
    x6, sr, stats, xn = _shadow6(x)
    y = x6 + 32  # the stored codes
    xx = _f32((x * x).sum(1))
    xxmax = np.float32(xx.max())
    x64 = x.astype(np.float64)
    for q in queries:
        lo, hi, sq, qqn, eq = _query16(q)
        qn = np.float32(np.sqrt(np.float32((q * q).sum())))
        ss = np.float32((q * q).sum())
        # the scan: two exact integer sums over the codes, the exact combine, ONE rounding, then two f32 products
        combined = 128 * (y @ hi) + (y @ lo) - 32 * int((128 * hi + lo).sum())
        assert (combined == x6 @ (128 * hi + lo)).all()
        dotf = _f32(_f32(_f32(combined) * sr) * sq)
        exact_dot = x64 @ q.astype(np.float64)
        d_ip = np.float32(sq * (eq * stats[0] + qqn * stats[1]) * np.float32(1.0001) + np.float32(6e-7) * qn * np.float32(math.sqrt(xxmax)))
        assert (np.abs(dotf.astype(np.float64) - exact_dot) <= d_ip).all(), f"InnerProduct, dim {dim}"
        d_cos = np.float32(sq * (eq * stats[2] + qqn * stats[3]) / qn * np.float32(1.0001) + np.float32(6e-7))
        approx_cos = _f32(dotf / _f32(qn * xn))
        exact_cos = exact_dot / (np.sqrt((q.astype(np.float64) ** 2).sum()) * np.sqrt((x64 ** 2).sum(1)))
        assert (np.abs(approx_cos.astype(np.float64) - exact_cos) <= d_cos).all(), f"Cosine, dim {dim}"
        d_l2 = np.float32(np.float32(2) * d_ip + np.float32(4e-7) * (ss + xxmax))
        approx_l2 = _f32(_f32(_f32(qn * qn) + xx) - _f32(np.float32(2) * dotf))
        exact_l2 = ((x64 - q.astype(np.float64)[None, :]) ** 2).sum(1)
        assert (np.abs(approx_l2.astype(np.float64) - exact_l2) <= d_l2).all(), f"L2, dim {dim}"
