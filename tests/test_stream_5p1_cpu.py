"""The 5+1 layout of the 6-bit shadow (csrc/shadow_5p1.h) and the rule by which its scan skips a row's low bit (scan_stream.inc,
S51), without a GPU: the host pack / unpack entry points against the 6-bit layout's, and a numpy restatement of the rule --
the key of the best a row can still reach is never worse than its 6-bit key, and no row inside the margin of the k-th best is
skipped whatever valid bound of that k-th best the scan holds."""
import numpy as np
import pytest

from metrovector_amd import gpu as G

L2, IP, COS = 0, 1, 2
DIMS = (1, 64, 65, 128, 129, 200, 768)


@pytest.mark.parametrize("dim", DIMS)
def test_pack_unpack_round_trip_and_the_6_bit_layouts_codes(dim):
    rng = np.random.default_rng(dim)
    rows = 131  # two tiles and three rows
    codes = rng.integers(-31, 32, (rows, dim)).astype(np.int8)
    codes[0] = 31
    codes[1] = -31
    codes[2] = 0
    codes[3] = np.where(np.arange(dim) % 2, 31, -31)
    units = (dim + 127) // 128
    assert G.shadow51_bytes(rows, dim) == 3 * units * 6 * 1024
    packed = G.shadow51_pack(codes)
    assert packed.size == G.shadow51_bytes(rows, dim)
    back = G.shadow51_unpack(packed, rows, dim)
    assert (back == codes).all()
    assert (back == G.shadow6_unpack(G.shadow6_pack(codes), rows, dim)).all()
    # the layout is no larger than the 6-bit one exactly where the scan takes it: dim mod 128 is 0 or above 64
    smaller = G.shadow51_bytes(rows, dim) <= G.shadow6_bytes(rows, dim)
    assert smaller == (dim % 128 == 0 or dim % 128 > 64)
    # the rows behind the last one are zero bytes, and the padding elements carry the code of zero (hi 16, lo 0)
    tile = units * 6 * 1024
    last = packed[2 * tile:3 * tile].reshape(units * 6, 64, 16)
    assert not last[:, 3:, :].any()


def test_where_a_code_sits():
    """one element set in one row: its hi value in the stated plane and bits, its low bit in the stated bit of the lo plane"""
    dim, rows = 256, 64
    for e, row in ((0, 0), (17, 5), (79, 63), (80, 1), (95, 2), (96, 3), (111, 4), (112, 6), (127, 7), (128 + 100, 9)):
        for code in (31, -31, 1):
            codes = np.zeros((rows, dim), np.int8)
            codes[row, e] = code
            base = G.shadow51_pack(np.zeros((rows, dim), np.int8)).astype(np.int64)
            diff = G.shadow51_pack(codes).astype(np.int64) ^ base
            y, y0 = code + 32, 32
            hi, lo = (y >> 1) ^ (y0 >> 1), (y & 1) ^ (y0 & 1)
            u, i, b = e // 128, e % 128, e % 16
            want = np.zeros_like(diff)
            if i < 80:
                want[(u * 5 + i // 16) * 1024 + row * 16 + b] = hi
            else:
                s = hi << (5 * ((i - 80) // 16))
                for p in range(5):
                    want[(u * 5 + p) * 1024 + row * 16 + b] = ((s >> (3 * p)) & 7) << 5
            bit = (i // 32) * 32 + (i % 32) // 4 + 8 * (i % 4)
            want[2 * 5 * 1024 + u * 1024 + row * 16 + bit // 8] = lo << (bit % 8)
            assert (diff == want).all(), (e, row, code)


# ---- the skip rule, restated ----------------------------------------------------------------------------------------------

def _ord(x):
    """mvf_common.h ord_f32: ascending float order as ascending u32, NaN last, -0 = +0"""
    x = (np.asarray(x, np.float32) + np.float32(0)).astype(np.float32)
    b = x.view(np.uint32)
    k = np.where(b >> 31, b ^ np.uint32(0xFFFFFFFF), b ^ np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(x), np.uint32(0xFFFFFFFF), k).astype(np.uint32)


def _unord(k):
    k = np.asarray(k, np.uint32)
    b = np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
    return np.where(k == np.uint32(0xFFFFFFFF), np.float32(np.nan), b.view(np.float32)).astype(np.float32)


def _key(score, metric):
    return _ord(score if metric == L2 else -np.asarray(score, np.float32))


def _score(key, metric):
    s = _unord(key)
    return s if metric == L2 else (-s + np.float32(0)).astype(np.float32)


def _margin_key(kth, delta, metric):
    """margin_key.h"""
    vk, d = _score(kth, metric), np.float32(2) * np.float32(delta)
    with np.errstate(invalid="ignore"):
        return _key((vk + d) if metric == L2 else (vk - d), metric)


def _make_key(D, sr, rn, sq, qn, metric):
    """scan_stream.inc make_key (QSK / S6) of the exact integer D = Q.x6: one rounding to f32, then the float key"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dotf = (D.astype(np.float32) * sr).astype(np.float32) * np.float32(sq)
        if metric == IP:
            sc = dotf
        elif metric == COS:
            den = (np.float32(qn) * rn).astype(np.float32)
            sc = np.where(den > 0, dotf / np.where(den > 0, den, np.float32(1)), np.float32(0)).astype(np.float32)
        else:
            sc = (np.float32(qn) * np.float32(qn) + rn - np.float32(2) * dotf).astype(np.float32)
    return _key(sc, metric)


def _corpus(n, dim, rng):
    x = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    x[7] = 0  # a zero row: s_r = 0
    x[8] *= np.float32(1e-3)
    x[9] *= np.float32(1e3)
    mx = np.abs(x).max(1)
    sr = (mx / np.float32(31)).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        x6 = np.where(sr[:, None] > 0, np.rint(x / np.where(sr > 0, sr, 1)[:, None]), 0).clip(-31, 31).astype(np.int64)
    return x, x6, sr


def _queries(dim, rng):
    q = rng.uniform(-1, 1, (8, dim)).astype(np.float32)
    q[0] = np.abs(q[0]) + np.float32(0.01)    # all positive: P = sum Q
    q[1] = -np.abs(q[1]) - np.float32(0.01)   # all negative: P = 0
    q[2] = 0                                  # all zero: s_q = 0
    q[3] = rng.standard_normal(dim).astype(np.float32) * np.float32(50)
    return q


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_the_skip_rule_never_drops_a_row_inside_the_margin(metric):
    n, dim, k = 20_000, 72, 100
    rng = np.random.default_rng(51 + metric)
    x, x6, sr = _corpus(n, dim, rng)
    y = x6 + 32
    hi, lo = y >> 1, y & 1
    assert ((2 * hi + lo) == y).all() and hi.min() >= 0 and hi.max() <= 31
    xn = np.sqrt((x.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    rn = (xn * xn).astype(np.float32) if metric == L2 else xn  # ScanParams::xrow: sum x^2 (L2) / |x| (Cosine)
    for qi, q in enumerate(_queries(dim, rng)):
        mx = np.abs(q).max()
        sq = np.float32(mx / np.float32(16256)) if mx > 0 else np.float32(0)
        Q = np.rint(q / sq).clip(-16256, 16256).astype(np.int64) if sq > 0 else np.zeros(dim, np.int64)
        qn = np.float32(np.sqrt((q.astype(np.float64) ** 2).sum()))
        P, bias = int(np.maximum(Q, 0).sum()), 32 * int(Q.sum())
        D6 = y @ Q - bias                      # = Q.x6, what the 6-bit unit rounds
        assert (D6 == x6 @ Q).all()
        Dbest = 2 * (hi @ Q) + P - bias        # phase 1 of the 5+1 unit: known before the low plane is read
        assert (Dbest >= D6).all() and (Dbest - D6 <= int(np.abs(Q).sum())).all()  # Q.lo lies in [sum min(Q, 0), P]
        key6 = _make_key(D6, sr, rn, sq, qn, metric)
        kbest = _make_key(Dbest, sr, rn, sq, qn, metric)
        assert (kbest <= key6).all(), f"metric {metric} query {qi}: key_best is worse than the 6-bit key of a row"
        order = np.sort(key6)
        kth = order[k - 1]
        lo16, hi84 = np.percentile(_score(key6, metric).astype(np.float64), (16, 84))
        sigma = float(hi84 - lo16) / 2  # the spread of the ordinary rows' scores (rows 8 and 9 are scaled a thousandfold)
        for delta in (0.0, 0.25 * sigma, 0.5 * sigma, 3.0 * sigma):
            tkey = _margin_key(kth, delta, metric)          # what select_final's margin mode keeps: key <= tkey
            inside = key6 <= tkey
            assert inside.sum() >= k
            # every valid bound the scan can hold: the k-th best of ANY k rows' keys lies at or behind the true k-th best -- the
            # true one, its 4096-key bucket's worse end (the scan's rounding), the k-th of a sample of the rows, and far weaker ones
            sample = np.sort(key6[rng.choice(n, 40 * k, replace=False)])[k - 1]
            for bound in (kth, kth | np.uint32(0xFFF), sample, sample | np.uint32(0xFFF), order[10 * k], order[-1], np.uint32(0xFFFFFFFF)):
                assert bound >= kth
                kskip = _margin_key(np.uint32(bound), delta, metric)
                assert kskip >= tkey, "a weaker bound gave a tighter skip key"
                skipped = kbest > kskip
                assert not (skipped & inside).any(), f"metric {metric} query {qi} delta {delta}: a row inside the margin is skipped"
            if qi == 4 and delta == 0.5 * sigma:  # the rule does skip on ordinary rows (the GPU tests count the lines)
                assert (kbest > _margin_key(kth | np.uint32(0xFFF), delta, metric)).mean() > 0.5
