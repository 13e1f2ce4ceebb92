"""Radius-search expectations from the oracle's score of every row ("Radius search")."""
import numpy as np

from _util import TOL, norms

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)


def oracle_radius(oracle, rows, dtype, metric, query, radius, max_per_query, dead=None, index_base=0, ids=None):
    """The match rule over every row: (count, scores[max], indices[max], raw[max]) with the library's padding; best
    first by the oracle's order key, ties by position."""
    sc, keys, raw = oracle.scores(rows, dtype, metric, query)
    live = ~np.isnan(sc)
    if dead is not None:
        live &= ~dead
    hit = live & ((sc <= np.float32(radius)) if metric == 0 else (sc >= np.float32(radius)))
    pos = np.nonzero(hit)[0]
    order = pos[np.lexsort((pos, keys[pos]))]
    count = int(order.size)
    m = int(max_per_query)
    out_s = np.full(m, np.inf if metric == 0 else -np.inf, np.float32)
    out_i = np.full(m, PAD, np.uint64)
    out_r = np.zeros(m, np.int32)
    take = order[:m]
    out_s[:take.size] = sc[take]
    out_i[:take.size] = (ids[take] if ids is not None else take.astype(np.uint64) + np.uint64(index_base))
    out_r[:take.size] = raw[take]
    return count, out_s, out_i, out_r


def radius_for_count(all_scores, metric, want, dead=None):
    """A radius whose inclusive match set holds about `want` rows (0: none)."""
    s = all_scores.astype(np.float64)
    ok = ~np.isnan(s)
    if dead is not None:
        ok &= ~dead
    s = np.sort(s[ok])
    if metric != 0:
        s = s[::-1]
    if want <= 0 or s.size == 0:
        return float(-1.0) if metric == 0 else float(np.abs(s).max() * 2 + 1 if s.size else 1.0)
    return float(np.float32(s[min(want, s.size) - 1]))


def float_band(metric, all_scores, rows_f32, q_f32, radius):
    """Absolute tolerance of the match test at the bound (DESIGN.md §3's score tolerance at the radius, doubled)."""
    if metric == 0:
        t = TOL * max(abs(radius), 1e-30)
    elif metric == 2:
        t = TOL
    else:
        xn, qn = norms(rows_f32, q_f32)
        xfin = xn[np.isfinite(xn)]
        t = TOL * float((xfin.max() if xfin.size else 0.0) * qn)
    return 2 * t


def assert_float_radius(metric, count, got_s, got_i, all_scores, rows_f32, q_f32, radius, max_per_query, dead=None,
                        index_base=0):
    """Float spaces: clear matches returned, clear non-matches not, the count inside the tolerance band, scores within
    tolerance, best first, padding behind."""
    s = all_scores.astype(np.float64)
    live = ~np.isnan(s)
    if dead is not None:
        live &= ~dead
    sign = 1.0 if metric == 0 else -1.0
    d = sign * (s - radius)  # <= 0: inside
    band = float_band(metric, all_scores, rows_f32, q_f32, radius)
    must = np.nonzero(live & (d < -band))[0]
    may = np.nonzero(live & (d <= band))[0]
    assert must.size <= count <= may.size, f"count {count} outside [{must.size}, {may.size}]"
    n = min(count, max_per_query)
    assert (got_i[n:] == PAD).all(), "padding indices"
    assert (got_s[n:] == (np.inf if metric == 0 else -np.inf)).all(), "padding scores"
    li = (got_i[:n] - np.uint64(index_base)).astype(np.int64)
    assert len(set(li.tolist())) == n, "duplicate indices"
    assert set(li.tolist()) <= set(may.tolist()), "returned a row clearly outside the radius"
    if count <= max_per_query:
        assert set(must.tolist()) <= set(li.tolist()), "missed a row clearly inside the radius"
    ref = s[li]
    if metric == 0:
        tol = TOL * np.maximum(np.abs(ref), 1e-30)
    elif metric == 2:
        tol = np.full(n, TOL)
    else:
        xn, qn = norms(rows_f32, q_f32, li)
        tol = TOL * np.maximum(xn * qn, 1e-30)
    assert (np.abs(got_s[:n].astype(np.float64) - ref) <= tol).all(), "score outside the tolerance"
    assert (np.diff(sign * got_s[:n].astype(np.float64)) >= 0).all(), "not best first"
