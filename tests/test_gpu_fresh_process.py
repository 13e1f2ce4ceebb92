"""Answers must not depend on what a process finds in memory the library allocated and has not written yet, nor on which
device call comes first in a process (tests/_fresh_process.py holds the scenarios; DESIGN.md §2, "Poisoned allocations").

Every scenario runs as a child process four times, one after the other: twice as it is, then with every allocation of the
library filled with 0x00 and with 0xFF before its first use (MVF_DEBUG_POISON).  Every run must match the CPU reference --
integer spaces bit for bit, float spaces by tests/_util.py's criterion with DESIGN.md §3's tolerance; the poisoned children
must report the byte they were given; where the two plain runs agree byte for byte, both poisoned runs must equal them byte
for byte; and on the routes whose bits DESIGN.md §3 defines the two plain runs must agree to begin with.

One child at a time, each under tests/_children.py's limit; after a child that faults no further process is started."""
import os
import sys

import numpy as np
import pytest

import _fresh_process as F
from _candidates import candidate_rows
from _children import RUNNER
from _filtered import assert_float_filtered, oracle_filtered
from _radius import assert_float_radius, oracle_radius
from _util import PAD
from metrovector_amd import gpu as G

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
INT = ("i8", "u8")


class Got:
    """the arrays one call left in a child's .npz"""

    def __init__(self, out, key):
        self.scores, self.indices, self.raw = out[key + ".scores"], out[key + ".indices"], out[key + ".raw"]
        self.counts = out.get(key + ".counts")
        self.vectors = out.get(key + ".vectors")


def _check_topk(oracle, rows, dt, metric, queries, k, admit, got, index_base=0, what=""):
    """`got` is the top-k of every query among rows[admit]: integer spaces bit for bit, float spaces within the tolerance"""
    code = F.DT[dt][1]
    assert got.scores.shape == got.indices.shape == got.raw.shape == (len(queries), k), what
    if dt in INT:
        sc, idx, raw = oracle_filtered(oracle, rows, code, metric, queries, k, admit, index_base=index_base)
        assert (got.indices == idx).all(), f"{what}: indices"
        assert (got.raw == raw).all(), f"{what}: raw"
        assert (got.scores.view(np.uint32) == sc.view(np.uint32)).all(), f"{what}: score bits"
        return
    assert (got.raw == 0).all(), f"{what}: raw of a float space"
    for j, q in enumerate(queries):
        assert_float_filtered(oracle, rows, code, metric, q, k, admit, got.scores[j], got.indices[j], index_base=index_base)


def _check_filter_info(info, n, admitted):
    assert info[1] == n and info[2] == admitted and info[0] in (0, 1) and info[3] >= ((n + 31) // 32 + 1) * 4


def expect_s1(oracle, name):
    inp = F.s1_inputs()

    def check(out):
        for k in F.S1_KS:
            got = Got(out, f"k{k}")
            _check_filter_info(out[f"k{k}.filter_info"], 60, 12)
            _check_topk(oracle, inp["rows"], "f32", F.L2, inp["query"], k, inp["allow"], got, what=f"k {k}")
            real = min(k, 12)
            assert (got.indices[0, :real] != PAD).all() and (got.indices[0, real:] == PAD).all(), f"k {k}: 12 rows are admitted"
            assert got.indices[0, :4].tolist() == [20, 25, 15, 30], f"k {k}"
            assert np.round(got.scores[0, :4].astype(np.float64), 1).tolist() == [1.0, 4.0, 6.0, 9.0], f"k {k}"
    return check


def expect_s2(oracle, name):
    route, shape = name.split("_")[1:]
    dt, dim = F.parse_shape(shape)
    inp = F.s2_inputs(dt, dim)
    adm = int(inp["admit"].sum())
    assert adm - 1 >= 1

    def check(out):
        _check_filter_info(out["filter.filter_info"], F.S2_ROWS, adm)
        if route == "r2":
            assert out["filter.filter_info"][0] == 1, "the forced list route builds the list"
        for key, metric, nq, k in F.s2_calls(inp):
            _check_topk(oracle, inp["rows"], dt, metric, inp["queries"][:nq], k, inp["admit"], Got(out, key), F.S2_BASE, key)
    return check


def expect_s3(oracle, name):
    dt, dim = F.parse_shape(name.split("_")[1])
    inp = F.s3_inputs(dt, dim)
    sels = [candidate_rows(inp["cand"][q], F.S2_ROWS, index_base=F.S2_BASE, dead=inp["dead"]) for q in range(F.S3_NQ)]
    assert all(1 <= s.size < F.S3_M for s in sels)

    def check(out):
        for metric in F.METRICS:
            got = Got(out, f"m{metric}")
            assert got.counts.tolist() == [s.size for s in sels], f"metric {metric}: counts"
            for q in range(F.S3_NQ):
                admit = np.zeros(F.S2_ROWS, bool)
                admit[sels[q]] = True
                one = Got({"x.scores": got.scores[q:q + 1], "x.indices": got.indices[q:q + 1], "x.raw": got.raw[q:q + 1]}, "x")
                _check_topk(oracle, inp["rows"], dt, metric, inp["queries"][q:q + 1], F.S3_K, admit, one, F.S2_BASE,
                            f"metric {metric} query {q}")
    return check


def expect_s4(oracle, name):
    dt, dim = F.parse_shape(name.split("_")[1])
    inp = F.s4_inputs(dt, dim)

    def check(out):
        for key, n, metric, nq, k in F.s4_calls():
            _check_topk(oracle, inp[n]["rows"], dt, metric, inp[n]["queries"][:nq], k, np.ones(n, bool), Got(out, key), what=key)
        for metric in F.METRICS:
            got = Got(out, f"fetch_m{metric}")
            _check_topk(oracle, inp[97]["rows"], dt, metric, inp[97]["queries"][:1], 10, np.ones(97, bool), got, what="fetch")
            assert (got.vectors[0] == inp[97]["rows"][got.indices[0].astype(np.int64)]).all(), "the fused payload rows"
    return check


def expect_s5(oracle, name):
    inp = F.s5_inputs(name.split("_")[1])

    def check(out):
        _check_topk(oracle, inp["rows"], inp["dt"], inp["metric"], inp["queries"], F.S5_K, np.ones(F.S5_ROWS, bool), Got(out, "batch"),
                    what=name)
    return check


def expect_s6(oracle, name):
    which = name.split("_")[1]
    inp = F.s6_inputs()
    nbytes = G.shadow6_bytes(F.S6_ROWS, F.S6_DIM) if which == "6b" else F.S6_ROWS * F.S6_DIM

    def check(out):
        for k in F.S6_KS:
            for metric in F.METRICS:
                key = f"m{metric}_k{k}"
                assert out[key + ".scan"].tolist()[:2] == [7, nbytes], f"{key}: the scan streamed the shadow"
                _check_topk(oracle, inp["rows"], "f32", metric, inp["queries"], k, np.ones(F.S6_ROWS, bool), Got(out, key), what=key)
    return check


def expect_s7(oracle, name):
    inp = F.s7_inputs()

    def check(out):
        for key, metric, nq, k in F.s7_calls():
            _check_topk(oracle, inp["rows"], "i8", metric, inp["queries"][:nq], k, np.ones(F.S7_ROWS, bool), Got(out, key), what=key)
    return check


def expect_s8(oracle, name):
    dt = name.split("_")[1]
    code = F.DT[dt][1]
    inp = F.s8_inputs(dt)
    rows, qs, radii = inp["rows"], inp["queries"], inp["radii"]
    want = [oracle_radius(oracle, rows, code, F.L2, qs[j], radii[j], F.S8_MAX) for j in range(3)]
    all_s = [oracle.scores(rows, code, F.L2, qs[j])[0] for j in range(3)]
    assert want[0][0] > G.RADIUS_LIST_CAP and 1 <= want[1][0] <= F.S8_MAX and want[2][0] == 0, [w[0] for w in want]

    def check(out):
        got = Got(out, "lists")
        only = out["counts_only.counts"]
        for j in range(3):
            if dt in INT:
                cnt, sc, idx, raw = want[j]
                assert got.counts[j] == cnt == only[j], f"query {j}: count"
                assert (got.indices[j] == idx).all() and (got.raw[j] == raw).all(), f"query {j}"
                assert (got.scores[j].view(np.uint32) == sc.view(np.uint32)).all(), f"query {j}: score bits"
            else:
                assert got.counts[j] == only[j], f"query {j}: the counts-only call"
                assert_float_radius(F.L2, int(got.counts[j]), got.scores[j], got.indices[j], all_s[j], rows.astype(np.float32),
                                    qs[j], float(radii[j]), F.S8_MAX)
    return check


def expect_s9(oracle, name):
    inp = F.s9_inputs()
    rows, dead = inp["rows"], inp["dead"]
    n, k = F.S9_ROWS, F.S9_K
    want = {}
    for metric in (F.L2, F.IP):
        S = np.full((n, k), np.inf if metric == F.L2 else -np.inf, np.float32)
        I = np.full((n, k), PAD, np.uint64)
        R = np.zeros((n, k), np.int32)
        for i in np.nonzero(~dead)[0]:  # a deleted query row is all padding
            sc, keys, raw = oracle.scores(rows, 2, metric, rows[i])
            comp = (keys.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
            comp[dead] = PAD
            comp[i] = PAD  # never its own neighbour, by position
            pos = (np.sort(np.partition(comp, k - 1)[:k]) & np.uint64(0xFFFFFFFF)).astype(np.int64)
            S[i], I[i], R[i] = sc[pos], pos.astype(np.uint64), raw[pos]
        want[metric] = (S, I, R)

    def check(out):
        for metric in (F.L2, F.IP):
            got = Got(out, f"m{metric}")
            S, I, R = want[metric]
            assert (got.indices == I).all() and (got.raw == R).all(), f"metric {metric}"
            assert (got.scores.view(np.uint32) == S.view(np.uint32)).all(), f"metric {metric}: score bits"
    return check


def expect_s10(oracle, name):
    dt = name.split("_")[1]
    inp = F.s10_inputs(dt)

    def check(out):
        for metric in F.METRICS:
            _check_topk(oracle, inp["rows"], dt, metric, inp["queries"], F.S10_K, np.ones(2 * F.S10_SHARD, bool),
                        Got(out, f"m{metric}"), what=f"metric {metric}")
    return check


EXPECT = dict(s1=expect_s1, s2=expect_s2, s3=expect_s3, s4=expect_s4, s5=expect_s5, s6=expect_s6, s7=expect_s7, s8=expect_s8,
              s9=expect_s9, s10=expect_s10)


def _child(name, tag, poison, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("MVF_DEBUG_POISON", "MVF_FILTER_ROUTE", "MVF_LARGE_K")}
    if poison is not None:
        env["MVF_DEBUG_POISON"] = str(poison)
    path = str(tmp_path / f"{tag}.npz")
    out = RUNNER.run([sys.executable, os.path.join(HERE, "_fresh_process.py"), name, path], env=env)
    assert out.returncode == 0, f"{name} ({tag}): exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}"
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files}
    assert arrays["poison"].tolist() == [-1 if poison is None else poison], f"{name} ({tag}): the child's poison byte"
    return arrays


def _differences(a, b):
    """the arrays of two runs that differ in shape, type or bytes (the poison byte itself aside)"""
    keys = sorted((set(a) | set(b)) - {"poison"})
    return [k for k in keys if k not in a or k not in b or a[k].dtype != b[k].dtype or a[k].shape != b[k].shape
            or a[k].tobytes() != b[k].tobytes()]


@pytest.mark.parametrize("name", list(F.scenarios()))
def test_fresh_process_answers_do_not_depend_on_stale_memory(oracle, tmp_path, name):
    bit_defined = F.scenarios()[name]
    check = EXPECT[name.split("_")[0]](oracle, name)
    first = _child(name, "plain1", None, tmp_path)
    second = _child(name, "plain2", None, tmp_path)
    check(first)
    plain_differ = _differences(first, second)
    if plain_differ:  # (a run that equals a checked one byte for byte has been checked)
        check(second)
    print(f"{name}: plain runs differ in {plain_differ or 'nothing'}")
    if bit_defined:
        assert not plain_differ, f"two plain runs of a bit-defined route differ in {plain_differ}"
    for tag, byte in (("poison00", 0x00), ("poisonFF", 0xFF)):  # 0x00 first: what it shows is diagnosed before 0xFF runs
        run = _child(name, tag, byte, tmp_path)
        diff = _differences(first, run)
        print(f"{name}: {tag} differs from the plain run in {diff or 'nothing'}")
        if not plain_differ:
            assert not diff, f"allocations filled with {byte:#04x} change {diff}"
        if diff:
            check(run)
