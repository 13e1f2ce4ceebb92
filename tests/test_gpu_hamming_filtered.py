"""-m gpu tests of the filtered Hamming search (include/mvf_gpu_hamming_filtered.h; DESIGN.md §3 "Filtered Hamming search", §5
"HG"): both routes, forced through MVF_FILTER_ROUTE, against the numpy reference over the admitted live rows (tests/_hamming.py),
byte for byte; ties; the twin handle whose tombstones are `deleted | ~allow`; the device call and the filter's refusals."""
import numpy as np
import pytest

from metrovector_amd import errors as E
from metrovector_amd import gpu as G

import _hamming as H

pytestmark = pytest.mark.gpu

MASK, LIST = 1, 2
N, BASE, NQ = 3001, 7, 130  # rows: no multiple of 16 or 256; 130 queries: two tiles of 128 / three of 64, the last ragged
SHAPES = [(1, 1), (17, 100), (130, 1024)]  # (nq, k)


def _force(monkeypatch, c, route):
    """MVF_FILTER_ROUTE is read into the handle's tuning; a filter takes it from the handle when it is created."""
    monkeypatch.setenv("MVF_FILTER_ROUTE", str(route))
    c.reload_tuning()


DEAD = np.random.default_rng(12).random(N) < 0.1
DEAD[[0, N - 1]] = False
ADMITTED = {"empty": 0, "last": 1, "15": 15, "255": 255, "257": 257, "1100": 1100, "2500": 2500}  # live rows a set admits


def _allow_sets():
    """the named number of LIVE rows each -- 255 and 257: the edge of an iteration of 256 list entries; 1100: two entries past a
    slice of 1024, rows 0 and N - 1 among them; 2500: two list slices -- and, but for the first two, every other deleted row"""
    rng = np.random.default_rng(11)
    live = np.nonzero(~DEAD)[0]
    out = {}
    for name, m in ADMITTED.items():
        at = [N - 1][:m] if m <= 1 else np.r_[0, N - 1, rng.choice(live[1:-1], m - 2, False)]
        out[name] = np.zeros(N, bool)
        out[name][np.asarray(at, np.int64)] = True
        if m > 1:
            out[name] |= DEAD & (np.arange(N) % 2 == 0)  # tombstones overlap the allow bits
    return out


ALLOW = _allow_sets()
IDS = np.random.default_rng(13).permutation(N).astype(np.uint64) * np.uint64(3) + np.uint64(10**12)


@pytest.mark.parametrize("route", [MASK, LIST])
@pytest.mark.parametrize("dim", [1, 16, 17, 64, 65, 256, 272, 512, 513])
def test_both_routes_against_the_reference(monkeypatch, dim, route):
    rng = np.random.default_rng(dim)
    x = rng.integers(0, 256, (N, dim), dtype=np.uint8)
    q = rng.integers(0, 256, (NQ, dim), dtype=np.uint8)
    q[::3] = x[(5 * np.arange(0, NQ, 3)) % N] ^ rng.integers(0, 2, (len(q[::3]), dim), dtype=np.uint8)  # near-copies of rows
    d = H.distances(q, x)
    with G.GpuCorpus.from_array(x, index_base=BASE) as c:
        c.set_tombstones(np.packbits(DEAD, bitorder="little"))
        _force(monkeypatch, c, route)
        for name, allow in ALLOW.items():
            admit = allow & ~DEAD
            with c.make_filter(allow) as f:
                assert f.admitted == int(admit.sum()) == ADMITTED[name]
                by_list = route == LIST and dim <= 512 and f.admitted > 0
                assert f.info().has_row_list == (1 if route == LIST and f.admitted else 0)  # no silent fall-back to the mask
                for nq, k in SHAPES:  # (k = 100 and 1024 exceed the smaller sets: padding)
                    form = G.hamming_filtered_form(dim, nq, k, N, f.admitted, bool(f.info().has_row_list), route)
                    assert form.route == (2 if by_list else 1)
                    assert not by_list or form.list_slices == (2 if name == "2500" else 1), (name, form)  # HG across a slice boundary
                    res = c.search_hamming_filtered(q[:nq], k, f)
                    assert H.same(res, H.select(d[:nq], k, ~admit, None, BASE)), (name, nq, k)
                if name == "1100":
                    c.set_vector_ids(IDS)
                    assert H.same(c.search_hamming_filtered(q[:17], 100, f), H.select(d[:17], 100, ~admit, IDS, BASE)), "vector ids"
                    c.set_vector_ids(None)


@pytest.mark.parametrize("dim", [16, 100])
def test_ties_go_by_position_on_both_routes(monkeypatch, dim):
    rng = np.random.default_rng(21)
    x = np.ascontiguousarray(np.tile(rng.integers(0, 256, (64, dim), dtype=np.uint8), (47, 1))[:N])  # 64 distinct rows repeated
    q = np.ascontiguousarray(np.concatenate([x[:3], rng.integers(0, 256, (14, dim), dtype=np.uint8)]))
    allow = rng.random(N) < 0.6
    want = H.select(H.distances(q, x), 100, ~(allow & ~DEAD), None, BASE)
    with G.GpuCorpus.from_array(x, index_base=BASE) as c:
        c.set_tombstones(np.packbits(DEAD, bitorder="little"))
        for route in (MASK, LIST):
            _force(monkeypatch, c, route)
            with c.make_filter(allow) as f:
                assert f.info().has_row_list == (route == LIST)
                assert H.same(c.search_hamming_filtered(q, 100, f), want), f"route {route}"


@pytest.mark.parametrize("route", [MASK, LIST])
def test_the_call_equals_the_hamming_search_of_a_twin_handle(monkeypatch, route):
    dim, k = 96, 50
    rng = np.random.default_rng(31)
    x = rng.integers(0, 256, (N, dim), dtype=np.uint8)
    q = rng.integers(0, 256, (NQ, dim), dtype=np.uint8)
    allow = ALLOW["1100"]
    with G.GpuCorpus.from_array(x, index_base=BASE) as twin:
        twin.set_tombstones(np.packbits(DEAD | ~allow, bitorder="little"))
        want = twin.search_hamming(q, k)
    with G.GpuCorpus.from_array(x, index_base=BASE) as c:
        c.set_tombstones(np.packbits(DEAD, bitorder="little"))
        _force(monkeypatch, c, route)
        plain = c.search_hamming(q, k)
        with c.make_filter(allow) as f:
            assert f.info().has_row_list == (route == LIST)
            assert H.same(c.search_hamming_filtered(q, k, f), (want.scores, want.indices, want.raw))
        assert H.same(c.search_hamming(q, k), (plain.scores, plain.indices, plain.raw)), "the handle's own search changed"


@pytest.mark.parametrize("route", [MASK, LIST])
def test_device_call_on_a_stream_and_the_filters_refusals(monkeypatch, route):
    import torch
    dim, nq, k = 48, 20, 100
    rng = np.random.default_rng(41)
    x = rng.integers(0, 256, (N, dim), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, dim), dtype=np.uint8)
    allow = ALLOW["2500"]
    with G.GpuCorpus.from_array(x, index_base=BASE) as c, G.GpuCorpus.from_array(x[:500]) as other:
        _force(monkeypatch, c, route)
        f = c.make_filter(allow)
        assert f.info().has_row_list == (route == LIST)
        host = c.search_hamming_filtered(q, k, f)
        assert H.same(host, H.reference(q, x, k, dead=~allow, index_base=BASE))
        dq = torch.from_numpy(q).cuda()
        ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        di = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        dr = torch.empty((nq, k), dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        c.search_hamming_filtered_device(f, dq.data_ptr(), G.UINT8, dim, nq, k, ds.data_ptr(), di.data_ptr(), dr.data_ptr(), st.cuda_stream)
        st.synchronize()
        assert di.cpu().numpy().view(np.uint64).tobytes() == host.indices.tobytes()
        assert ds.cpu().numpy().tobytes() == host.scores.tobytes() and dr.cpu().numpy().tobytes() == host.raw.tobytes()
        with pytest.raises(E.InvalidArgument, match="another corpus handle"):
            other.search_hamming_filtered(q, k, f)
        c.set_tombstones(np.packbits(DEAD, bitorder="little"))
        with pytest.raises(E.InvalidArgument, match="stale filter.*set_tombstones"):
            c.search_hamming_filtered(q, k, f)
        f.close()


def test_the_automatic_rule_on_the_device(monkeypatch):
    """MVF_FILTER_ROUTE unset.  10M rows of 64 bytes with a ten-thousandth admitted: the filter holds its list and the rule takes
    HG; the small corpus of the other tests stays on the mask route.  (The reference scores the admitted rows only.)"""
    monkeypatch.delenv("MVF_FILTER_ROUTE", raising=False)
    rng = np.random.default_rng(51)
    for n, dim, admitted, route in ((10_000_000, 64, 1000, LIST), (N, 64, 255, MASK)):
        x = rng.integers(0, 256, (n, dim), dtype=np.uint8)
        q = rng.integers(0, 256, (3, dim), dtype=np.uint8)
        allow = np.zeros(n, bool)
        allow[np.r_[0, n - 1, rng.choice(n - 2, admitted - 2, False) + 1]] = True
        with G.GpuCorpus.from_array(x, index_base=BASE) as c:
            c.reload_tuning()
            with c.make_filter(allow) as f:
                assert f.admitted == admitted
                assert G.hamming_filtered_form(dim, 3, 10, n, admitted, bool(f.info().has_row_list), 0).route == route
                assert H.same(c.search_hamming_filtered(q, 10, f), H.reference(q, x, 10, dead=~allow, index_base=BASE))
