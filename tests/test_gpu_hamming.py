"""Hamming search on the GPU (include/mvf_gpu_hamming.h; DESIGN.md §3 "Hamming search", §5 "H0 / H1"): every answer against
the numpy reference of tests/_hamming.py, byte for byte -- indices, raw distances and score bits, no query left out."""
import os
import subprocess

import numpy as np
import pytest

from _children import RUNNER
from metrovector_amd import errors as E
from metrovector_amd import gpu as G

import _hamming as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

POOL = np.random.default_rng(0x48414D).integers(0, 256, (20000, 1000), dtype=np.uint8)
QPOOL = np.random.default_rng(0x48414E).integers(0, 256, (70, 1000), dtype=np.uint8)
QPOOL[::3] = POOL[7:7 + 24 * 5:5] ^ np.random.default_rng(3).integers(0, 2, (24, 1000), dtype=np.uint8)  # near-copies of rows

QT = G.hamming_form(128, 1024, 10, 3001).query_tile
EDGE = max(d for d in range(1, 2049) if G.hamming_form(d, 1, 1, 1).form == 0)  # the last dimension of the register form
R3 = next(r for r in range(3002, 20001) if G.hamming_form(48, 2, 100, r).row_slices >= 3)

CASES = ([(d, 3001, QT + 1, 10) for d in (1, 15, 16, 17, 48, 128, EDGE, EDGE + 1, 1000)]
         + [(48, r, 2, 100) for r in (1, 63, 65, 3001, R3)]
         + [(128, 3001, nq, 10) for nq in (1, 2, QT - 1, QT, QT + 1, 70)]
         + [(d, 3001, 3, k) for d in (17, EDGE + 16) for k in (1, 10, 100, 1024)]
         + [(48, 63, 5, 1024), (1000, 65, 9, 1024), (16, 20000, 1, 1024), (100, R3, 70, 1024)]
         + [(16, 140000, 2, 100), (20, 600000, 1, 100)])  # more list entries than H1 sorts in one round: its bound, its rounds


def _data(dim, rows, nq):
    x = POOL[:rows, :dim] if rows <= len(POOL) else POOL[np.arange(rows) % len(POOL), :dim]  # beyond the pool: copies, so ties
    return np.ascontiguousarray(x), np.ascontiguousarray(QPOOL[:nq, :dim])


@pytest.mark.parametrize("dim,rows,nq,k", sorted(set(CASES)))
def test_against_numpy(dim, rows, nq, k):
    x, q = _data(dim, rows, nq)
    with G.GpuCorpus.from_array(x, device=0, index_base=1000) as c:
        res = c.search_hamming(q, k)
    assert H.same(res, H.reference(q, x, k, index_base=1000))


def test_rows_put_there_by_write_rows():
    """searches see written rows: a corpus created as all ones and overwritten row by row answers as the written rows do
    (the write, like the upload, leaves zeros in the pitch padding behind `dimension`: DESIGN.md §5 "W0")"""
    x, q = _data(17, 3001, 5)
    with G.GpuCorpus.from_array(np.full_like(x, 0xFF), device=0) as c:
        c.write_rows(np.arange(3001, dtype=np.uint64), x)
        res = c.search_hamming(q, 100)
    assert H.same(res, H.reference(q, x, 100))


@pytest.mark.parametrize("dim,distinct", [(16, 8), (48, 8), (300, 8), (48, 1)])
def test_ties_and_deletions(dim, distinct):
    """rows drawn from a few vectors: hundreds of ties at the k-th rank, a fifth of the rows deleted, ids permuted"""
    rng = np.random.default_rng(dim + distinct)
    n = 4000
    x = np.ascontiguousarray(POOL[:distinct, :dim][rng.integers(0, distinct, n)])
    q = np.ascontiguousarray(np.concatenate([POOL[:distinct, :dim][:2], QPOOL[:3, :dim]]))
    dead = rng.random(n) < 0.2
    ids = rng.permutation(n).astype(np.uint64) + np.uint64(10**12)
    with G.GpuCorpus.from_array(x, device=0) as c:
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        c.set_vector_ids(ids)
        for k in (1, 100, 1024):
            assert H.same(c.search_hamming(q, k), H.reference(q, x, k, dead=dead, ids=ids)), k


def test_accumulator_width():
    """33025 bytes of ones against zeros: 264 200 differing bits, beyond any 16-bit sum"""
    rng = np.random.default_rng(11)
    x = np.full((300, 33025), 0xFF, np.uint8)
    x[::7] = rng.integers(0, 256, (43, 33025), dtype=np.uint8)
    q = np.zeros((2, 33025), np.uint8)
    q[1] = rng.integers(0, 256, 33025, dtype=np.uint8)
    with G.GpuCorpus.from_array(x, device=0) as c:
        res = c.search_hamming(q, 300)
    assert int(res.raw[0].max()) == 264200 and res.scores[0].max() == np.float32(264200)
    assert H.same(res, H.reference(q, x, 300))


@pytest.mark.parametrize("dim", [17, 128])
def test_the_unpacked_l2_recipe_gives_the_same_answer(dim):
    x, q = _data(dim, 500, 6)
    with G.GpuCorpus.from_array(x, device=0) as c, G.GpuCorpus.from_array(np.unpackbits(x, axis=1), device=0) as c8:
        for k in (10, 505):
            res, l2 = c.search_hamming(q, k), c8.search(np.unpackbits(q, axis=1), k, G.L2)
            assert res.indices.tobytes() == l2.indices.tobytes() and res.raw.tobytes() == l2.raw.tobytes()
            assert res.scores.tobytes() == np.where(res.indices == H.PAD, np.float32(np.inf), res.raw.astype(np.float32)).tobytes()


def test_device_call_on_a_stream_and_the_handle_afterwards():
    import torch
    x, q = _data(48, 3001, 20)
    k = 100
    with G.GpuCorpus.from_array(x, device=0) as c:
        before = c.search(q, k, G.L2)
        host = c.search_hamming(q, k)
        dq = torch.from_numpy(q).cuda()
        ds = torch.empty((20, k), dtype=torch.float32, device="cuda")
        di = torch.empty((20, k), dtype=torch.int64, device="cuda")
        dr = torch.empty((20, k), dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        c.search_hamming_device(dq.data_ptr(), G.UINT8, 48, 20, k, ds.data_ptr(), di.data_ptr(), dr.data_ptr(), st.cuda_stream)
        st.synchronize()
        assert di.cpu().numpy().view(np.uint64).tobytes() == host.indices.tobytes()
        assert ds.cpu().numpy().tobytes() == host.scores.tobytes() and dr.cpu().numpy().tobytes() == host.raw.tobytes()
        after = c.search(q, k, G.L2)
        assert after.indices.tobytes() == before.indices.tobytes() and after.raw.tobytes() == before.raw.tobytes()
        assert after.scores.tobytes() == before.scores.tobytes()
    assert H.same(host, H.reference(q, x, k))


def test_two_stages_from_a_file_and_the_cpp_example(tmp_path):
    """find_top_k_hamming on a file's UInt8 space, with and without payloads, and examples/cpp/hamming_then_rerank.cpp (compiled
    with -Wall -Wextra -Werror against the built libraries): both printed lines hold the bytes of search_hamming and of
    search_candidates on the Float32 space of the same file"""
    import metrovector_amd as M
    x = np.random.default_rng(24).standard_normal((600, 100)).astype(np.float32)
    bits = G.pack_sign_bits(x)
    b = M.MvfBuilder()
    b.add_vector_space("bits", bits.shape[1], 0, 0, G.UINT8)
    b.add_vectors_raw("bits", bits)
    b.add_vector_space("floats", 100, 0, G.L2, G.FLOAT32)
    b.add_vectors("floats", x)
    path = str(tmp_path / "two_spaces.mvf")
    b.build().save(path)
    row, fetch_k, k = 17, 50, 5
    with G.GpuCorpus.from_array(bits) as c, G.GpuCorpus.from_array(x) as cf:
        coarse = c.search_hamming(bits[row], fetch_k)
        fine = cf.search_candidates(x[row:row + 1], coarse.indices, k, G.L2)
    assert H.same(coarse, H.reference(bits[row:row + 1], bits, fetch_k)) and coarse.indices[0, 0] == row
    with M.MvfReader.open(path) as r:
        hits = M.find_top_k_hamming(r.vector_space("bits"), bits[row], fetch_k)
        assert [h.index for h in hits] == coarse.indices[0].tolist() and [h.score for h in hits] == coarse.scores[0].tolist()
        assert all(h.vector is None for h in hits)
        every = M.find_top_k_hamming(r.vector_space("bits"), bits[row], 700, with_vectors=True)  # k beyond the rows: fewer items
        assert [h.index for h in every] == H.reference(bits[row:row + 1], bits, 600)[1][0].tolist()
        assert all(h.vector.dtype == np.uint8 and (h.vector == bits[h.index]).all() for h in every)
        with pytest.raises(E.BuildError):
            M.find_top_k_hamming(r.vector_space("floats"), bits[row], 3)
    exe = str(tmp_path / "hamming_then_rerank_cpp")
    libdir = os.path.join(ROOT, "metrovector_amd")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "cpp", "hamming_then_rerank.cpp"), "-L", libdir, "-lmvf_gpu", "-lmvf_host", f"-Wl,-rpath,{libdir}", "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    out = RUNNER.run([exe, path, "bits", "floats", str(row), str(fetch_k), str(k)])
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert [ln.split(":", 1)[0] for ln in lines] == ["hamming", "reranked"], out.stdout
    for line, want in zip(lines, (coarse, fine)):
        pairs = [p.split(":") for p in line.split(":", 1)[1].split()]
        assert [int(p[0]) for p in pairs] == want.indices[0].tolist(), line
        assert [int(p[1], 16) for p in pairs] == want.scores[0].view(np.uint32).tolist(), line
