"""include/mvf.hpp's GpuVectorSpace::rerank_top_k_documents beside find_top_k_documents, through examples/cpp/rerank_documents.cpp
(the mechanism of tests/test_cpp_mirror.py: the example is compiled with -Wall -Wextra -Werror against the built libraries and
run): its lines must be the Python binding's score bits and keys for the same file."""
import os
import subprocess

import numpy as np
import pytest

import metrovector_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "examples", "cpp", "rerank_documents.cpp")
LIBDIR = os.path.join(ROOT, "metrovector_amd")


def _compile(tmp_path):
    exe = str(tmp_path / "rerank_documents_cpp")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), SRC,
           "-L", LIBDIR, "-lmvf_gpu", "-lmvf_host", f"-Wl,-rpath,{LIBDIR}", "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def test_the_example_compiles_without_warnings(tmp_path):
    _compile(tmp_path)


def _line(stdout, name):
    hits = [l for l in stdout.splitlines() if l.startswith(name + ":")]
    assert len(hits) == 1, stdout
    pairs = [t.split(":") for t in hits[0].split(":", 1)[1].split()]
    return [int(p[0]) for p in pairs], [int(p[1], 16) for p in pairs]


@pytest.mark.gpu
def test_the_cpp_helper_gives_the_python_bindings_bytes(tmp_path):
    n, dim, T, k = 600, 8, 3, 6
    rng = np.random.default_rng(21)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    doc = rng.integers(0, 30, n).astype(np.uint64) * np.uint64(1000003)
    b = M.MvfBuilder()
    b.add_vector_space("s", dim, 0, 0, 0)
    b.add_vectors("s", rows)
    b.add_metadata_column("doc", 5, doc.astype("<u8").tobytes())
    path = str(tmp_path / "documents.mvf")
    b.build().save(path)
    cand = [int(v) for v in (np.array([4, 9, 9, 77, 0, 13, 4, 21], np.uint64) * np.uint64(1000003))] + [(1 << 64) - 1]
    exe = _compile(tmp_path)
    out = subprocess.run([exe, path, "s", "doc", str(T), str(k)] + [str(c) for c in cand], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    with M.MvfReader.open(path) as r:
        space = r.vector_space("s")
        full = M.find_top_k_documents(space, rows[:T], k, column="doc")
        want = M.rerank_top_k_documents(space, rows[:T], np.array(cand, np.uint64), k, column="doc")
    assert want.counts[0] == 5, "4, 9, 0, 13, 21: the repeats, 77 and the pad are skipped"
    for name, res in (("documents", full), ("reranked", want)):
        keys, bits = _line(out.stdout, name)
        c = int(res.counts[0])
        assert keys == res.keys[0, :c].tolist() and bits == res.scores[0, :c].view(np.uint32).tolist(), name
    assert _line(out.stdout, "no candidates") == ([], [])
