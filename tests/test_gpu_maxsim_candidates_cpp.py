"""include/mvf.hpp's GpuVectorSpace::rerank_top_k_documents beside find_top_k_documents, through examples/cpp/rerank_documents.cpp
(the mechanism of tests/test_cpp_mirror.py: the example is compiled with -Wall -Wextra -Werror against the built libraries and
run).  The example runs N_RUNS times, every run a fresh process, one at a time through tests/_children.py's runner: every run's
three lines must be the first run's bytes, the float64 contract of the documents scenario (tests/_fresh_process.py S17) and the
Python binding's score bits and keys for the same file."""
import os
import subprocess

import numpy as np
import pytest

import _fresh_process as F
import metrovector_amd as M
from _children import RUNNER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "examples", "cpp", "rerank_documents.cpp")
LIBDIR = os.path.join(ROOT, "metrovector_amd")

# Fresh runs of the example.  Before the scratch pool kept a block in use, 11 of 24 fresh runs printed wrong candidate sums
# (profiles/r20_fresh_index_routes.txt, section 2): with p = 11 / 24, N = ceil(ln 0.01 / ln(1 - p)) = 8 runs let that library
# pass by luck less than once in a hundred times.
N_RUNS = 8


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


def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


@pytest.mark.gpu
def test_the_cpp_helper_gives_the_python_bindings_bytes(tmp_path):
    from test_gpu_fresh_process import check_s17_answer, s17_reference
    inp = F.s17_inputs()
    rows, doc, T, k = inp["rows"], inp["doc"], F.S17_T, F.S17_K
    b = M.MvfBuilder()
    b.add_vector_space("s", F.S17_DIM, 0, 0, 0)
    b.add_vectors("s", rows)
    b.add_metadata_column("doc", 5, doc.astype("<u8").tobytes())
    path = str(tmp_path / "documents.mvf")
    b.build().save(path)
    cand = [int(c) for c in inp["cand"]]
    ref = s17_reference()
    exe = _compile(tmp_path)
    first = None
    for run in range(N_RUNS):
        out = RUNNER.run([exe, path, "s", "doc", str(T), str(k)] + [str(c) for c in cand])
        assert out.returncode == 0, f"run {run}: " + out.stdout + out.stderr
        lines = [l for l in out.stdout.splitlines() if l.split(":")[0] in ("documents", "reranked", "no candidates")]
        assert len(lines) == 3, f"run {run}: {out.stdout}"
        (dkeys, dbits), (rkeys, rbits) = _line(out.stdout, "documents"), _line(out.stdout, "reranked")
        check_s17_answer(_f32(dbits), np.array(dkeys, np.uint64), _f32(rbits), np.array(rkeys, np.uint64), ref)
        assert _line(out.stdout, "no candidates") == ([], []), f"run {run}"
        if first is None:
            first = lines
        assert lines == first, f"run {run} differs from the first run:\n{lines}\n{first}"
    with M.MvfReader.open(path) as r:
        space = r.vector_space("s")
        full = M.find_top_k_documents(space, rows[:T], k, column="doc")
        want = M.rerank_top_k_documents(space, rows[:T], np.array(cand, np.uint64), k, column="doc")
    assert want.counts[0] == 5, "4, 9, 0, 13, 21: the repeats, 77 and the pad are skipped"
    stdout = "\n".join(first)
    for name, res in (("documents", full), ("reranked", want)):
        keys, bits = _line(stdout, name)
        c = int(res.counts[0])
        assert keys == res.keys[0, :c].tolist() and bits == res.scores[0, :c].view(np.uint32).tolist(), name
