"""MVF_DEBUG_POISON ("Poisoned allocations") without a GPU: how the switch is read, that no allocation of the
library can bypass it, and that the child-process runner of the GPU tests stops starting processes after a fault."""
import os
import re
import subprocess
import sys

import pytest

import _children

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metrovector_amd", "csrc")


def _poison_of_a_child(value):
    env = {k: v for k, v in os.environ.items() if k != "MVF_DEBUG_POISON"}
    if value is not None:
        env["MVF_DEBUG_POISON"] = value
    code = ("import sys; sys.modules.setdefault('torch', None); sys.path.insert(0, sys.argv[1]); "
            "from metrovector_amd import gpu; print(gpu.selftest_poison())")
    out = subprocess.run([sys.executable, "-c", code, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return int(out.stdout.split()[-1])


@pytest.mark.parametrize("value,want", [("165", 165), ("0", 0), ("255", 255), ("0xFF", 255), (None, -1), ("", -1), ("256", -1),
                                        ("-1", -1), ("poison", -1), ("12abc", -1)])
def test_the_switch_is_a_byte_or_nothing(value, want):
    assert _poison_of_a_child(value) == want


# Allocation calls that deliberately do not fill: none.  An entry is "file.hip:function" with the reason behind it.
EXEMPT = {
}

ALLOC = re.compile(r"\b(hipMalloc|hipMallocAsync|hipMallocFromPoolAsync|hipHostMalloc)\s*\(")
FILL = re.compile(r"\bpoison_fill(_host)?\s*\(")


def _functions(text):
    """(name, body) of every top-level or member function body: a `)` ... `{` at brace depth <= 2 opens one, its matching brace
    closes it (good enough for this code base: the check below fails loudly on an allocation it cannot place)."""
    out, stack = [], []
    for m in re.finditer(r"[{}]", text):
        if m.group() == "{":
            head = text[max(0, m.start() - 400):m.start()]
            sig = re.search(r"([A-Za-z_][A-Za-z_0-9:]*)\s*\([^;{}]*\)\s*(const\s*)?(->\s*[\w:]+\s*)?$", head)
            stack.append((m.start(), sig.group(1) if sig and sig.group(1) not in ("if", "for", "while", "switch") else None))
        elif stack:
            start, name = stack.pop()
            if name:
                out.append((name, start, m.end()))
    return out


def test_every_allocation_is_filled_under_the_switch():
    missing, sites = [], 0
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith((".hip", ".h", ".inc", ".cpp")):
            continue
        text = open(os.path.join(CSRC, fn)).read()
        text = re.sub(r"//[^\n]*", lambda m: " " * len(m.group()), text)  # comments may name the calls
        funcs = _functions(text)
        for m in ALLOC.finditer(text):
            sites += 1
            holders = [(e - s, name, s, e) for name, s, e in funcs if s < m.start() < e]
            assert holders, f"{fn}: {m.group(1)} at offset {m.start()} sits in no function this check can find"
            _, name, s, e = min(holders)  # the innermost function (a lambda's body counts as its own)
            if not FILL.search(text[s:e]) and f"{fn}:{name}" not in EXEMPT:
                missing.append(f"{fn}:{name} ({m.group(1)})")
    assert sites >= 15, "the allocation sites were not found at all"
    assert not missing, f"allocations that bypass MVF_DEBUG_POISON (fill them with poison_fill, or exempt them with a reason): {missing}"


def test_the_runner_stops_after_a_child_that_faults():
    """a host-only child that exits as a segmentation fault is reported: nothing runs on a GPU here"""
    r = _children.ChildRunner()
    assert r.run([sys.executable, "-c", "print('fine')"]).stdout.strip() == "fine"
    with pytest.raises(_children.ChildFault, match="139"):
        r.run([sys.executable, "-c", "import sys; sys.exit(139)"])
    started = r.started
    with pytest.raises(_children.ChildFault, match="not started"):
        r.run([sys.executable, "-c", "print('must not run')"])
    assert r.started == started and r.stopped


@pytest.mark.parametrize("code", ["import os, signal; os.kill(os.getpid(), signal.SIGKILL)",
                                  "print('hipErrorIllegalAddress: an illegal memory access was encountered')",
                                  "import time; time.sleep(30)"])
def test_what_counts_as_a_fault(code):
    r = _children.ChildRunner()
    with pytest.raises(_children.ChildFault):
        r.run([sys.executable, "-c", code], timeout=1)
    with pytest.raises(_children.ChildFault, match="not started"):
        r.run([sys.executable, "-c", "pass"])
