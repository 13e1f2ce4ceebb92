"""The stream discipline's bookkeeping (DESIGN.md §3 "Stream discipline"), without a GPU: every function the header declares
has a class in tests/_streams.py ENTRY_CLASS, and every device-call route is named by a scenario of
tests/test_gpu_stream_order.py.  Works from the header and the tables only."""
import os
import re

import _streams as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = {S.NO_HANDLE, S.NO_DEVICE_WORK, S.DEVICE_CALL, S.BLOCKS_DEVICE, S.HOST_WAIT}


def declared_functions():
    with open(os.path.join(ROOT, "include", "mvf_gpu.h")) as fh:
        text = fh.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#[^\n]*(\\\n[^\n]*)*", " ", text, flags=re.M)  # the preprocessor's lines
    return set(re.findall(r"\b(mvfgpu_\w+)\s*\(", text))


def test_the_parser_finds_the_header_s_functions():
    fns = declared_functions()
    assert len(fns) > 80
    assert {"mvfgpu_search_device", "mvfgpu_corpus_destroy", "mvfgpu_abi_version", "mvfgpu_selftest_shadow6_bytes",
            "mvfgpu_strerror", "mvfgpu_shardset_search"} <= fns
    assert "mvfgpu_corpus" not in fns and "mvfgpu_timing" not in fns  # types


def test_every_declared_function_has_a_class():
    fns = declared_functions()
    missing = sorted(fns - set(S.ENTRY_CLASS))
    assert not missing, f"include/mvf_gpu.h declares functions tests/_streams.py ENTRY_CLASS does not list: {missing}"
    gone = sorted(set(S.ENTRY_CLASS) - fns)
    assert not gone, f"ENTRY_CLASS lists functions the header no longer declares: {gone}"
    odd = {f: c for f, c in S.ENTRY_CLASS.items() if c not in CLASSES}
    assert not odd, f"unknown classes: {odd}"


def test_every_device_call_route_is_named_by_a_scenario():
    named = S.entries_named()
    unknown = sorted(named - set(S.ENTRY_CLASS))
    assert not unknown, f"scenarios name functions the header does not declare: {unknown}"
    for aid, form in S.TIMED_FORM_OF.items():
        assert S.ENTRY_CLASS[aid] == S.DEVICE_CALL and S.ENTRY_CLASS[form] == S.DEVICE_CALL
    routes = {f for f, c in S.ENTRY_CLASS.items() if c == S.DEVICE_CALL}
    uncovered = sorted(f for f in routes if f not in named and S.TIMED_FORM_OF.get(f) not in named)
    assert not uncovered, f"device-call routes no scenario of tests/test_gpu_stream_order.py names: {uncovered}"


def test_every_blocking_and_waiting_call_of_a_live_handle_is_named_too():
    """what a caller may run behind pending device work of a handle: the calls that wait by themselves"""
    named = S.entries_named()
    creates = {"mvfgpu_corpus_create", "mvfgpu_corpus_create_ex", "mvfgpu_corpus_create_synthetic"}  # no handle exists before them
    waits = {f for f, c in S.ENTRY_CLASS.items() if c in (S.BLOCKS_DEVICE, S.HOST_WAIT)} - creates
    assert not sorted(waits - named), sorted(waits - named)


def test_scenario_ids_are_well_formed():
    for sid, entries in S.SCENARIOS.items():
        assert sid.split(":")[0] in ("lazy", "scratch", "entry") and len(entries) == 2, sid
    assert len(S.LAZY) + len(S.SCRATCH) + len(S.ENTRIES) == len(S.SCENARIOS)
