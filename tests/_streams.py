"""Cross-stream ordering of one handle's calls (DESIGN.md §3 "Stream discipline", §8): a stall that keeps a torch stream busy,
the two controls that prove a missing dependency WOULD be seen, `run_pair`, and the class of every function the header declares.

No pytest in here; torch only for the stall and the device buffers (imported where it is used: the table below is read without it).
"""
import time

import numpy as np

STALL_MS = 100.0        # of a scenario: bounded, ends by itself
CONTROL_STALL_MS = 30.0  # of a control: the calls it has to outrun take well under a millisecond
TRIES = 8

# ---- the class of every extern "C" function of include/mvf_gpu.h ------------------------------------------------------------
NO_HANDLE = "takes no handle"
NO_DEVICE_WORK = "no device work"
DEVICE_CALL = "runs under corpus_device_call"
BLOCKS_DEVICE = "blocks the device"          # hipDeviceSynchronize under the handle's lock, then synchronous copies
HOST_WAIT = "waits for the handle's newest work on the host"  # hipEventSynchronize(ev_done) (or a blocking copy of rows that
#                                                               never change), then own-stream work it waits for itself

ENTRY_CLASS = {
    "mvfgpu_device_count": NO_HANDLE,
    "mvfgpu_strerror": NO_HANDLE,
    "mvfgpu_last_error_message": NO_HANDLE,
    "mvfgpu_merge_topk_host": NO_HANDLE,
    "mvfgpu_merge_topk_device": NO_HANDLE,
    "mvfgpu_merge_topk_packed_device": NO_HANDLE,
    "mvfgpu_synth_queries_device": NO_HANDLE,
    "mvfgpu_abi_version": NO_HANDLE,
    "mvfgpu_selftest_filter_route": NO_HANDLE,
    "mvfgpu_selftest_partition_plan": NO_HANDLE,
    "mvfgpu_selftest_group_plan": NO_HANDLE,
    "mvfgpu_selftest_maxsim_plan": NO_HANDLE,
    "mvfgpu_selftest_maxsim_form": NO_HANDLE,
    "mvfgpu_selftest_maxsim_candidates_plan": NO_HANDLE,
    "mvfgpu_selftest_predicate_range": NO_HANDLE,
    "mvfgpu_selftest_radius_bound": NO_HANDLE,
    "mvfgpu_selftest_radius_route": NO_HANDLE,
    "mvfgpu_selftest_feedback": NO_HANDLE,
    "mvfgpu_selftest_route": NO_HANDLE,
    "mvfgpu_selftest_stream_rows": NO_HANDLE,
    "mvfgpu_selftest_stream_bits": NO_HANDLE,
    "mvfgpu_selftest_shadow6_bytes": NO_HANDLE,
    "mvfgpu_selftest_shadow6_pack": NO_HANDLE,
    "mvfgpu_selftest_shadow6_unpack": NO_HANDLE,
    "mvfgpu_selftest_schedule": NO_HANDLE,
    "mvfgpu_selftest_poison": NO_HANDLE,
    # a handle is made: no other call can hold it yet
    "mvfgpu_corpus_create": BLOCKS_DEVICE,
    "mvfgpu_corpus_create_ex": BLOCKS_DEVICE,
    "mvfgpu_corpus_create_synthetic": BLOCKS_DEVICE,
    "mvfgpu_corpus_destroy": BLOCKS_DEVICE,
    "mvfgpu_corpus_set_tombstones": BLOCKS_DEVICE,
    "mvfgpu_corpus_set_vector_ids": BLOCKS_DEVICE,
    "mvfgpu_corpus_get_info": NO_DEVICE_WORK,
    "mvfgpu_filter_get_info": NO_DEVICE_WORK,
    "mvfgpu_column_get_info": NO_DEVICE_WORK,
    "mvfgpu_partition_get_info": NO_DEVICE_WORK,
    "mvfgpu_partition_lookup": NO_DEVICE_WORK,
    "mvfgpu_partition_keys": NO_DEVICE_WORK,
    "mvfgpu_set_profiling": NO_DEVICE_WORK,
    "mvfgpu_set_scan_path": NO_DEVICE_WORK,
    "mvfgpu_corpus_reload_tuning": NO_DEVICE_WORK,
    "mvfgpu_shardset_create": NO_DEVICE_WORK,   # streams, events and the communicator of the set: nothing of a shard's handle
    "mvfgpu_shardset_destroy": NO_DEVICE_WORK,  # (its searches have been waited for by the search call)
    "mvfgpu_shardset_get_info": NO_DEVICE_WORK,
    "mvfgpu_shardset_last_timing": NO_DEVICE_WORK,
    "mvfgpu_corpus_read_rows": HOST_WAIT,
    "mvfgpu_corpus_gather_rows": HOST_WAIT,
    "mvfgpu_last_timing": HOST_WAIT,
    "mvfgpu_filter_destroy": HOST_WAIT,
    "mvfgpu_column_destroy": HOST_WAIT,
    "mvfgpu_partition_destroy": HOST_WAIT,
    "mvfgpu_search": DEVICE_CALL,
    "mvfgpu_search_fetch": DEVICE_CALL,
    "mvfgpu_search_device": DEVICE_CALL,
    "mvfgpu_search_radius": DEVICE_CALL,
    "mvfgpu_search_candidates": DEVICE_CALL,
    "mvfgpu_search_candidates_device": DEVICE_CALL,
    "mvfgpu_filter_create": DEVICE_CALL,
    "mvfgpu_filter_create_device": DEVICE_CALL,
    "mvfgpu_filter_create_where": DEVICE_CALL,
    "mvfgpu_search_filtered": DEVICE_CALL,
    "mvfgpu_search_filtered_device": DEVICE_CALL,
    "mvfgpu_column_create": DEVICE_CALL,
    "mvfgpu_column_create_device": DEVICE_CALL,
    "mvfgpu_column_gather": DEVICE_CALL,
    "mvfgpu_partition_create": DEVICE_CALL,
    "mvfgpu_search_partitioned": DEVICE_CALL,
    "mvfgpu_search_partitioned_device": DEVICE_CALL,
    "mvfgpu_search_grouped": DEVICE_CALL,
    "mvfgpu_search_grouped_device": DEVICE_CALL,
    "mvfgpu_search_maxsim": DEVICE_CALL,
    "mvfgpu_search_maxsim_device": DEVICE_CALL,
    "mvfgpu_search_maxsim_candidates": DEVICE_CALL,
    "mvfgpu_search_maxsim_candidates_device": DEVICE_CALL,
    "mvfgpu_knn_join": DEVICE_CALL,
    "mvfgpu_knn_join_device": DEVICE_CALL,
    "mvfgpu_shardset_search": DEVICE_CALL,  # mvfgpu_search_device on every shard, on the set's streams
    "mvfgpu_selftest_grouped_stage_ms": DEVICE_CALL,
    "mvfgpu_selftest_maxsim_stage_ms": DEVICE_CALL,
    "mvfgpu_selftest_maxsim_candidates_stage_ms": DEVICE_CALL,
    "mvfgpu_selftest_where_kernel_ms": DEVICE_CALL,
}

# The measurement aids among the device-call routes: each runs the device form it times (named there) between events and waits
# for the stream -- the scenarios name the form, not the aid.
TIMED_FORM_OF = {
    "mvfgpu_selftest_grouped_stage_ms": "mvfgpu_search_grouped_device",
    "mvfgpu_selftest_maxsim_stage_ms": "mvfgpu_search_maxsim_device",
    "mvfgpu_selftest_maxsim_candidates_stage_ms": "mvfgpu_search_maxsim_candidates_device",
    "mvfgpu_selftest_where_kernel_ms": "mvfgpu_filter_create_where",
}


# ---- the scenarios of tests/test_gpu_stream_order.py: id -> the entries its calls are (producer, consumer, ...) ------------------
def _lazy(dtype, path, metric, consumers, extra=""):
    entry = {"dev": "mvfgpu_search_device", "host": "mvfgpu_search", "hostother": "mvfgpu_search", "batch5": "mvfgpu_search_device",
             "filtermask": "mvfgpu_search_filtered", "filterlist": "mvfgpu_search_filtered", "filterdev": "mvfgpu_search_filtered_device",
             "join": "mvfgpu_knn_join", "cand": "mvfgpu_search_candidates"}
    out = {}
    for cons in consumers:
        e = "mvfgpu_search_radius" if cons.startswith("radius") else "mvfgpu_search" if cons.startswith("p") else entry[cons]
        out[f"lazy:{dtype}:{path}:{metric}:{cons}{extra}"] = ("mvfgpu_search_device", e)
    return out


def _entries():
    forms = {"candidates": "mvfgpu_search_candidates", "filtered": "mvfgpu_search_filtered", "partitioned": "mvfgpu_search_partitioned",
             "grouped": "mvfgpu_search_grouped", "maxsim": "mvfgpu_search_maxsim", "maxsimcand": "mvfgpu_search_maxsim_candidates",
             "join": "mvfgpu_knn_join", "join2": "mvfgpu_knn_join"}
    out = {}
    for name, host in forms.items():
        out[f"entry:f32:{name}:host"] = (host + "_device", host)
        out[f"entry:f32:{name}:dev"] = ("mvfgpu_search_device", host + "_device")
    out["entry:f32:join2:search"] = ("mvfgpu_knn_join_device", "mvfgpu_search")
    return out


# lazy state built behind the stall: lazy:<stored type>:<producer's scan path>:<metric>:<consumer>
LAZY = {}
LAZY.update(_lazy("f32", 2, "cos", ["dev", "host", "radius16", "radius4", "filtermask", "filterlist", "join"]))
LAZY.update(_lazy("f32", 2, "l2", ["dev", "host", "radius16"]))
LAZY.update(_lazy("f32", 3, "cos", ["dev", "host", "p4x1"]))
LAZY.update(_lazy("f32", 5, "ip", ["dev", "host", "p6x1", "p6x4", "filterdev"]))
LAZY.update(_lazy("f16", 5, "l2", ["dev", "host"]))
LAZY.update(_lazy("f32", 6, "cos", ["dev", "host", "batch5"]))
LAZY.update(_lazy("f32", 7, "l2", ["host", "dev"]))
LAZY.update(_lazy("f32", 1, "l2", ["hostother", "dev"], ":passes"))
LAZY.update(_lazy("f32", 1, "l2", ["hostother"], ":sort"))
LAZY.update(_lazy("i8", 2, "l2", ["dev", "host", "radius5", "cand"]))
LAZY.update(_lazy("i8", 2, "ip", ["host", "radius5"]))
# two different batches under the handle's query matrix and candidate regions
SCRATCH = {f"scratch:f32:{path}": ("mvfgpu_search_device", "mvfgpu_search_device") for path in (2, 3, 5)}
# every other *_device entry on the stalled stream and its host form at once; and the reverse: a batched search that builds the
# norms on the stalled stream, the *_device entry on the other stream at once
ENTRIES = _entries()
SCENARIOS = {**LAZY, **SCRATCH, **ENTRIES}
# the tests of the GPU file that are no producer / consumer pair: name -> the entries they call around the stall
CUSTOM = {
    "test_three_device_searches_on_three_streams": ("mvfgpu_search_device",),
    "test_column_created_on_the_stalled_stream": ("mvfgpu_column_create_device", "mvfgpu_filter_create_where", "mvfgpu_partition_create",
                                                  "mvfgpu_column_gather"),
    "test_filter_created_on_the_stalled_stream": ("mvfgpu_filter_create_device", "mvfgpu_search_filtered"),
    "test_host_calls_behind_pending_device_work": ("mvfgpu_search_device", "mvfgpu_corpus_gather_rows", "mvfgpu_corpus_read_rows",
                                                   "mvfgpu_search_fetch", "mvfgpu_corpus_set_tombstones", "mvfgpu_corpus_set_vector_ids",
                                                   "mvfgpu_search", "mvfgpu_column_create", "mvfgpu_filter_create",
                                                   "mvfgpu_filter_create_where", "mvfgpu_search_filtered"),
    "test_last_timing_behind_a_stalled_k1_search": ("mvfgpu_search_device", "mvfgpu_last_timing"),
    "test_shardset_search_with_one_shard_pending": ("mvfgpu_search_device", "mvfgpu_shardset_search"),
    "test_destroy_behind_pending_work": ("mvfgpu_search_filtered_device", "mvfgpu_search_partitioned_device", "mvfgpu_column_create_device",
                                         "mvfgpu_filter_destroy", "mvfgpu_partition_destroy", "mvfgpu_column_destroy",
                                         "mvfgpu_corpus_destroy"),
}


def entries_named():
    """every entry some scenario or test of the GPU file names"""
    named = set()
    for entries in list(SCENARIOS.values()) + list(CUSTOM.values()):
        named.update(entries)
    return named


# ---- the stall ----------------------------------------------------------------------------------------------------------------
_UNITS_PER_MS = None  # _sleep cycles, or matmuls of the fallback chain, per millisecond: measured once per process
_CHAIN = None


def _sleep_units(units):
    import torch
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(units))
    else:
        global _CHAIN
        if _CHAIN is None:
            _CHAIN = torch.eye(1024, device="cuda")
        for _ in range(max(1, int(units))):
            torch.mm(_CHAIN, _CHAIN, out=_CHAIN)  # the identity squared: bounded, no overflow


def _calibrate():
    """units per millisecond, from ONE event-timed call on the current stream"""
    global _UNITS_PER_MS
    if _UNITS_PER_MS is None:
        import torch
        probe = 5_000_000 if hasattr(torch.cuda, "_sleep") else 200
        _sleep_units(probe // 100)  # the first launch pays for loading the kernel
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _sleep_units(probe)
        b.record()
        b.synchronize()
        _UNITS_PER_MS = probe / max(a.elapsed_time(b), 1e-3)
    return _UNITS_PER_MS


def stall(stream, ms=STALL_MS):
    """Keeps `stream` busy for about `ms` milliseconds; returns an event recorded behind the stall.  What a scenario asserts is
    not the time but that this event still reads query() == False where it matters (`pending`)."""
    import torch
    units = _calibrate() * ms
    with torch.cuda.stream(stream):
        _sleep_units(units)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def pending(ev):
    return not ev.query()


class NothingTested(AssertionError):
    """the stall had ended where the scenario needed it: the run says nothing about ordering"""


def require_pending(ev, where):
    if not pending(ev):
        raise NothingTested(f"the stall on the producer's stream had ended {where}: this run has tested nothing "
                            f"(a call waited on the host, or the stall is too short for this machine)")


# ---- the two controls ---------------------------------------------------------------------------------------------------------
def stream_control(s1, s2):
    """s1 does not wait for s2 by itself (one hardware queue under both, say): a fill behind the stall on s2 is NOT seen by a
    clone enqueued on s1 at once.  torch tensors only."""
    import torch
    buf = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ev = stall(s2, CONTROL_STALL_MS)
    with torch.cuda.stream(s2):
        buf.fill_(1)
    with torch.cuda.stream(s1):
        seen = buf.clone()
    still = pending(ev)
    torch.cuda.synchronize()
    return still and int(seen.max().item()) == 0 and int(buf.min().item()) == 1


def own_stream_control(corpus, query, s2):
    """A handle whose newest work ran on its own stream does not wait for s2 by itself: with a stall on s2 and no library call on
    it, a one-query K1 search returns while the stall is pending."""
    import torch
    corpus.set_scan_path(1)
    corpus.search(query, 1)  # the handle's newest work is on its own stream
    torch.cuda.synchronize()
    ev = stall(s2, CONTROL_STALL_MS)
    corpus.search(query, 1)
    still = pending(ev)
    corpus.set_scan_path(0)
    torch.cuda.synchronize()
    return still


class ControlFailed(Exception):
    pass


_STREAMS = None


def pick_streams(make_corpus, query):
    """(s1, s2): side streams for which both controls hold, chosen once per process among up to TRIES fresh pairs.  Raises
    ControlFailed naming the control that never held."""
    global _STREAMS
    if _STREAMS is None:
        import torch
        kept, failed = [], "stream control"
        for _ in range(TRIES):
            s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
            kept.append((s1, s2))  # a stream that failed stays alive: the next one is another
            if not stream_control(s1, s2):
                failed = "stream control"
                continue
            c = make_corpus()
            try:
                ok = own_stream_control(c, query, s2)
            finally:
                c.close()
            if ok:
                _STREAMS = (s1, s2)
                break
            failed = "own-stream control"
        else:
            raise ControlFailed(f"the {failed} held for none of {TRIES} pairs of side streams: a missing dependency could not be seen")
    return _STREAMS


def _one_more_stream():
    """(runtime, stream, buffer) of one more HIP stream that has run something, or None.  The runtime spreads a process' streams
    over its few hardware queues in turn; an attempt that makes a whole turn's worth of streams (two handles: four) would put
    its handle on the stalled stream's queue every time.  One stream more between attempts moves the turn on."""
    import ctypes as C
    import torch
    try:
        from _partitioned import _hip_runtime
        hip = _hip_runtime()
    except (SystemExit, OSError):
        return None
    st = C.c_void_p()
    if hip.hipStreamCreateWithFlags(C.byref(st), 1) != 0:  # hipStreamNonBlocking
        return None
    buf = torch.zeros(16, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    hip.hipMemsetAsync(C.c_void_p(buf.data_ptr()), 0, C.c_size_t(64), st)
    hip.hipStreamSynchronize(st)
    return hip, st, buf


def on_an_independent_handle(attempt, query, s2):
    """attempt() -> (result, handle, close) runs a stalled scenario with a host consumer on a FRESH handle.  Every handle has a
    stream of its own, which may share a hardware queue with s2 and then waits for it by itself: afterwards the own-stream control
    runs on that very handle, and where it does not hold the attempt has shown nothing and is made again on another handle (the
    failed ones stay open meanwhile: the next handle's stream is another).  Up to TRIES attempts."""
    import torch
    held, extra = [], []
    try:
        for _ in range(TRIES):
            result, handle, close = attempt()
            held.append(close)
            if own_stream_control(handle, query, s2):
                return result
            extra.append(_one_more_stream())
        raise NothingTested(f"the own-stream control held for none of {TRIES} fresh handles: their streams all wait for the "
                            f"stalled stream by themselves, a missing dependency could not be seen")
    finally:
        for close in held:
            close()
        torch.cuda.synchronize()
        for more in extra:
            if more is not None:
                more[0].hipStreamDestroy(more[1])


# ---- one producer and one consumer --------------------------------------------------------------------------------------------
def run_pair(make_ctx, producer, consumer, stalled, query=None):
    """Runs `producer`, then `consumer`, on a fresh context of `make_ctx` (closed again) and returns (what the producer wrote, what
    the consumer wrote), each a dict of arrays.

    A call has .entry, .is_async, .handle(ctx), .prepare(ctx) (device buffers), .force(ctx) (its scan path), .issue(ctx, stream)
    -> collect() and .after(ctx) (checks with the device idle behind it).
    stalled = None: producer, a full device synchronise, consumer, a synchronise -- the decoy and the reference.
    stalled = (s1, s2): the producer on s2 behind a stall with no host wait, the consumer on s1 (a host call: on its handle's own
    stream, which must pass the own-stream control afterwards), then a synchronise.  The stall must be pending when the consumer
    is issued and, for an asynchronous consumer, when it returns.  Two exceptions, each a host wait the library makes by design
    and each leaving the stall pending only when the call is ISSUED: a producer with .waits_for_its_stream (the first 6-bit
    search of a handle reads its shadow's bound maxima back: api.hip search_locked), and a consumer with .grows_scratch (a batch
    behind a one-query search: the handle's scratch grows, and the old buffer's hipFree waits for the device)."""
    import torch
    if stalled is None:
        ctx = make_ctx()
        try:
            producer.prepare(ctx)
            consumer.prepare(ctx)
            producer.force(ctx)
            torch.cuda.synchronize()
            got_p = producer.issue(ctx, None)
            torch.cuda.synchronize()
            producer.after(ctx)
            consumer.force(ctx)
            got_c = consumer.issue(ctx, None)
            torch.cuda.synchronize()
            consumer.after(ctx)
            return got_p(), got_c()
        finally:
            ctx.close()
    s1, s2 = stalled

    def attempt():
        ctx = make_ctx()
        try:
            producer.prepare(ctx)
            consumer.prepare(ctx)
            producer.force(ctx)
            torch.cuda.synchronize()
            ev = stall(s2)
            require_pending(ev, f"when the producer ({producer.entry}) was issued")
            t0 = time.perf_counter()
            got_p = producer.issue(ctx, s2)
            t1 = time.perf_counter()
            consumer.force(ctx)
            if not getattr(producer, "waits_for_its_stream", False):
                require_pending(ev, f"when the producer ({producer.entry}) had returned, {(t1 - t0) * 1e3:.1f} ms after it was issued, "
                                    f"and the consumer ({consumer.entry}) was issued")
            got_c = consumer.issue(ctx, s1)
            t2 = time.perf_counter()
            if consumer.is_async and not getattr(producer, "waits_for_its_stream", False) and not getattr(consumer, "grows_scratch", False):
                require_pending(ev, f"when the consumer ({consumer.entry}) returned, {(t2 - t1) * 1e3:.1f} ms after it was issued")
            torch.cuda.synchronize()
            consumer.after(ctx)
            return (got_p(), got_c()), consumer.handle(ctx), ctx.close
        except BaseException:
            ctx.close()
            raise

    if consumer.is_async:
        result, _, close = attempt()
        close()
        return result
    return on_an_independent_handle(attempt, query, s2)
