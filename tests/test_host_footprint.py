"""Every *_batch call of include/zkp_toolbox.h on the host backend (ctx == NULL, 1 and 3 threads) writes its own output rows and nothing else, and
leaves its inputs alone: the catalogue and the check of tests/footprint_cases.py on numpy buffers.  And the catalogue is complete: every function
of the two headers that takes a non-const pointer has an entry or a reason in NOT_COVERED.  No GPU needed."""
import os
import re

import pytest

from tests import footprint_cases as F
from zkp_amd import cabi
from zkp_amd import toolbox as T

BATCH = F.cases("batch")


@pytest.mark.parametrize("case", BATCH, ids=[c.id for c in BATCH])
def test_batch_call_writes_its_rows_and_nothing_else(case):
    failures = F.run_case(case, T.lib(), None, device=False)
    assert not failures, "\n".join(failures)


def test_the_check_sees_a_stray_byte_and_a_missing_row():
    """the check itself: a `call` that writes one byte behind its output, three bytes behind it, one in front of it, one that skips the last row, one
    that damages an input"""
    import ctypes

    import numpy as np
    rows = np.arange(3 * 32, dtype=np.uint8).reshape(3, 32)

    class Lib:
        def __init__(self, at, value):
            self.at, self.value = at, value

        def call(self, src, dst):
            ctypes.memmove(dst.value, src.value, 64 if self.at[0] == "skip" else 96)
            if self.at[0] == "skip":
                return 0
            target = (dst if self.at[0] == "out" else src).value + self.at[1]
            ctypes.memmove(target, bytes([self.value]), 1)
            return 0

    def run(at, value):
        case = F.Case("call", "batch", 3, "", lambda: [F.IN("in", rows), F.OUT("out", rows)])
        return F.run_case(case, Lib(at, value), None, device=False)

    assert run(("out", 0), 0) == []
    assert "out: first differing byte at (row 3, byte 0)" in run(("out", 96), 0)[0]
    assert "out: first differing byte at (row 3, byte 3)" in run(("out", 99), 1)[0]
    assert "out: first differing byte at (row -1, byte 31)" in run(("out", -1), 0)[0]
    assert "in: first differing byte at (row 1, byte 0)" in run(("in", 32), 0xff)[0]
    skipped = run(("skip", 0), 0)[0]
    assert "out: first differing byte at (row 2, byte 0)" in skipped and "32 bytes differ" in skipped and "(prefill)" not in skipped


# ---- completeness ---------------------------------------------------------------------------------------------------------------------------------
def writers(header):
    """the functions of include/<header>, test-hook section included, with at least one non-const pointer (or array) parameter"""
    with open(os.path.join(cabi.INCLUDE, header)) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", src, flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    out = []
    for m in cabi._PROTO.finditer(src):
        _, name, params = m.groups()
        for p in params.split(","):
            if ("*" in p or "[" in p) and not p.strip().startswith("const"):
                out.append(name)
                break
    return out


_MANAGEMENT = "context, graph, job, pipe or statement management: takes a handle, writes no caller buffer"
_GETTER = "getter: returns one scalar, or writes one small record (a few words, a string) that its own tests read back"
_DEBUG = "zkp_debug_* hook of the test-hook build: not part of the shipped library"
_PIPE = "zkp_pipe_* / pipe job: scatters through strides of the caller's and needs a catalogue of its own; out of scope here"
_HOST_ONLY = ("zkp_toolbox.h is catalogued through its batch calls: this one handles a single item (one transcript, one scalar, one block, one proof's "
              "wire bytes) or is a host-only half of a batch call that has its own entry")

NOT_COVERED = {}
NOT_COVERED.update({n: _MANAGEMENT for n in (
    "zkp_ctx_create", "zkp_ctx_destroy", "zkp_ctx_set_stream", "zkp_ctx_synchronize", "zkp_ctx_set_option", "zkp_ctx_capture_begin",
    "zkp_ctx_capture_end", "zkp_ctx_capture_abort", "zkp_graph_launch", "zkp_graph_destroy", "zkp_ctx_prepare_fixed_points", "zkp_ctx_job_wait",
    "zkp_ctx_job_poll", "zkp_ctx_job_pending", "zkp_ctx_job_discard", "zkp_host_alloc", "zkp_host_alloc_on", "zkp_host_free", "zkp_host_register",
    "zkp_host_unregister", "zkp_ctx_prepare_dlog", "zkp_ctx_prepare_dlog_point", "zkp_ctx_release_dlog_point", "zkp_ctx_set_profiling",
    "zkp_statement_free", "zkp_statement_add_secret", "zkp_statement_add_point", "zkp_statement_constrain", "zkp_job_wait")})
NOT_COVERED.update({n: _GETTER for n in (
    "zkp_ctx_job_timing", "zkp_dlog_baby_bits", "zkp_dlog_point_baby_bits", "zkp_dlog_point_base", "zkp_dlog_point_find", "zkp_dlog_point_last_use",
    "zkp_ctx_last_timing", "zkp_ctx_last_kernels")})
NOT_COVERED.update({n: _DEBUG for n in (
    "zkp_debug_quad_selftest", "zkp_debug_row_selftest", "zkp_debug_wave_cycles", "zkp_debug_sha512", "zkp_debug_last_schedule",
    "zkp_debug_ragged_blocks", "zkp_debug_fill_workspace", "zkp_debug_ws_bytes", "zkp_debug_ws_count")})
NOT_COVERED.update({n: _PIPE for n in (
    "zkp_pipe_create", "zkp_pipe_destroy", "zkp_pipe_context", "zkp_pipe_shard_plan",
    "zkp_pipe_set_submit_threads", "zkp_prove_batch_submit", "zkp_verify_compact_batch_submit",
    "zkp_verify_batchable_each_submit", "zkp_batch_verify_many_submit", "zkp_pipe_prove_batch", "zkp_pipe_verify_compact_batch",
    "zkp_pipe_verify_batchable_each", "zkp_pipe_batch_verify", "zkp_pipe_batch_verify_many", "zkp_pipe_batch_verify_locate")})
NOT_COVERED.update({n: _HOST_ONLY for n in (
    "zkp_transcript_init", "zkp_transcript_append_message", "zkp_transcript_challenge_bytes", "zkp_scalar_from_wide", "zkp_scalar_muladd",
    "zkp_scalar_neg", "zkp_chacha20_block", "zkp_proof_compact_encode", "zkp_proof_compact_decode", "zkp_proof_batchable_encode",
    "zkp_proof_batchable_decode", "zkp_batch_verify_build", "zkp_prove_phase_a", "zkp_prove_phase_b")})


def test_every_function_that_writes_through_a_pointer_is_catalogued_or_listed_with_a_reason():
    have = F.catalogued()
    names = writers("zkp_mi355x.h") + writers("zkp_toolbox.h")
    missing = [n for n in names if n not in have and n not in NOT_COVERED]
    assert not missing, "neither in tests/footprint_cases.py nor in NOT_COVERED: %s" % missing
    assert all(isinstance(r, str) and r.strip() for r in NOT_COVERED.values())
    both = sorted(set(NOT_COVERED) & have)
    assert not both, "catalogued and listed as not covered: %s" % both
    stale = sorted(set(NOT_COVERED) - set(names))
    assert not stale, "listed as not covered, but no such function takes a non-const pointer: %s" % stale
    declared = set(cabi.signatures("zkp_mi355x.h")) | set(cabi.signatures("zkp_mi355x.h", test_hooks=True)) | set(cabi.signatures("zkp_toolbox.h"))
    unknown = sorted(have - declared)
    assert not unknown, "catalogued, but declared in no header: %s" % unknown
