"""GPU test of the scalar layer's DEVICE path.  zkp_amd/csrc/sc25519.h was tested with g++ only (tests/test_host_field.py), yet on the device
it reduces every hash output, builds every response and every batch-verification coefficient and feeds every recoder -- on operands no
flow can steer to the values where Montgomery code breaks.  The probe program (tools/microbench/sc_probe.hip) pushes an operand file
through one kernel per function: the catalogue of tests/scalar_edge_cases.py crossed with itself, an all-ones first operand against l - 1,
single all-ones words, multiples of 2^32 (m = 0), products that end in [l, 2l) and below l before the last subtraction, wide values at l,
2^256, 2^512 - 1 and the largest multiple of l, random records.  Its output must equal, byte for byte, what Python integers give
(scalar_edge_cases.probe_expected); tests/test_host_scalar_edges.py proves the same expectations for the host build of the header."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import scalar_edge_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = ["sc_reduce", "sc_to_mont", "sc_mont", "sc_mul", "sc_add", "sc_neg", "sc_from_wide", "sc_halve", "sc_halve_canonical", "sc_fold_sign", "flags",
          "sc_add_pattern 0x88888888", "sc_add_pattern 0xAAAAAAAA", "sc_add_pattern 0x80808080", "tops", "response"]


@pytest.mark.gpu
def test_probe_kernels_match_python_integers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "sc_probe")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", os.path.join(ROOT, "tools", "microbench", "sc_probe.hip"), "-o", exe])
    recs = S.probe_records()
    assert len(recs) >= 4000
    operands = np.array([S.words(a) + S.words(b) + S.words(c) for a, b, c in recs], np.uint32)
    fin, fout = str(tmp_path / "operands.bin"), str(tmp_path / "results.bin")
    operands.tofile(fin)
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    got = np.fromfile(fout, np.uint32)
    want = np.array([S.probe_expected(a, b, c) for a, b, c in recs], np.uint32)
    assert got.shape == (want.size,)
    bad = np.nonzero((got.reshape(len(recs), 16, 8) != want.reshape(len(recs), 16, 8)).any(axis=2))
    assert got.tobytes() == want.tobytes(), "first mismatches (record, function): %s" % [(int(r), BLOCKS[f]) for r, f in zip(*bad)][:8]
