"""GPU test of the field core's DEVICE path: on gfx950 fe_mul / fe_sq pin the v_mad_u64_u32 of the low columns with inline assembly (the
host path of the same header is plain C++), so the host tests do not cover it.  The probe program (tools/microbench/fe_probe.hip) pushes
an operand file of every admissible class pair through one kernel per function; its output must equal, byte for byte, what the host
build of the header computes for the same file (tests/host/fe_core_host_lib.cpp, bound-tracked).  The first operand of a record is squared
as well, so it is tight or sum; the pairs diff x sum, diff x tight and extreme x tight reach fe_mul through the swapped kernel
(k_probe<7>: b * a).  k_probe<8> multiplies by the curve constant d: a constant operand takes the compiler's path on the device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import fe_core_cases as K

D = 37095705934669439343138083508754565189542113879843219016388785533085940283555      # the curve constant d (fe_constants.h: FE_D)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_probe_kernels_match_the_host_path(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "fe_probe")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", os.path.join(ROOT, "tools", "microbench", "fe_probe.hip"), "-o", exe])
    recs = K.probe_records()
    assert len(recs) >= 500
    limbs = np.array([a + b for a, b, _, _ in recs], np.uint32)
    bounds = np.array([ua + ub for _, _, ua, ub in recs], np.uint32)
    fin, fout = str(tmp_path / "operands.bin"), str(tmp_path / "results.bin")
    limbs.tofile(fin)
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    got = np.fromfile(fout, np.uint32)
    want = np.zeros(len(recs) * 54, np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    K.build("bound-tracked").t_core_probe(ctypes.c_uint32(len(recs)), limbs.ctypes.data_as(u32p), bounds.ctypes.data_as(u32p), want.ctypes.data_as(u32p))
    assert got.shape == want.shape
    bad = np.nonzero((got != want).reshape(len(recs), 6, 9).any(axis=2))
    assert got.tobytes() == want.tobytes(), "first mismatches (record, function): %s" % list(zip(*bad))[:8]
    # ... and the host result itself is right: a*b and a^(2^10) of every record against Python integers
    res = want.reshape(len(recs), 6, 9)
    for (a, b, _, _), r in zip(recs, res):
        assert K.value([int(x) for x in r[0]]) == K.value([int(x) for x in r[1]]) == K.value(a) * K.value(b) % K.P
        assert K.value([int(x) for x in r[4]]) == pow(K.value(a), 2 ** 10, K.P)
        assert K.value([int(x) for x in r[5]]) == K.value(a) * D % K.P
