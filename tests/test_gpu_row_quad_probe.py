"""GPU test of the two layers on top of the field core, on operands at the edges of their limb classes:

  * zkp_amd/csrc/rowfe.h (one limb per lane: the Horner tail of every Pippenger run, the inversion behind every block of batched encodings) is
    device-only code -- DPP row moves, v_permlane32_swap / v_permlane16_swap, __umul24 -- whose claim is "tools/model/rowfe_model.py is this
    file instruction for instruction".  tools/microbench/row_probe.hip runs every function of the header on full 64-lane register images and
    writes full images back; they must equal the model's, byte for byte, idle lanes included: the class maxima, single-limb maxima,
    non-canonical zeros and curve points of tests/row_quad_cases.py, the lane index through the moves between rows, row_invert, and whole
    Horner tails at the (windows, doublings) shapes of pip_run.  The -DZKP_AB_ROW_BPERMUTE build of the probe must write the same bytes.
  * zkp_amd/csrc/quad.h (a coordinate per lane of a quad): tools/microbench/quad_probe.hip against the host build of fe25519.h making
    quad.h's calls lane by lane (tests/host/fe_core_host_lib.cpp: t_quad_probe, bound-tracked).

tests/test_rowfe_model.py and tests/test_host_fe_core.py check the same expectations against Python integers without a GPU.  Each program
is compiled once and run once, as a child process with a time limit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import row_quad_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_probe(name, exe, *defines):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", *defines, os.path.join(ROOT, "tools", "microbench", name), "-o", exe])


def first_mismatches(got, want, names):
    """(record, operation, lane) of the first differing words of two [records][operations][lanes] arrays"""
    return [(int(r), names[o], int(l)) for r, o, l in zip(*np.nonzero(got != want))][:8]


@pytest.mark.gpu
def test_row_probe_matches_the_model(tmp_path):
    main, _, imgs, inv, inv_imgs, hor, hor_imgs = C.row_expected()
    assert len(main) >= 700 and len(inv) == 64 and len(hor) == 16
    fin = str(tmp_path / "row_operands.bin")
    C.row_input_words(main, inv, hor).tofile(fin)
    want = np.concatenate([imgs.ravel(), inv_imgs.ravel(), hor_imgs.ravel()])
    n_main = imgs.size
    outputs = {}
    for build, defines in (("default", ()), ("ZKP_AB_ROW_BPERMUTE", ("-DZKP_AB_ROW_BPERMUTE",))):
        exe, fout = str(tmp_path / ("row_probe_" + build)), str(tmp_path / ("row_results_%s.bin" % build))
        compile_probe("row_probe.hip", exe, *defines)
        subprocess.run([exe, fin, fout], check=True, timeout=120)
        got = np.fromfile(fout, np.uint32)
        assert got.shape == want.shape, build
        outputs[build] = got
        bad = first_mismatches(got[:n_main].reshape(imgs.shape), imgs, C.ROW_OPS)
        assert not bad, "%s build, main records %s: first mismatches (record, operation, lane) %s" % (build, [main[r]["kind"] for r, _, _ in bad], bad)
        bad = first_mismatches(got[n_main:n_main + inv_imgs.size].reshape(len(inv), 1, 64), inv_imgs.reshape(len(inv), 1, 64), ["row_invert"])
        assert not bad, "%s build: first mismatches (record, operation, lane) %s" % (build, bad)
        bad = first_mismatches(got[n_main + inv_imgs.size:].reshape(len(hor), 1, 64), hor_imgs.reshape(len(hor), 1, 64), ["horner tail"])
        assert not bad, "%s build, (W, C) %s: first mismatches (record, operation, lane) %s" % (build, [hor[r][:2] for r, _, _ in bad], bad)
        assert got.tobytes() == want.tobytes(), build
    assert outputs["default"].tobytes() == outputs["ZKP_AB_ROW_BPERMUTE"].tobytes()


@pytest.mark.gpu
def test_quad_probe_matches_the_host_path(tmp_path):
    recs = C.quad_records()
    assert len(recs) >= 160
    want = C.quad_expected("bound-tracked")
    exe, fin, fout = str(tmp_path / "quad_probe"), str(tmp_path / "quad_operands.bin"), str(tmp_path / "quad_results.bin")
    compile_probe("quad_probe.hip", exe)
    C.quad_input_words(recs).tofile(fin)
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    got = np.fromfile(fout, np.uint32)
    assert got.size == want.size
    got = got.reshape(want.shape)
    bad = [(int(r), C.QUAD_OPS[o], "lane %d limb %d" % (q, k)) for r, o, q, k in zip(*np.nonzero(got != want))][:8]
    assert not bad, "%s: first mismatches (record, operation, lane) %s" % ([recs[r][0] for r, _, _ in bad], bad)
    assert got.tobytes() == want.tobytes()
