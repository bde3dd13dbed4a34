"""The batchable 1-of-k OR-proofs without a GPU: the toolbox's host route (ctx == NULL: the items of zkp_amd/csrc/or_batch_lane.h on host
threads) against the model of tests/or_batch_model.py over oracle.model -- commitments, transcripts, verdicts and the batch verifier's
coefficient vector --; the rejection matrix and the localisation; the two new headers as C99; the lane code under AddressSanitizer and
UBSan in a stand-alone program; the tally example.  Inputs: tests/or_batch_cases.py."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import or_batch_cases as B
from tests import or_proof_cases as C
from zkp_amd import cabi
from zkp_amd import toolbox as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_STATEMENT = -10


def prove(c, eng=None, threads=0):
    ts = c.transcripts.copy()
    coms, chal, resp, status = T.or_prove_batchable(eng, c.st, ts, c.secrets, c.real, c.inst, c.common, c.entropy, threads)
    return ts, coms, chal, resp, status


@pytest.mark.parametrize("k", C.KS)
@pytest.mark.parametrize("name", C.NAMES)
def test_host_backend_equals_the_model(name, k):
    c = C.case(name, k)
    mts, mcoms, mchal, mresp = B.model(name, k)
    for threads in (1, 3):
        ts, coms, chal, resp, status = prove(c, None, threads)
        assert not status.any() and (coms == mcoms).all() and (chal == mchal).all() and (resp == mresp).all() and (ts == mts).all()
        vts = c.transcripts.copy()
        assert not T.or_verify_batchable(None, c.st, vts, c.inst, c.common, coms, chal, resp, threads).any() and (vts == mts).all()
        bts = c.transcripts.copy()
        assert T.or_batch_verify(None, c.st, bts, c.inst, c.common, coms, chal, resp, B.weights("random", c.n, k, c.st.nc), threads) and (bts == mts).all()
    assert B.model_verify(name, c, 1, mcoms, mchal, mresp)
    assert T.or_batch_verify(None, c.st, c.transcripts.copy(), c.inst, c.common, mcoms, mchal, mresp)          # weights from the operating system


@pytest.mark.parametrize("k", C.KS)
@pytest.mark.parametrize("name", C.NAMES)
def test_the_prover_gives_or_proves_challenges_responses_and_transcripts(name, k):
    c = C.case(name, k)
    ts, _, chal, resp, status = prove(c)
    ots, ochal, oresp, ostatus = c.prove(None)
    assert (ts == ots).all() and (chal == ochal).all() and (resp == oresp).all() and (status == ostatus).all()


@pytest.mark.parametrize("pattern", B.WEIGHT_PATTERNS)
@pytest.mark.parametrize("name,k", [("S1", 1), ("S1", 2), ("S2", 3), ("S3", 5)])
def test_coefficient_vectors_equal_the_models(name, k, pattern):
    c = C.case(name, k)
    _, coms, chal, resp = B.model(name, k)
    w = B.weights(pattern, c.n, k, c.st.nc)
    ok, co = T.or_batch_verify_coeffs(None, c.st, c.transcripts.copy(), c.inst, c.common, coms, chal, resp, w, 3)
    assert ok and (co == B.model_coeffs(name, k, chal, resp, w)).all()


def test_the_group_check_of_the_model_and_of_the_host_backend_agree():
    name, k, n = "S2", 2, 5
    c = C.case(name, k, n)
    _, coms, chal, resp = B.model(name, k, n)
    bad = resp.copy()
    bad[1, 0, 0] = C._bump(resp[1, 0, 0])                             # canonical and hashed nowhere: only the sum can notice
    for pattern in B.WEIGHT_PATTERNS:                                 # (all-zero weights: the sum is the identity whatever the proofs are)
        w = B.weights(pattern, n, k, c.st.nc)
        for rs in (resp, bad):
            want = B.model_batch_verify(name, c, coms, chal, rs, w)
            assert want == (rs is resp or pattern == "zero"), pattern
            assert T.or_batch_verify(None, c.st, c.transcripts.copy(), c.inst, c.common, coms, chal, rs, w) == want, pattern


@pytest.mark.parametrize("name,k", [("S1", 2), ("S2", 3), ("S3", 5)])
def test_each_tampering_fails_the_batch_and_is_located(name, k):
    c = C.case(name, k)
    _, coms, chal, resp = B.model(name, k)
    w = B.weights("random", c.n, k, c.st.nc)
    for what, cm, ch, rs, inst, victim in B.tamperings(c, coms, chal, resp):
        want = np.zeros(c.n, np.uint8)
        want[victim] = 1
        res = T.or_verify_batchable(None, c.st, c.transcripts.copy(), inst, c.common, cm, ch, rs)
        assert (res == want).all(), what
        assert not B.model_verify(name, c, victim, cm, ch, rs, inst), what
        assert not T.or_batch_verify(None, c.st, c.transcripts.copy(), inst, c.common, cm, ch, rs, w), what
        ok, res = T.or_batch_verify_locate(None, c.st, c.transcripts.copy(), inst, c.common, cm, ch, rs, w, 3)
        assert not ok and (res == want).all(), what
    ts = c.transcripts.copy()
    ok, res = T.or_batch_verify_locate(None, c.st, ts, c.inst, c.common, coms, chal, resp, w)
    assert ok and not res.any() and (ts == B.model(name, k)[0]).all()


def test_mixed_strobe_positions_and_the_most_branches():
    c = C.Case("S3", 3, 65, ragged=True)
    ts, coms, chal, resp, status = prove(c, None, 3)
    vts = c.transcripts.copy()
    assert not status.any() and not T.or_verify_batchable(None, c.st, vts, c.inst, c.common, coms, chal, resp, 1).any() and (vts == ts).all()
    assert T.or_batch_verify(None, c.st, c.transcripts.copy(), c.inst, c.common, coms, chal, resp)
    wide = C.Case("S2", 64, 2)
    ts, coms, chal, resp, status = prove(wide)
    assert not status.any() and T.or_batch_verify(None, wide.st, wide.transcripts.copy(), wide.inst, wide.common, coms, chal, resp)
    assert B.model_verify("S2", wide, 1, coms, chal, resp)


def test_argument_errors_write_nothing():
    c = C.case("S1", 2, 33)
    _, coms, chal, resp = B.model("S1", 2, 33)
    lib, p = T.lib(), T._p
    res = np.full(33, 0x5a, np.uint8)
    for k in (0, 65):
        ts = c.transcripts.copy()
        assert lib.zkp_or_batch_verify_batch(None, c.st._h, k, 33, p(ts), p(c.inst), p(c.common), p(coms), p(chal), p(resp), None, 1) == BAD_STATEMENT
        assert lib.zkp_or_verify_batchable_batch(None, c.st._h, k, 33, p(ts), p(c.inst), p(c.common), p(coms), p(chal), p(resp), 1, p(res)) == BAD_STATEMENT
        assert lib.zkp_or_batch_verify_locate(None, c.st._h, k, 33, p(ts), p(c.inst), p(c.common), p(coms), p(chal), p(resp), None, 1, p(res)) == BAD_STATEMENT
        assert (ts == c.transcripts).all() and (res == 0x5a).all()
    ts = c.transcripts.copy()
    ts[7, 200] = 166
    before = ts.copy()
    assert lib.zkp_or_batch_verify_batch(None, c.st._h, 2, 33, p(ts), p(c.inst), p(c.common), p(coms), p(chal), p(resp), None, 1) == BAD_STATEMENT
    assert lib.zkp_or_batch_verify_batch(None, c.st._h, 2, 33, p(before), p(c.inst), p(c.common), None, p(chal), p(resp), None, 1) == BAD_STATEMENT
    assert (ts == before).all()
    assert lib.zkp_or_batch_verify_batch(None, c.st._h, 2, 0, p(ts), p(c.inst), p(c.common), p(coms), p(chal), p(resp), None, 1) == 0 and (ts == before).all()
    assert lib.zkp_or_verify_batchable_batch(None, c.st._h, 2, 0, p(ts), p(c.inst), p(c.common), p(coms), p(chal), p(resp), 1, p(res)) == 0 and (res == 0x5a).all()


def test_threshold_setter_leaves_the_or_threshold_alone():
    old = T.get_or_batch_min_batch()
    T.set_or_batch_min_batch(65)
    assert T.get_or_batch_min_batch() == 65 and T.get_or_min_batch() == 4096
    T.set_or_batch_min_batch(old)


@pytest.mark.parametrize("header", ["zkp_or_batch_mi355x.h", "zkp_or_batch_toolbox.h"])
def test_headers_compile_as_c99_and_every_prototype_is_typed(tmp_path, header):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed"
    src = tmp_path / "use.c"
    src.write_text('#include "%s"\nint main(void) { return ZKP_OR_MAX_BRANCHES == 64 ? 0 : 1; }\n' % header)
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", cabi.INCLUDE, "-c", str(src), "-o", str(tmp_path / "use.o")], check=True,
                   capture_output=True, text=True)
    sigs = cabi.signatures(header)
    want = {"zkp_or_batch_mi355x.h": {"zkp_or_prove_batchable": 14, "zkp_or_verify_batchable": 11, "zkp_or_batch_verify": 13, "zkp_or_prove_batchable_dev": 14,
                                      "zkp_or_verify_batchable_dev": 11, "zkp_or_batch_verify_dev": 12},
            "zkp_or_batch_toolbox.h": {"zkp_or_prove_batchable_batch": 15, "zkp_or_verify_batchable_batch": 12, "zkp_or_batch_verify_batch": 12,
                                       "zkp_or_batch_verify_locate": 13, "zkp_or_batch_verify_coeffs": 13, "zkp_toolbox_set_or_batch_min_batch": 1,
                                       "zkp_toolbox_get_or_batch_min_batch": 0}}[header]
    assert {name: len(args) for name, (_, args) in sigs.items()} == want
    lib = T.lib() if header == "zkp_or_batch_toolbox.h" else None
    for name in (want if lib is not None else ()):
        assert getattr(lib, name).argtypes == sigs[name][1]


def test_lane_code_under_sanitizers(tmp_path):
    """tests/host/or_batch_host_main.cpp, g++ -fsanitize=address,undefined, as a child process: or_batch_lane.h's check, match and
    coefficient items over k = 1, 2, 64 and m = 1, 11, on heap blocks of exactly each buffer's size, against a restatement with plain loops"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed (it builds the host library too)"
    exe = tmp_path / "or_batch_host_main"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "host", "or_batch_host_main.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert r.stdout.split("\n")[:-1] == ["checks %d 0" % (6 * 3), "coeffs %d 0" % (2 * 3 * (1 + 2 + 64))]


def test_the_tally_example_on_the_host():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "vote_1_of_k_tally_batch.py"), "64", "--host"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert "box of 64 ballots: batch check passed" in lines and "box with 2 bad ballots: batch check failed" in lines
    assert "located: ballots 64 and 65" in lines
    cast = int(np.random.default_rng(64).integers(0, 4, size=64).sum())
    assert "tally: %d (cast: %d)" % (cast, cast) in lines
