"""The batched 1-of-k OR-proofs without a GPU: the toolbox's host route (ctx == NULL: the items of zkp_amd/csrc/or_lane.h on host threads)
against the model of tests/or_proof_model.py over oracle.model, byte for byte; the rejection matrix; branch hiding; the argument errors; the
two headers as C99; the lane code under AddressSanitizer and UBSan in a stand-alone program; the vote example.  Inputs:
tests/or_proof_cases.py."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import or_proof_cases as C
from zkp_amd import cabi
from zkp_amd import toolbox as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_STATEMENT = -10


@pytest.mark.parametrize("k", C.KS)
@pytest.mark.parametrize("name", C.NAMES)
def test_host_proofs_equal_the_model_byte_for_byte(name, k):
    c = C.case(name, k)
    mts, mchal, mresp = C.model(name, k)
    for threads in (1, 3):
        ts, chal, resp, status = c.prove(None, threads)
        assert not status.any() and (chal == mchal).all() and (resp == mresp).all() and (ts == mts).all()
        vts, res = c.verify(None, chal, resp, threads)
        assert not res.any() and (vts == mts).all()
    assert C.model_verify(name, c, 1, mchal, mresp)
    for n in (1, 33):                                                # smaller batches are the model's first proofs
        small = C.case(name, k, n)
        ts, chal, resp, status = small.prove(None, 3)
        assert (chal == mchal[:n]).all() and (resp == mresp[:n]).all() and (ts == mts[:n]).all()


@pytest.mark.parametrize("name,k", [("S1", 2), ("S2", 3), ("S3", 5)])
def test_each_tampering_rejects_its_own_proof_only(name, k):
    c = C.case(name, k)
    _, chal, resp = C.model(name, k)
    for what, ch, rs, inst, victim in C.tamperings(c, chal, resp):
        _, res = c.verify(None, ch, rs, inst=inst)
        want = np.zeros(c.n, np.uint8)
        want[victim] = 1
        assert (res == want).all(), what
        assert not C.model_verify(name, c, victim, ch, rs, inst), what


def test_a_witness_that_does_not_satisfy_the_claimed_branch_is_rejected():
    c = C.case("S2", 3, 33)
    real = c.real.copy()
    real[4] = (real[4] + 1) % 3                                       # claims a branch whose points the witness does not open
    ts = c.transcripts.copy()
    chal, resp, status = T.or_prove(None, c.st, ts, c.secrets, real, c.inst, c.common, c.entropy)
    assert not status.any()
    _, res = c.verify(None, chal, resp)
    want = np.zeros(33, np.uint8)
    want[4] = 1
    assert (res == want).all()


def test_branch_hiding_every_branch_proves_and_the_proofs_differ():
    name, k, n = "S1", 3, 33
    lo = C.Case(name, k, n, real=np.zeros(n))
    # the same keys on every branch: a ring in which the prover knows EVERY key, proved once on branch 0 and once on branch k - 1
    x = lo.secrets
    X, bad = T.point_mul(None, x[:, 0], np.tile(lo.common[0], (n, 1)))
    assert not bad.any()
    inst = np.ascontiguousarray(np.broadcast_to(X, (k, 1, n, 32)))
    proofs = []
    for real in (np.zeros(n, np.uint8), np.full(n, k - 1, np.uint8)):
        ts = lo.transcripts.copy()
        chal, resp, status = T.or_prove(None, lo.st, ts, x, real, inst, lo.common, lo.entropy)
        assert not status.any()
        assert not T.or_verify(None, lo.st, lo.transcripts.copy(), inst, lo.common, chal, resp).any()
        proofs.append((chal, resp))
    assert (proofs[0][0] != proofs[1][0]).any(axis=(1, 2)).all() and (proofs[0][1] != proofs[1][1]).any(axis=(1, 2, 3)).all()


def test_a_witness_that_is_not_reduced_verifies_and_differs():
    c = C.case("S1", 2, 33)
    wide = c.secrets.copy()
    for j in range(33):
        wide[j, 0] = C.add_l(c.secrets[j, 0])
    ts = c.transcripts.copy()
    chal, resp, status = T.or_prove(None, c.st, ts, wide, c.real, c.inst, c.common, c.entropy)
    _, mchal, mresp = C.model("S1", 2, 33)
    assert not status.any() and not c.verify(None, chal, resp)[1].any()
    assert (chal != mchal).any(axis=(1, 2)).all() and (resp != mresp).any(axis=(1, 2, 3)).all()


def test_mixed_strobe_positions_in_one_batch():
    c = C.Case("S3", 3, 65, ragged=True)
    assert len(set(c.transcripts[:, 200].tolist())) > 8
    ts, chal, resp, status = c.prove(None, 3)
    vts, res = c.verify(None, chal, resp, 1)
    assert not status.any() and not res.any() and (vts == ts).all()
    stmt = C.model_statement("S3")
    for j in (0, 1, 36, 64):
        t = C.blob_to_model(c.transcripts[j])
        ch, rs = C.OM.prove(t, stmt, 3, [c.secrets[j, i].tobytes() for i in range(2)], int(c.real[j]),
                            [[c.inst[b, 0, j].tobytes()] for b in range(3)], [c.common[p].tobytes() for p in range(2)], c.entropy[j].tobytes())
        assert b"".join(ch) == chal[j].tobytes() and b"".join(b"".join(r) for r in rs) == resp[j].tobytes() and (C.model_to_blob(t) == ts[j]).all()


def test_the_most_branches_against_the_model():
    c = C.Case("S2", 64, 2)
    ts, chal, resp, status = c.prove(None)
    assert not status.any() and not c.verify(None, chal, resp)[1].any()
    t = C.blob_to_model(c.transcripts[1])
    ch, rs = C.OM.prove(t, C.model_statement("S2"), 64, [c.secrets[1, 0].tobytes()], int(c.real[1]),
                        [[c.inst[b, v, 1].tobytes() for v in range(3)] for b in range(64)], [c.common[0].tobytes()], c.entropy[1].tobytes())
    assert b"".join(ch) == chal[1].tobytes() and b"".join(b"".join(r) for r in rs) == resp[1].tobytes() and (C.model_to_blob(t) == ts[1]).all()


def test_entropy_from_the_operating_system_gives_different_valid_proofs():
    c = C.case("S2", 2, 33)
    a, b = c.prove(None, entropy=None), c.prove(None, entropy=None)
    assert (a[2] != b[2]).any(axis=(1, 2, 3)).all()
    assert not c.verify(None, a[1], a[2])[1].any() and not c.verify(None, b[1], b[2])[1].any()


def test_argument_errors_write_nothing():
    c = C.case("S1", 2, 33)
    lib = T.lib()
    p = T._p

    def prove(k, n, real, ts):
        chal, resp, status = np.full((33, 64, 32), 0x5a, np.uint8), np.full((33, 64, 1, 32), 0x5a, np.uint8), np.full(33, 0x5a, np.uint8)
        inst = np.ascontiguousarray(np.resize(c.inst, (max(k, 1), 1, 33, 32)))
        rc = lib.zkp_or_prove_batch(None, c.st._h, k, n, p(ts), p(c.secrets), p(real), p(inst), p(c.common), p(c.entropy), 1, p(chal), p(resp), p(status))
        return rc, (chal == 0x5a).all() and (resp == 0x5a).all() and (status == 0x5a).all()

    for k in (0, 65):
        ts = c.transcripts.copy()
        assert prove(k, 33, c.real, ts) == (BAD_STATEMENT, True) and (ts == c.transcripts).all()
    real = c.real.copy()
    real[32] = 2
    ts = c.transcripts.copy()
    assert prove(2, 33, real, ts) == (BAD_STATEMENT, True) and (ts == c.transcripts).all()
    ts[7, 200] = 166
    before = ts.copy()
    assert prove(2, 33, c.real, ts) == (BAD_STATEMENT, True) and (ts == before).all()
    ts = c.transcripts.copy()
    assert prove(2, 0, c.real, ts) == (0, True) and (ts == c.transcripts).all()
    res = np.full(33, 0x5a, np.uint8)
    for k in (0, 65):
        rc = lib.zkp_or_verify_batch(None, c.st._h, k, 33, p(ts), p(c.inst), p(c.common), p(c.inst), p(c.inst), 1, p(res))
        assert rc == BAD_STATEMENT and (res == 0x5a).all() and (ts == c.transcripts).all()
    assert lib.zkp_or_verify_batch(None, c.st._h, 2, 0, p(ts), p(c.inst), p(c.common), p(c.inst), p(c.inst), 1, p(res)) == 0 and (res == 0x5a).all()


def test_threshold_setter_and_its_default():
    old = T.get_or_min_batch()
    assert old == 4096                                               # profiles/or_proof_bench.txt: the smallest measured N, ahead at every shape
    T.set_or_min_batch(65)
    assert T.get_or_min_batch() == 65
    T.set_or_min_batch(old)


@pytest.mark.parametrize("header", ["zkp_or_mi355x.h", "zkp_or_toolbox.h"])
def test_headers_compile_as_c99_and_every_prototype_is_typed(tmp_path, header):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed"
    src = tmp_path / "use.c"
    src.write_text('#include "%s"\nint main(void) { return ZKP_OR_MAX_BRANCHES == 64 ? 0 : 1; }\n' % header)
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", cabi.INCLUDE, "-c", str(src), "-o", str(tmp_path / "use.o")], check=True,
                   capture_output=True, text=True)
    sigs = cabi.signatures(header)
    want = {"zkp_or_mi355x.h": {"zkp_or_prove": 13, "zkp_or_verify": 10, "zkp_or_prove_dev": 13, "zkp_or_verify_dev": 10},
            "zkp_or_toolbox.h": {"zkp_or_prove_batch": 14, "zkp_or_verify_batch": 11, "zkp_toolbox_set_or_min_batch": 1, "zkp_toolbox_get_or_min_batch": 0}}[header]
    assert {name: len(args) for name, (_, args) in sigs.items()} == want
    lib = T.lib() if header == "zkp_or_toolbox.h" else None
    for name in (want if lib is not None else ()):
        assert getattr(lib, name).argtypes == sigs[name][1]


def test_lane_code_under_sanitizers(tmp_path):
    """tests/host/or_proof_host_main.cpp, g++ -fsanitize=address,undefined, as a child process: or_lane.h's assemble / respond / check /
    verdict items over k = 1, 2, 64 and m = 1, 11 with every branch as the real one, on heap blocks of exactly each buffer's size, against a
    restatement with plain branches"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed (it builds the host library too)"
    exe = tmp_path / "or_proof_host_main"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "host", "or_proof_host_main.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    cases = 2 * (1 + 2 + 64)
    assert r.stdout.split("\n")[:-1] == ["masks 4900 0", "rows %d 0" % cases, "proofs %d 0" % cases, "verdicts %d 0" % cases]


def test_the_vote_example_on_the_host():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "vote_1_of_k_batch.py"), "64", "--host"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert "ballots verified: 64 of 64" in lines and "v = 4 ballot: rejected" in lines and "tampered ballot: rejected" in lines
    cast = int(np.random.default_rng(64).integers(0, 4, size=64).sum())
    assert "tally: %d (cast: %d)" % (cast, cast) in lines
