"""The sign-folded radix-16 recoding of the comb walks and the ladder, and the grouped walk's Horner order, on the host.

tests/host/comb_fold_host_main.cpp is a stand-alone program (its own main) built with g++ -fsanitize=address,undefined and run as a child
process; a second build with -DZKP_FE_TRACK asserts the limb bounds of every field operation of the walk, the merges between and after the
two passes included.  No GPU needed.

(a) sc_fold_recode16 over the catalogue of tests/comb_fold_cases.py: every digit in range, the top digit at most 8 with 0 and 8 reached,
    the digits re-sum to min(s, l - s), the flip bit as the integers give it.
(b) a 16-teeth table built with ge_double / ge_add_cached and walked in the new order -- pass 0: S3 and S2; acc = 16 (16 S3 + S2); pass 1:
    S1 onto acc and S0 in a fresh accumulator; 16 acc + S0 -- without the fold (129 entries, the carry tooth read) and with it (a table of
    exactly 128 entries: a read of the carry tooth would be a heap overflow), and the folded ladder order, against plain double-and-add on
    three points, and against oracle/model.py on one of them."""
import os
import shutil
import subprocess

import pytest

from oracle import model as M
from tests import comb_fold_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = F.L
LOGS = (1, 0x1234567, (L - 1) // 3)                      # the points: k * B
h = lambda v: int(v).to_bytes(32, "little").hex()


def _build(tmp_path, name, extra):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed (it builds the host library too)"
    exe = tmp_path / name
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Wno-unknown-pragmas"] + extra +
                   [os.path.join(ROOT, "tests", "host", "comb_fold_host_main.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    return exe


def _run(exe, tmp_path, lines):
    (tmp_path / "records.txt").write_text("".join(x + "\n" for x in lines))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), str(tmp_path / "records.txt")], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return out


def test_the_catalogue_reaches_both_ends_of_the_top_digit():
    tops = set()
    for s in F.CAT:
        f, _ = F.fold(s)
        d = F.digits(f)
        assert all(-8 <= x <= 7 for x in d[:-1]) and 0 <= d[-1] <= 8
        assert sum(x << (4 * i) for i, x in enumerate(d)) == f
        tops.add(d[-1])
    assert {0, 7, 8} <= tops
    assert {0, 1, F.HALF, F.HALF + 1, L - 1, 2**251 - 1, 2**251, 2**251 + 1, 2**248 - 1, 2**248, 2**248 - F.K62} <= set(F.CAT)
    assert all((L - s) % L in F.CAT for s in F.CAT)


def test_folded_recoding_under_sanitizers(tmp_path):
    exe = _build(tmp_path, "comb_fold_host_main", [])
    vals = F.CAT + [L]                                    # (a vouched scalar may be l itself: it folds to 0)
    out = _run(exe, tmp_path, ["R " + h(s) for s in vals])
    tops = set()
    for s, line in zip(vals, out):
        flip, e = line.split()
        e = int.from_bytes(bytes.fromhex(e), "little")
        f, want_flip = F.fold(s)
        assert int(flip) == want_flip, hex(s)
        d = [((e >> (4 * i)) & 15) - 8 for i in range(F.TOP)] + [e >> (4 * F.TOP)]
        assert d == F.digits(f), hex(s)
        assert all(-8 <= x <= 7 for x in d[:-1]) and 0 <= d[-1] <= 8, hex(s)
        assert sum(x << (4 * i) for i, x in enumerate(d)) == f, hex(s)
        tops.add(d[-1])
    assert 0 in tops and 8 in tops and max(tops) == 8


@pytest.mark.parametrize("track", [False, True], ids=["plain", "fe_track"])
def test_regrouped_walk_and_folded_ladder_equal_double_and_add(tmp_path, track):
    exe = _build(tmp_path, "comb_fold_host_main_" + ("track" if track else "plain"), ["-DZKP_FE_TRACK"] if track else [])
    encs = [M.ristretto_encode(M.pt_mul(k, M.BASEPOINT)) for k in LOGS]
    recs, lines = [], []
    for k, enc in zip(LOGS, encs):
        for s in F.CAT:
            for kind in ("W 0", "W 1", "L 1"):
                recs.append((kind, k, s))
                lines.append("%s %s %s" % (kind, enc.hex(), h(s)))
    out = _run(exe, tmp_path, lines)
    bad = [(r[0], hex(r[2])) for r, line in zip(recs, out) if line.split()[0] != line.split()[1]]
    assert not bad, (len(bad), bad[:6])
    if not track:                                         # the program's double-and-add itself against the model, on one point
        k = LOGS[1]
        for r, line in zip(recs, out):
            if r[1] == k and r[0] == "W 1":
                assert line.split()[1] == M.ristretto_encode(M.pt_mul(r[2] * k % L, M.BASEPOINT)).hex(), hex(r[2])
