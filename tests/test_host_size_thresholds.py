"""Every size threshold of the sources has a row in tests/size_thresholds.py with the same value (no GPU needed).

The thresholds are parsed out of zkp_amd/csrc/zkp_kernels.hip and fused_flows.h: the integer k-constants (constexpr kName = value), the
literal boundaries of the size rules (n < (1u << 18), N >= 65536, n_terms >= 1024), the default of ZKP_OPT_BATCH_ENCODE_MIN and the
encoder's block size.  Retuning one of them, or adding a new one, without its row fails here on any machine.  The parser's reach: k-constants,
and comparisons of n / N / n_terms / n_msm / n_each / total against literals of three or more digits or (1u << b); the size rules outside it are
listed with their reasons in size_thresholds.UNPARSED_RULES."""
import os
import re

import pytest

from tests import size_thresholds as S

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zkp_amd", "csrc")
SOURCES = ("zkp_kernels.hip", "fused_flows.h")


def _int(expr: str) -> int:
    expr = re.sub(r"(?<=[0-9a-fA-F])(ull|ul|u)\b", "", expr.strip())
    assert re.fullmatch(r"[0-9x<\s()]+", expr), expr
    return int(eval(expr))          # digits and shifts only (checked above)


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _k_constants(text):
    """{name: value} of every `constexpr <type> kName = <int>[, kOther = <int>]` declaration"""
    out = {}
    for decl in re.finditer(r"constexpr\s+[\w:]+\s+(k[A-Z]\w*\s*=\s*[^;]+);", text):
        for name, val in re.findall(r"(k[A-Z]\w*)\s*=\s*([0-9][0-9a-fA-Fxu]*(?:\s*<<\s*[0-9]+)?)", decl.group(1)):
            out.setdefault(name, set()).add(_int(val))
    return out


def _literal_boundaries(text):
    """[(as written, value)] of the size comparisons against literals: n < (1u << 21), N >= 65536, n_terms >= 1024, ..."""
    out = []
    for m in re.finditer(r"\b(n|N|n_terms|n_msm|n_each|total)\s*(<|<=|>=|>)\s*(\(1u << [0-9]+\)|[0-9]{3,}\b)", text):
        lit = m.group(3).strip("()")
        out.append((m.group(0), lit, _int(lit)))
    return out


CMZ_TERMS_PER_PROOF = 31                 # bench.cmz_shape: 11 commitment MSMs, 31 terms per proof


def _call_size(r, n):
    """a row's size in the unit its boundary counts: prove_cmz rows list proofs against term thresholds"""
    return CMZ_TERMS_PER_PROOF * n if r["entry"] == "prove_cmz" else n


def _first_upper(r):
    """the smallest size that takes the upper choice: kSmallOptional is compared with <= (n <= 192: the per-term path)"""
    return r["value"] + 1 if r["const"] == "kSmallOptional" else r["value"]


def _rows_for(const):
    return [r for r in S.ROWS if r["const"] == const]


def test_rows_are_well_formed():
    keys = {"row", "name", "const", "value", "source", "entry", "schedule", "sizes", "unit", "key", "expect", "option", "unreachable"}
    for r in S.ROWS:
        assert set(r) == keys, r
        assert r["source"] in SOURCES, r
        assert r["schedule"] in ("latency", "throughput"), r
        assert len(r["sizes"]) == len(r["expect"]) >= 2, r
        assert list(r["sizes"]) == sorted(r["sizes"]), r
        # the sizes sit on both sides of the boundary: one below the first size of the upper choice, one at it or above
        # (rows counted in other units -- proofs of a 1 + 5 N term MSM, outputs per block of blocks, points per ladder block -- are checked
        #  in test_expectations_follow_from_the_value)
        if r["row"] not in ("3b", 2, 9):
            assert _call_size(r, min(r["sizes"])) < _first_upper(r) <= _call_size(r, max(r["sizes"])), r
        if r["entry"] == "prove_cmz":           # the nearest N on each side
            assert _call_size(r, max(r["sizes"]) - 1) < _first_upper(r) <= _call_size(r, max(r["sizes"])), r
        assert r["unreachable"] is None or (isinstance(r["unreachable"], str) and r["unreachable"]), r
    ids = [S.row_id(r, n) for r in S.ROWS for n in r["sizes"]]
    assert len(ids) == len(set(ids)), "duplicate test ids"


def test_every_k_constant_has_a_row_or_a_reason():
    for src in SOURCES:
        for name, values in _k_constants(_read(src)).items():
            if name in S.NOT_THRESHOLDS:
                continue
            rows = _rows_for(name)
            assert rows, "%s (%s = %s) is neither a row of tests/size_thresholds.py nor listed in NOT_THRESHOLDS" % (src, name, sorted(values))
            for r in rows:
                assert {r["value"]} == values, "%s: %s = %s in the sources, %s in the table" % (src, name, sorted(values), r["value"])


def test_every_literal_boundary_has_a_row():
    found = []
    for src in SOURCES:
        for text, lit, value in _literal_boundaries(_read(src)):
            found.append((src, text, lit, value))
    assert found, "the size rules were not found: has the parser gone stale?"
    for src, text, lit, value in found:
        consts = (lit, "N >= %s" % lit, "n_terms >= %s" % lit)
        rows = [r for c in consts for r in _rows_for(c)]
        assert rows, "%s: `%s` has no row in tests/size_thresholds.py" % (src, text)
        assert all(r["value"] == value for r in rows), (src, text, rows)


def test_known_rules_are_parsed():
    """the parser sees what the table says it should: a rule it stopped seeing would otherwise pass unnoticed"""
    lits = {(src, lit) for src in SOURCES for _, lit, _ in _literal_boundaries(_read(src))}
    for want in (("zkp_kernels.hip", "1u << 12"), ("zkp_kernels.hip", "1u << 13"), ("zkp_kernels.hip", "1u << 18"), ("zkp_kernels.hip", "1u << 21"),
                 ("zkp_kernels.hip", "1024"), ("fused_flows.h", "16384"), ("fused_flows.h", "32768"), ("fused_flows.h", "65536")):
        assert want in lits, want
    ks = {}
    for src in SOURCES:
        ks.update(_k_constants(_read(src)))
    for r in S.ROWS:
        if re.fullmatch(r"k[A-Z]\w*", r["const"]):
            assert ks.get(r["const"]) == {r["value"]}, (r["const"], ks.get(r["const"]), r["value"])


def test_option_default_and_encoder_block():
    k = _read("zkp_kernels.hip")
    m = re.search(r"uint64_t batch_encode_min\s*=\s*([0-9]+);", k)
    assert m, "zkp_ctx::batch_encode_min not found"
    assert [r["value"] for r in _rows_for("batch_encode_min")] == [int(m.group(1))]
    m = re.search(r"constexpr int ENC_BLOCK\s*=\s*([0-9]+);", k)
    assert m, "ENC_BLOCK not found"
    rows = _rows_for("ENC_BLOCK")
    assert rows and all(r["value"] == int(m.group(1)) for r in rows)
    # the encoder's inversion groups: ENC_BLOCK blocks of ENC_BLOCK outputs per k_encode_invert block
    b = int(m.group(1))
    for r in rows:
        assert [-(-(-(-n // b)) // b) for n in r["sizes"]] == list(r["expect"]), r


@pytest.mark.parametrize("r", S.ROWS, ids=[S.row_id(r, r["sizes"][-1]) for r in S.ROWS])
def test_expectations_follow_from_the_value(r):
    """each row's expected choices change exactly at its boundary (the expectations are not copied from a GPU run)"""
    below = [e for n, e in zip(r["sizes"], r["expect"]) if _call_size(r, n) < _first_upper(r)]
    above = [e for n, e in zip(r["sizes"], r["expect"]) if _call_size(r, n) >= _first_upper(r)]
    if r["unreachable"]:
        return                     # the row says why the choice cannot flip for a default call
    if r["key"] == "enc_groups":
        return                     # several boundaries: test_option_default_and_encoder_block
    if r["row"] == "3b":           # DLEQ batch MSM: 1 + 5 N terms against kSmallOptional
        assert [int(1 + 5 * n > r["value"]) for n in r["sizes"]] == list(r["expect"])
        return
    if r["key"] == "ladder_interleave":    # ceil(single-use points / 256) ladder blocks against kInterleaveLadderBlocks
        assert [int(-(-n // 256) >= r["value"]) for n in r["sizes"]] == list(r["expect"])
        return
    assert below and above, r
    assert len(set(below)) == 1 and len(set(above)) == 1, r
    if not (r["key"] == "grouped" and r["const"] == "kGroupedCombTerms"):    # (the walk stays on across that one, see the table)
        assert below[0] != above[0], r


def test_unparsed_rules_have_reasons():
    assert all(isinstance(v, str) and v for v in S.UNPARSED_RULES.values())
    ff = _read("fused_flows.h")
    assert "pl.N >= 2 ? pl.s.ns : 0" in ff and "pl.N >= 6 ? 16 : 4" in ff, "each_terms_cfg changed: update size_thresholds.UNPARSED_RULES"
