"""The workspace each host-pointer call asks for, pinned byte for byte.

A host-pointer entry point carves its staging regions and the launcher's own space out of the context's one workspace, in a fixed order with fixed
sizes.  That layout is what the residue tests and the layout tables describe, so host-side changes must leave it alone: every
case of tests/staged_ws_cases.py makes its one call on a fresh test-hook context, and zkp_debug_ws_bytes -- what that call asked ensure_ws for, plus
ensure_ws's eighth -- must equal the figure in tests/golden/staged_ws_bytes.json, which tools/record_staged_ws_bytes.py recorded at the commit
named in the file, before the calls were moved onto the staging helper."""
import json
import os

import pytest

from tests.staged_ws_cases import CASES

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "staged_ws_bytes.json")


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)["ws_bytes"]


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_ws_bytes(name, recorded):
    from zkp_amd.engine import Engine
    eng = Engine(0, test_hooks=True)
    try:
        assert eng.debug_ws_bytes() == 0
        CASES[name](eng)
        got = eng.debug_ws_bytes()
    finally:
        eng.close()
    print("%s: %d bytes (recorded: %d)" % (name, got, recorded[name]))
    assert got == recorded[name]
