"""zkp_or_prove_batch / zkp_or_verify_batch on the host backend (ctx == NULL, 1 and 3 threads) write their own output rows and nothing else,
advance the transcripts to the model's bytes and leave their inputs alone: the check of tests/footprint_cases.py over the cases of
tests/or_proof_cases.py.  And the completeness check of the two OR headers: every function of theirs with a non-const pointer parameter
has a case.  No GPU needed."""
import pytest

from tests import footprint_cases as F
from tests import or_proof_cases as C
from tests.test_host_footprint import writers
from zkp_amd import toolbox as T

BATCH = C.footprint_cases("batch")


@pytest.mark.parametrize("case", BATCH, ids=[c.id for c in BATCH])
def test_batch_call_writes_its_rows_and_nothing_else(case):
    failures = F.run_case(case, T.lib(), None, device=False)
    assert not failures, "\n".join(failures)


def test_every_function_of_the_or_headers_that_writes_through_a_pointer_has_a_case():
    covered = {c.fn for form in C.FOOTPRINT_FUNCTIONS for c in C.footprint_cases(form)}
    assert set(writers("zkp_or_mi355x.h")) == set(C.FOOTPRINT_FUNCTIONS["host"] + C.FOOTPRINT_FUNCTIONS["dev"])
    assert set(writers("zkp_or_toolbox.h")) == set(C.FOOTPRINT_FUNCTIONS["batch"])
    assert set(writers("zkp_or_mi355x.h")) | set(writers("zkp_or_toolbox.h")) <= covered
