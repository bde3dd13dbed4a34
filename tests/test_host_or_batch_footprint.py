"""The toolbox calls of include/zkp_or_batch_toolbox.h on the host backend (ctx == NULL, 1 and 3 threads) write their own output rows and
nothing else, advance the transcripts to the model's bytes and leave their inputs alone: the check of tests/footprint_cases.py over the cases
of tests/or_batch_cases.py.  And the completeness check of the two new headers: every function of theirs with a non-const pointer parameter
has a case.  No GPU needed."""
import pytest

from tests import footprint_cases as F
from tests import or_batch_cases as B
from tests.test_host_footprint import writers
from zkp_amd import toolbox as T

BATCH = B.footprint_cases("batch")


@pytest.mark.parametrize("case", BATCH, ids=[c.id for c in BATCH])
def test_batch_call_writes_its_rows_and_nothing_else(case):
    failures = F.run_case(case, T.lib(), None, device=False)
    assert not failures, "\n".join(failures)


def test_every_function_of_the_new_headers_that_writes_through_a_pointer_has_a_case():
    covered = {c.fn for form in B.FOOTPRINT_FUNCTIONS for c in B.footprint_cases(form)}
    assert set(writers("zkp_or_batch_mi355x.h")) == set(B.FOOTPRINT_FUNCTIONS["host"] + B.FOOTPRINT_FUNCTIONS["dev"])
    assert set(writers("zkp_or_batch_toolbox.h")) == set(B.FOOTPRINT_FUNCTIONS["batch"])
    assert set(writers("zkp_or_batch_mi355x.h")) | set(writers("zkp_or_batch_toolbox.h")) <= covered
