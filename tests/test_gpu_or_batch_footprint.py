"""The six calls of include/zkp_or_batch_mi355x.h write their own output rows and nothing else on the MI355X, advance the transcripts to
the model's bytes and leave their inputs alone: the check of tests/footprint_cases.py over the cases of tests/or_batch_cases.py.  The _dev
forms get views into torch.uint8 device tensors at the least alignment the header accepts, the host-pointer forms views into numpy arrays
at odd addresses.  tests/test_host_or_batch_footprint.py has the completeness check."""
import pytest

from tests import footprint_cases as F
from tests import or_batch_cases as B

pytestmark = pytest.mark.gpu
DEV, HOST = B.footprint_cases("dev"), B.footprint_cases("host")


@pytest.fixture(scope="module")
def eng():
    from zkp_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("case", DEV, ids=[c.id for c in DEV])
def test_dev_call_writes_its_rows_and_nothing_else(eng, case):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch cannot see the GPU in this process (its HIP runtime must initialise before libzkp_mi355x.so: run with -m gpu)")
    failures = F.run_case(case, eng._lib, eng._h, device=True)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", HOST, ids=[c.id for c in HOST])
def test_host_pointer_call_writes_its_rows_and_nothing_else(eng, case):
    failures = F.run_case(case, eng._lib, eng._h, device=False)
    assert not failures, "\n".join(failures)
