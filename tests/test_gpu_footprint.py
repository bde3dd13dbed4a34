"""Every call of include/zkp_mi355x.h that writes through a pointer of the caller's writes its own output rows and nothing else, and leaves its
inputs alone, on the MI355X: the catalogue and the check of tests/footprint_cases.py.  The _dev forms get views into the middle of torch.uint8
device tensors at the least alignment the header promises to accept, the host-pointer forms views into numpy arrays at odd addresses; guards of
256 rows on both sides hold what a tail lane of the last workgroup, a status store of the wrong width or a download that is a row too long
would write.  All cases share one context; the calls are made through the raw C ABI (no wrapper copy stands between a call and the guards).
tests/test_host_footprint.py has the completeness test and the check's own test."""
import pytest

from oracle import cbind as C
from tests import footprint_cases as F

pytestmark = pytest.mark.gpu
DEV, HOST = F.cases("dev"), F.cases("host")


@pytest.fixture(scope="module")
def eng():
    from zkp_amd.engine import Engine
    C.build()
    e = Engine(0)
    yield e
    e.close()


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch cannot see the GPU in this process (its HIP runtime must initialise before libzkp_mi355x.so: run with -m gpu)")
    return torch


@pytest.mark.parametrize("case", DEV, ids=[c.id for c in DEV])
def test_dev_call_writes_its_rows_and_nothing_else(eng, case):
    _torch()
    failures = F.run_case(case, eng._lib, eng._h, device=True)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", HOST, ids=[c.id for c in HOST])
def test_host_pointer_call_writes_its_rows_and_nothing_else(eng, case):
    failures = F.run_case(case, eng._lib, eng._h, device=False)
    assert not failures, "\n".join(failures)
