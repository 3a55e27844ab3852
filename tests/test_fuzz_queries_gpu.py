"""The randomised sweep of the query entry points (tests/fuzz_queries.py) in its bounded form: one test per family, a
fixed seed and a fixed number of cases (fuzz_queries.SUITE), the device against the family's restatement for equality.
tests/test_fuzz_queries.py shows, without a GPU, that these case lists are not empty-handed.  The CPU restatements take
most of each test's time; the device's share is printed."""
import pytest

import fuzz_queries as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family", F.FAMILIES)
def test_family(vcp_ctx, oracle, family):
    count, seed = F.SUITE[family]
    F.ctx = vcp_ctx  # the session's context (run() leaves a context it did not create open)
    try:
        done = F.run(cases=count * 2 if family in F.HALF else count, seed=seed, families=(family,), quiet=True)
    finally:
        F.ctx = None
    print("%s: %.2f s references, %.2f s device and comparison" % (family, F.spent[family][0], F.spent[family][1]))
    assert done == {family: count}
