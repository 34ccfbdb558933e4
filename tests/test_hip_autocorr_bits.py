"""Every spatial-autocorrelation entry against the bits recorded in tests/golden/extra_autocorr_bits.npz (layout and cases:
tests/autocorr_bits_cases.py): the gene entries, the column entries, the four permutation functions and the residual entries
on the GPU, the plan queries on the host."""
import functools

import numpy as np
import pytest

import autocorr_bits_cases as A


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(A.PATH) as z:
        return {k: z[k] for k in z.files}


def _check(got: dict, prefix: str):
    want = {k: v for k, v in _golden().items() if k.startswith(prefix + "/")}
    assert set(got) == set(want) and want                     # every recorded array is recomputed, and nothing else
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_plan_queries_return_the_recorded_values():
    _check(A.plans(), "plan")


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted(A.GROUPS))
def test_entries_give_the_recorded_bits(group):
    _check(A.GROUPS[group](), group)
