"""The conditions test_gpu_simple_agg_reduce.py relies on, asserted without a device, and the CPU oracle against the model on
the small cases (tests/simple_reduce_cases.py).

1. SUM(f64) is compared by VALUE in every case: the single group of a case is never of a class (NaN / Inf / all zero) that
   agg_model compares by class.
2. The masks of the filters come from expr_model; every filter keeps between a tenth and nine tenths of its case's rows (the
   constant-false one: none), one has NULL mask slots, one compares doubles with NaNs among them.
3. FilterExecutor -> SimpleAggExecutor on the oracle (what SimpleAggExecutor(..., child_filter=) runs on a backend that is not the HIP
   library) equals the model of the kept rows."""
import numpy as np
import pytest

import agg_edge_cases as E
import agg_model as M
import simple_reduce_cases as S
from sqlrs_amd.executor import SimpleAggExecutor


@pytest.mark.parametrize("name", list(S.SPECS))
def test_sum_f64_is_compared_by_value(name):
    c = S.case(name)
    exp = c.model(E.ALL_FUNCS, classes_only=True)
    assert len(exp) == 1
    shares = M.class_share(exp)
    assert len(shares) == 2 and all(by_class == 0 for by_class, _ in shares), shares  # (sum(f), sum(g))


def test_the_cases_cover_sizes_batches_and_validity():
    assert sorted({v["n"] for v in S.SPECS.values()}) == S.SIZES
    for n in S.SIZES:
        mine = [v for v in S.SPECS.values() if v["n"] == n]
        assert {v["nullable"] for v in mine} == {None, "random", "flip64"}
        assert {v["batches"] for v in mine} == {1, 2, 3}
    assert (1 << 22) < S.SIZES[-1] < 3 * (1 << 21) and S.SIZES[-1] % 64  # a third sweep of the 2^21-row grid, with a ragged tail


@pytest.mark.parametrize("fname,cname,nans", S.FILTER_CASES)
def test_filter_masks(fname, cname, nans):
    c, _, mask = S.filter_case(fname, cname, nans)
    share = S.kept_of(mask).mean()
    if fname == "false":
        assert share == 0 and all(v == 0 for v in mask)
    else:
        assert 0.1 <= share <= 0.9, share
    if nans:
        f = c.cols["f"][0]
        assert np.isnan(f).sum() >= c.n // 97 and not np.isnan(f[S.kept_of(mask)]).any()


def test_filter_masks_have_null_slots_and_nans():
    nulls = [k for k in S.FILTER_CASES if any(v is None for v in S.filter_case(*k)[2])]
    assert any(f == "i_gt_c" for f, _, _ in nulls), nulls
    assert any(nans and f == "f_lt_g" for f, _, nans in S.FILTER_CASES)


@pytest.mark.parametrize("name", S.ORACLE)
def test_oracle_without_filter(oracle, name):
    c = S.case(name)
    (out,) = list(SimpleAggExecutor(oracle, E.agg_funcs(E.ALL_FUNCS), S.with_empty(c.batches()), reduce=True).execute())
    S.compare_one_row(out, c.model(E.ALL_FUNCS), E.ALL_FUNCS, name)


@pytest.mark.parametrize("fname,cname,nans", [k for k in S.FILTER_CASES if k[1] in S.ORACLE])
def test_oracle_filter_below_simple_agg(oracle, fname, cname, nans):
    c, expr, mask = S.filter_case(fname, cname, nans)
    if fname == "range_and_g":
        ex = SimpleAggExecutor(oracle, S.computed_aggs(), c.batches(), child_filter=expr)
        exp, funcs = S.kept_model(c, S.kept_of(mask), S.COMPUTED_FUNCS, S.computed_args(c)), S.COMPUTED_FUNCS
    else:
        ex = SimpleAggExecutor(oracle, E.agg_funcs(E.ALL_FUNCS), c.batches(), child_filter=expr)
        exp, funcs = S.kept_model(c, S.kept_of(mask), E.ALL_FUNCS), E.ALL_FUNCS
    (out,) = list(ex.execute())
    assert ex.reduced_batches == 0
    S.compare_one_row(out, exp, funcs, f"{fname} {cname}")
