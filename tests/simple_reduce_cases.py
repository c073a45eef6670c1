"""The cases of SimpleAgg's reduce route (SQLRS_SIMPLE_AGG_REDUCE of sqlrs_simple_agg_create), shared by test_simple_agg_reduce_cpu.py (the conditions
the GPU file relies on, the oracle against the model) and test_gpu_simple_agg_reduce.py (the device against the model).

A case is agg_edge_cases.build(..., groups=1): ONE key value, the columns f, g (float64), i (int64), j (int32) of that file with
their edge values, cut into 1 - 3 batches.  With one group the builder plants no NaN / Inf group, so SUM(f) is compared inside
the any-order bound in every case, never by class (asserted on the CPU).

Filters are BoundExprs over the batch [k, f, g, i, j]; which rows they keep comes from expr_model.evaluate, never from the
library.  `kept_model` is the model (agg_model.aggregate) of the kept rows; computed arguments are evaluated with numpy /
Python integers here, validity included."""
import functools

import numpy as np
import pyarrow as pa

import agg_edge_cases as E
import agg_model as M
import expr_model as X
from sqlrs_amd import abi
from sqlrs_amd.expr import AggFunc, Constant, InputRef, TypeCast

SIZES = [1, 63, 64, 65, 4097, 100_003, 4_194_381]  # the last: 2 * 2^21 + 77 — two full sweeps of the kernel's grid, then a tail of 77 rows
NULLABLE = [None, "random", "flip64"]
SPECS = {}
for _s, _n in enumerate(SIZES):
    for _v, _nullable in enumerate(NULLABLE):
        SPECS[f"n{_n}_{_nullable or 'plain'}"] = dict(n=_n, seed=1000 + 10 * _s + _v, groups=1, nullable=_nullable, batches=1 + (_s + _v) % 3)
SMALL = [k for k, v in SPECS.items() if v["n"] <= 100_003]
LARGE = [k for k, v in SPECS.items() if v["n"] > 100_003]
ORACLE = [k for k, v in SPECS.items() if v["n"] <= 4097]
F, G, I, J = 1, 2, 3, 4  # column numbers in a case's batches


@functools.lru_cache(maxsize=4)
def case(name) -> E.Case:
    return E.build(name, **SPECS[name])


def with_empty(batches):
    """the case's batches with a zero-row batch behind the first one"""
    return [batches[0], batches[0].slice(0, 0)] + list(batches[1:])


def with_nans(c: E.Case) -> E.Case:
    """`c` with positive NaNs (quiet, and all ones: the top of the total order) in every 97th slot of f.  They are above every g, so
    `f < g` drops them and SUM(f) of the kept rows stays a value"""
    f, valid = c.cols["f"]
    f = f.copy()
    f[::97] = np.array([0x7FF8000000000000, 0x7FFFFFFFFFFFFFFF], np.uint64).view(np.float64)[np.arange(len(f[::97])) % 2]
    cols = dict(c.cols)
    cols["f"] = (f, valid)
    return E.Case(c.name + "_nans", c.keys, c.key_valid, cols, c.bounds, c.arrival)


def with_zero_divisors(c: E.Case, rows) -> E.Case:
    """`c` with j = 0 in `rows`"""
    j, valid = c.cols["j"]
    j = j.copy()
    j[rows] = 0
    cols = dict(c.cols)
    cols["j"] = (j, valid)
    return E.Case(c.name + "_zeros", c.keys, c.key_valid, cols, c.bounds, c.arrival)


# ---- filters -------------------------------------------------------------------------------------------------------------------
C1, C2, C3 = (1 << 62) - 500, (1 << 62) + 900, 100.0
FILTERS = {
    "i_gt_c": lambda: InputRef(I) > Constant(0, abi.INT64),                      # (over a nullable i: NULL mask slots)
    "f_lt_g": lambda: InputRef(F) < InputRef(G),                                 # (doubles, NaNs among them: total order)
    "j_ge_c_and_g_lt_c": lambda: (InputRef(J) >= Constant(-(1 << 30), abi.INT32)) & (InputRef(G) < Constant(0.5, abi.FLOAT64)),
    "false": lambda: Constant(False, abi.BOOLEAN),
    "range_and_g": lambda: ((InputRef(I) >= Constant(C1, abi.INT64)) & (InputRef(I) < Constant(C2, abi.INT64))) & (InputRef(G) < Constant(C3, abi.FLOAT64)),
}
FILTER_CASES = [("i_gt_c", "n4097_random", False), ("i_gt_c", "n100003_flip64", False), ("f_lt_g", "n4097_plain", True), ("f_lt_g", "n100003_random", True),
                ("j_ge_c_and_g_lt_c", "n4097_flip64", False), ("j_ge_c_and_g_lt_c", "n100003_plain", False),
                ("false", "n4097_plain", False), ("false", "n100003_random", False),
                ("range_and_g", "n4097_random", False), ("range_and_g", "n100003_plain", False)]  # (filter, case, NaNs planted in f)


@functools.lru_cache(maxsize=None)
def filter_case(fname, cname, nans):
    """(case, the filter, mask values per row: 1 / 0 / None) — the mask is expr_model's"""
    c = with_nans(case(cname)) if nans else case(cname)
    expr = FILTERS[fname]()
    whole = pa.Table.from_batches(c.batches()).combine_chunks().to_batches()[0]
    res = X.evaluate(expr, whole)
    assert res.dtype == abi.BOOLEAN and all(s == X.EXACT for s in res.state)
    return c, expr, res.vals


def kept_of(mask):
    return np.array([v == 1 for v in mask], bool)


# ---- the model of the kept rows ------------------------------------------------------------------------------------------------
def kept_model(c: E.Case, kept, funcs, args=None) -> M.Groups:
    """agg_model over the rows of `c` where `kept`; `args`: {name: (values, valid or None)} in place of the case's columns, `funcs`
    [(name, argument name)]"""
    args = dict(c.cols) if args is None else args
    names = list(args)
    rows = np.nonzero(kept)[0]
    sub = [(np.asarray(args[a][0])[rows], None if args[a][1] is None else np.asarray(args[a][1])[rows]) for a in names]
    return M.aggregate(c.keys[rows], None, sub, [(f, names.index(a)) for f, a in funcs])


def compare_one_row(got: pa.RecordBatch, exp: M.Groups, funcs, label=""):
    """the operator's one row against the model's single group — or, when no row was kept, COUNT = 0 and NULL for the others"""
    assert got.num_rows == 1 and got.num_columns == len(funcs), (label, got.num_rows, got.num_columns)
    if len(exp) == 0:
        assert [col.to_pylist() for col in got.columns] == [[0] if f == "count" else [None] for f, _ in funcs], label
        return 0
    assert len(exp) == 1, label
    table = pa.Table.from_batches([got]).add_column(0, "k", pa.array(exp.keys, type=pa.int64()))
    return M.compare(table, exp, label)


def _valid(c, name):
    v = c.cols[name][1]
    return np.ones(c.n, bool) if v is None else v


def computed_args(c: E.Case):
    """{f*g, i+j, j*j, f}: f * g one IEEE multiplication, i + cast(j as int64) wrapping at 64 bits, j * j wrapping at 32 bits (and
    widened for its SUM), NULL where an operand is"""
    f, g, i, j = (c.cols[k][0] for k in "fgij")
    with np.errstate(over="ignore"):
        ij = (i.view(np.uint64) + j.astype(np.int64).view(np.uint64)).view(np.int64)
        jj = (j.astype(np.int64) * j.astype(np.int64)).astype(np.int32)  # (the exact product, cut to its low 32 bits)
    return {"f*g": (f * g, _valid(c, "f") & _valid(c, "g")), "i+j": (ij, _valid(c, "i") & _valid(c, "j")), "j*j": (jj, c.cols["j"][1]),
            "f": (f, c.cols["f"][1])}


COMPUTED_FUNCS = [("sum", "f*g"), ("sum", "i+j"), ("sum", "j*j"), ("count", "f")]


def computed_aggs():
    return [AggFunc("sum", InputRef(F) * InputRef(G), abi.FLOAT64), AggFunc("sum", InputRef(I) + TypeCast(InputRef(J), abi.INT64), abi.INT64),
            AggFunc("sum", InputRef(J) * InputRef(J), abi.INT64), AggFunc("count", InputRef(F), abi.INT64)]


def quotient_arg(c: E.Case, rows):
    """i / cast(j as int64) on `rows` (every one with j != 0 where both are valid): truncating, INT64_MIN / -1 wraps"""
    i, j = c.cols["i"][0], c.cols["j"][0]
    valid = _valid(c, "i") & _valid(c, "j")
    q = np.zeros(c.n, np.int64)
    for r in np.nonzero(rows & valid)[0].tolist():
        a, b = int(i[r]), int(j[r])
        mag = abs(a) // abs(b)
        q[r] = M.wrap_i64(mag if (a < 0) == (b < 0) else -mag)
    return {"i/j": (q, valid)}


def quotient_aggs():
    return [AggFunc("sum", InputRef(I) / TypeCast(InputRef(J), abi.INT64), abi.INT64), AggFunc("count", InputRef(I) / TypeCast(InputRef(J), abi.INT64), abi.INT64)]


QUOTIENT_FUNCS = [("sum", "i/j"), ("count", "i/j")]
