"""sqlrs_hash_join_set_async_filter: the cases of tests/test_async_join_filter_cpu.py and tests/test_gpu_async_join_filter.py,
and the eligibility rule of include/sqlrs_hip.h restated from the batch, the build side's true M, the filter's nodes and the
header's constants (no library call: numpy and pyarrow only).  The unfiltered part of the rule — rows x M, the byte formulas,
Utf8 reservations — is the one of tests/async_utf8_cases.py."""
import numpy as np
import pyarrow as pa

from async_utf8_cases import SA_MAX_OUT_ROWS, eligible as eligible_unfiltered, max_run, rand_strings, str_array
from sqlrs_amd import abi
from sqlrs_amd.expr import Constant, InputRef, JoinCondition, TypeCast

SA_PROG_MAX, SA_STACK_MAX = 24, 8  # (sqlrs_hip.h / csrc/small_async.hpp)
JOIN_TYPES = ["inner", "left", "right", "full"]
FORMS = ["unique_dense", "unique_sparse", "dup_dense", "dup_sparse"]
NUMERIC = (abi.INT32, abi.INT64, abi.FLOAT64)


# ---- the rule ---------------------------------------------------------------------------------------------------------
def filter_compiles(expr, dtypes):
    """the header's "the filter must compile", over the joined schema's dtypes"""
    nodes = expr.nodes()
    if not nodes or len(nodes) > SA_PROG_MAX:
        return False
    st = []
    for n in nodes:
        if n.op == abi.EXPR_INPUT_REF:
            if not 0 <= n.index < len(dtypes) or dtypes[n.index] not in NUMERIC or len(st) >= SA_STACK_MAX:
                return False
            st.append(dtypes[n.index])
        elif n.op == abi.EXPR_CONSTANT:
            if n.dtype not in NUMERIC + (abi.BOOLEAN,) or len(st) >= SA_STACK_MAX:
                return False
            st.append(n.dtype)
        elif n.op == abi.EXPR_TYPE_CAST:
            if not st:
                return False
            if st[-1] != n.dtype:
                if n.dtype not in NUMERIC or st[-1] not in NUMERIC + (abi.BOOLEAN,):
                    return False
                st[-1] = n.dtype
        else:
            if len(st) < 2:
                return False
            r, l = st.pop(), st.pop()
            if abi.EXPR_PLUS <= n.op <= abi.EXPR_DIVIDE:
                if l != r or l not in NUMERIC:
                    return False
                st.append(l)
            elif abi.EXPR_GT <= n.op <= abi.EXPR_NOTEQ:
                if l != r or l not in NUMERIC + (abi.BOOLEAN,):
                    return False
                st.append(abi.BOOLEAN)
            elif n.op in (abi.EXPR_AND, abi.EXPR_OR):
                if l != abi.BOOLEAN or r != abi.BOOLEAN:
                    return False
                st.append(abi.BOOLEAN)
            else:
                return False
    return st == [abi.BOOLEAN]


def joined_dtypes(lb, rb):
    return [abi.dtype_of(f.type) for f in list(lb.schema) + list(rb.schema)]


def eligible(case, rb, jt, filt, general=True, utf8=False, filter_on=True):
    """the header's rule for one probe batch of a join WITH the filter `filt`: the switch on, the filter compiles, and
    everything the batch would have to meet without the filter (candidates = rows x M bound the output)"""
    if not filter_on or not filter_compiles(filt, joined_dtypes(case.lb, rb)):
        return False
    return eligible_unfiltered(case.lb, rb, case.lkey, case.rkey, jt, max_run(case.lb, case.lkey), general, utf8)


def count_eligible(case, rbs, jt, filt, **kw):
    return sum(1 for b in rbs if eligible(case, b, jt, filt, **kw))


# ---- the filters ------------------------------------------------------------------------------------------------------
# joined schema of the form cases: l.k 0, l.x 1 (f64, NULLs), l.i 2 (int32), l.d 3 (int64, zeros) | r.v 4 (f64, NULLs), r.k 5, r.w 6 (int64)
ARITH_C = 3


def form_filters():
    return {
        "both": InputRef(1) > InputRef(4),                     # l.x > r.v: about half pass, NULL wherever a payload is NULL
        "right_only": InputRef(4) > Constant(0.5, abi.FLOAT64),  # TRUE on (NULL, r) candidates of Right / Full too
        "left_only": InputRef(1) > Constant(0.5, abi.FLOAT64),   # NULL on every (NULL, r) candidate
        "all": InputRef(6).eq(InputRef(6)),
        "none": InputRef(6).ne(InputRef(6)),
        "arith": (TypeCast(InputRef(2), abi.INT64) + InputRef(6)) >= Constant(ARITH_C, abi.INT64),  # int32 + int64 through a cast
        "div0": (InputRef(6) / InputRef(3)).eq(Constant(1, abi.INT64)),  # r.w / l.d = 1
    }


class Case:
    def __init__(self, name, lb, rbs, lkey, rkey, filters, bad=None):
        self.name, self.lb, self.rbs, self.lkey, self.rkey, self.filters, self.bad = name, lb, rbs, lkey, rkey, filters, bad

    def cond(self, filt):
        return JoinCondition([(InputRef(self.lkey), InputRef(self.rkey))], self.filters[filt] if isinstance(filt, str) else filt)

    def __repr__(self):
        return self.name


_cache = {}


def _cached(fn):
    def wrapped(*a):
        key = (fn.__name__,) + a
        if key not in _cache:
            _cache[key] = fn(*a)
        return _cache[key]
    return wrapped


SIZES = [1024] * 4 + [0, 1, 63, 64, 65, 1023, 1025, 2048, 4096, 5000]  # wave, 1024-row tile and slot boundaries; 5000: synchronous


@_cached
def form_case(form):
    """build (k, x, i, d), nb 2000-3000: unique keys or runs of 1-6 rows, dense or x 7919 - 5; probe (v, k, w) in the sizes of
    the issue plus a batch with NULL probe keys.  l.d is 0 on the rows of three reserved keys that no batch of `rbs` probes and
    `bad` probes once (a matched, valid pair): the batch on which `div0` divides by zero.  Other rows of l.d: 1-4, a tenth of
    them NULL with a 0 underneath (a NULL divisor divides nothing)."""
    rng = np.random.default_rng(61 + FORMS.index(form))
    conv = (lambda x: np.asarray(x).astype(np.int64) * 7919 - 5) if form.endswith("sparse") else (lambda x: np.asarray(x).astype(np.int64))
    if form.startswith("unique"):
        key_space = 2500  # (raw probe keys: a fifth of them have no build row)
        raw = rng.permutation(key_space)[:2000]
    else:
        key_space = 940
        raw = np.repeat(rng.permutation(key_space)[:750], rng.integers(1, 7, 750))  # M = 6
        rng.shuffle(raw)
    nb = len(raw)
    zero_keys = raw[:3].copy()
    d = rng.integers(1, 5, nb)
    dnull = rng.random(nb) < 0.1
    d[dnull] = 0
    on_zero = np.isin(raw, zero_keys)
    d[on_zero] = 0
    dnull[on_zero] = False
    x = rng.random(nb)
    lb = pa.RecordBatch.from_arrays([pa.array(conv(raw)), pa.array(x, mask=rng.random(nb) < 0.1), pa.array(rng.integers(-3, 4, nb).astype(np.int32)),
                                     pa.array(d, mask=dnull)], names=["k", "x", "i", "d"])
    allowed = np.setdiff1d(np.arange(key_space), zero_keys)  # (the build side's other keys and those that have no build row)

    def probe(rows, key_nulls=None, keys=None):
        keys = rng.choice(allowed, rows) if keys is None else keys
        return pa.RecordBatch.from_arrays([pa.array(rng.random(rows), mask=rng.random(rows) < 0.2), pa.array(conv(keys), mask=key_nulls),
                                           pa.array(rng.integers(0, 5, rows))], names=["v", "k", "w"])
    rbs = [probe(rows) for rows in SIZES]
    rbs.insert(3, probe(1024, rng.random(1024) < 0.1))  # NULL probe keys: the synchronous operator inside the stream
    bad_keys = rng.choice(allowed, 1024)
    bad_keys[517] = zero_keys[1]
    bad = probe(1024, keys=bad_keys)
    return Case(form, lb, rbs, 0, 1, form_filters(), bad)


def div0_batches(case):
    """two clean batches, the one that divides by zero, two clean ones"""
    return case.rbs[:2] + [case.bad, case.rbs[2], case.rbs[4]], 2


@_cached
def skew_case():
    """one int32 key carried by 16 build rows scattered over the build side; 1024 and 64 probe rows that all hit it: 16384 and
    1024 candidates — SA_MAX_OUT_ROWS, 16 chunks of phase A.  Columns are narrow (24 bytes per joined row) so that the bytes
    admit 16384 rows.  joined schema: l.k 0, l.x 1 | r.k 2, r.v 3"""
    rng = np.random.default_rng(71)
    nb, hot = 2000, 77
    keys = np.arange(nb, dtype=np.int32)
    keys[rng.choice(np.setdiff1d(np.arange(nb), [hot]), 15, replace=False)] = hot
    lb = pa.RecordBatch.from_arrays([pa.array(keys), pa.array(rng.random(nb), mask=rng.random(nb) < 0.1)], names=["k", "x"])
    rbs = [pa.RecordBatch.from_arrays([pa.array(np.full(rows, hot, dtype=np.int32)), pa.array(rng.random(rows), mask=rng.random(rows) < 0.2)], names=["k", "v"])
           for rows in (1024, 64)]
    filters = {"both": InputRef(1) > InputRef(3), "none": InputRef(2).ne(InputRef(2))}
    return Case("skew", lb, rbs, 0, 0, filters)


@_cached
def utf8_case():
    """Utf8 payload columns on both sides next to the float64 ones the filter reads; M = 4.  joined schema: l.k 0, l.s 1, l.x 2 |
    r.t 3, r.k 4, r.v 5.  `utf8_ref` reads the two Utf8 columns: it does not compile"""
    rng = np.random.default_rng(73)
    raw = np.repeat(np.arange(600), 4)
    rng.shuffle(raw)
    nb = len(raw)
    lb = pa.RecordBatch.from_arrays([pa.array(raw.astype(np.int64)), str_array(rand_strings(rng, nb), rng.random(nb) < 0.1),
                                     pa.array(rng.random(nb), mask=rng.random(nb) < 0.1)], names=["k", "s", "x"])
    rbs = [pa.RecordBatch.from_arrays([str_array(rand_strings(rng, rows), rng.random(rows) < 0.2, shift=5), pa.array(rng.integers(0, 750, rows)),
                                       pa.array(rng.random(rows), mask=rng.random(rows) < 0.2)], names=["t", "k", "v"])
           for rows in (1024, 1, 65, 700, 1024, 5000)]
    filters = {"both": InputRef(2) > InputRef(5), "utf8_ref": InputRef(1) >= InputRef(3)}
    return Case("utf8", lb, rbs, 0, 1, filters)
