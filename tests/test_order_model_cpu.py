"""The ORDER BY model (order_model.py) and its cases (order_edge_cases.py) checked without a GPU:

* the fast form of the model (numpy.lexsort over images) against its row-by-row restatement (a comparator over values, no
  image) on the first rows of every case and on a few thousand random small inputs drawn from the pools;
* the model against the CPU oracle on every case at full size, bit for bit (order.rs:27-66 decides where the two would differ:
  arrow's lexsort orders doubles by total order and puts NULLs first under either direction — they do not differ, see
  test_model_agrees_with_the_oracle);
* the conditions every case is named for, in exact Python integers, computed from the case alone;
* planted faults: applied to the EXPECTED output of the model, never to a library, and `compare` must reject each."""
import numpy as np
import pyarrow as pa
import pytest

import order_edge_cases as E
import order_model as M
from sqlrs_amd.expr import InputRef, OrderBy

CASES = E.all_cases()
# (named here, not filtered by building every case at collection time; test_the_other_named_properties_hold checks the lists)
RANGE_CASES = [n for n in CASES if n.startswith(("i64_range_", "i64_kbits_", "i32_min_max_"))]
FIELD_BITS_CASES = ["comp_fields_64_bits", "comp_fields_65_bits", "comp_nullable_63_value_bits_desc", "comp_nullable_64_value_bits",
                    "comp_full_range_key_and_a_constant"]
GENERAL_BY_DECISION = ["i64_wide_declined_sample_blind", "comp_fields_65_bits", "comp_garbage_under_nulls_widens_the_range",
                       "nsplit_one_valid_row_short", "topk_hint_ignored_sample_not_representative"]


def key_values(c, k=0):
    """the valid values of key column k as Python ints (doubles: bit patterns) / bytes"""
    return [v for v in M.X.column_values(M.key_arrays(c.table(), c.order_by)[k]) if v is not None]


def key_values_np(c, k=0) -> np.ndarray:
    """... of a fixed-width InputRef key as a numpy array (doubles: uint64 bit patterns)"""
    arr = M.key_arrays(c.table(), c.order_by)[k]
    dt = {pa.float64(): np.uint64, pa.int64(): np.int64, pa.int32(): np.int32}[arr.type]
    raw = np.frombuffer(arr.buffers()[1], dtype=dt, count=arr.offset + len(arr))[arr.offset:]
    return raw[np.asarray(arr.is_valid()).astype(bool)] if arr.null_count else raw


# ---- fast form = row-by-row restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fast_model_agrees_with_the_restatement(name):
    c = E.case(name).reduced(400)
    assert M.perm_fast(c.batches, c.order_by).tolist() == M.perm_slow(c.batches, c.order_by), name


def test_fast_model_agrees_with_the_restatement_on_random_small_inputs():
    rng = np.random.default_rng(E.seed_of("random small inputs"))
    pools = {
        "f64": lambda n: pa.array(E.f64_of(rng.choice(np.array(E.POOL_F64, dtype=np.uint64), n)), from_pandas=False),
        "i64": lambda n: pa.array(rng.choice(np.array(E.POOL_I64, dtype=np.int64), n)),
        "i32": lambda n: pa.array(rng.choice(np.array(E.POOL_I32 + [-1, 0, 1], dtype=np.int32), n)),
        "bool": lambda n: pa.array(rng.random(n) < 0.5),
        "utf8": lambda n: E.utf8_by_take(rng, n, nulls=0),
    }
    kinds = list(pools)
    for _ in range(4000):
        n = int(rng.integers(0, 13))
        nk = int(rng.integers(1, 4))
        cols, ob = [], []
        for k in range(nk):
            arr = pools[kinds[int(rng.integers(0, len(kinds)))]](n)
            if rng.random() < 0.5 and n:
                arr = pa.array(arr.to_pylist(), type=arr.type, mask=rng.random(n) < 0.3) if arr.type != pa.float64() else \
                    E.with_validity(np.frombuffer(arr.buffers()[1], dtype=np.float64, count=n).copy(), rng.random(n) >= 0.3)
            cols.append(arr)
            ob.append(OrderBy(InputRef(k), asc=bool(rng.random() < 0.5)))
        b = pa.RecordBatch.from_arrays(cols, names=[f"k{k}" for k in range(nk)])
        assert M.perm_fast([b], ob).tolist() == M.perm_slow([b], ob), (b.to_pydict(), ob)


def test_the_restatement_orders_the_pools_as_defined():
    """the comparator itself, on orders known from the definition and written out here"""
    f = E.f64_of([0x7FF8000000000000, 0x0, 0xFFFFFFFFFFFFFFFF, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x1,
                  0x7FF8000000000123, 0xFFF8000000000001, 0x7FFFFFFFFFFFFFFF])
    b = pa.RecordBatch.from_arrays([pa.array(f, from_pandas=False)], names=["k"])
    #       -NaN(all ones) < -NaN(payload 1) < -inf < -0.0 < +0.0 < subnormal < +inf < NaN < NaN(0x123) < NaN(all ones)
    assert M.perm_slow([b], [OrderBy(InputRef(0), True)]) == [2, 8, 5, 3, 1, 6, 4, 0, 7, 9]
    s = pa.RecordBatch.from_arrays([pa.array(["a\x00", None, "a", "", "é", "z", "a\x00\x00", "abcdefgh", "abcdefg", "abcdefghi"])], names=["k"])
    assert M.perm_slow([s], [OrderBy(InputRef(0), True)]) == [1, 3, 2, 0, 6, 8, 7, 9, 5, 4]     # NULL, "", prefixes first, bytes >= 0x80 last
    assert M.perm_slow([s], [OrderBy(InputRef(0), False)]) == [1, 4, 5, 9, 7, 8, 6, 0, 2, 3]    # NULL still first
    t = pa.RecordBatch.from_arrays([pa.array([True, None, False, True, None])], names=["k"])
    assert M.perm_slow([t], [OrderBy(InputRef(0), False)]) == [1, 4, 0, 3, 2]


# ---- model = oracle --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_model_agrees_with_the_oracle(oracle, name):
    c = E.case(name)
    M.compare(E.run(oracle, c), M.expected(c.batches, c.order_by, c.limit, c.offset), name)


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------
def test_every_route_has_cases_at_the_sizes_of_the_issue():
    for r in E.ROUTES:
        assert E.cases_of(r), r
    sizes = {r: {E.case(n).rows for n in E.cases_of(r)} for r in E.ROUTES}
    assert set(E.GENERAL_SIZES) | {70_001} <= sizes["general"]
    for r in ("narrow", "wide", "composite"):      # the smallest counts the fast routes take, one that is no multiple of 64 / the tile
        assert {E.N20, E.N20 + 1, E.NODD} <= sizes[r], (r, sizes[r])
    assert E.N21P in sizes["wide"] and E.N21P % 64 and E.N21P > 1 << 21
    assert E.N21 in sizes["null_split"] and E.NTOPK in sizes["topk"] and E.NTOPK == 1 << 17
    assert E.N20 - 1 in sizes["general"] and E.NTOPK - 1 in sizes["general"]   # one row short of the fast routes / of the forced top-k
    forms = {len(E.case(n).batches) for n in CASES}
    assert forms == {1, 3} and all(E.case(n).batches[1].num_rows == 0 for n in CASES if len(E.case(n).batches) == 3)
    for n in CASES:
        assert E.case(n).rows <= 1 << 22
        if any(M.key_kind(a.type) == "utf8" for a in M.key_arrays(E.case(n).table().slice(0, 0), E.case(n).order_by)):
            assert E.case(n).rows <= 1 << 17, n        # Utf8 keys run on the general path


def test_every_pool_value_occurs_on_every_route_that_admits_its_type():
    """f64: the narrow route (<= 32 varying bits: the pool piecewise), the splitter route, the NULL split, the general path and the
    in-order return; int64: those and the composite (64 + 0 bits); int32: narrow, composite, general (an int32 key is never wide
    by range).  Top-k keys have their own list of thresholds (test_every_topk_case_...)."""
    seen = {}
    for n in CASES:
        c = E.case(n)
        for k, arr in enumerate(M.key_arrays(c.table().slice(0, 0), c.order_by)):
            kind = M.key_kind(arr.type)
            if kind in ("f64", "i64", "i32") and isinstance(c.order_by[k].expr, InputRef):
                pool = np.array({"f64": E.POOL_F64, "i64": E.POOL_I64, "i32": E.POOL_I32}[kind], dtype=np.uint64 if kind == "f64" else np.int64)
                seen.setdefault((c.route, kind), set()).update(pool[np.isin(pool, key_values_np(c, k))].tolist())
    for route in ("narrow", "wide", "null_split", "general", "in_order"):
        assert set(E.POOL_F64) <= seen[(route, "f64")], (route, [hex(v) for v in set(E.POOL_F64) - seen[(route, "f64")]])
    for route in ("narrow", "wide", "null_split", "general", "composite"):
        assert set(E.POOL_I64) <= seen[(route, "i64")], (route, set(E.POOL_I64) - seen[(route, "i64")])
    for route in ("narrow", "composite", "general"):
        assert set(E.POOL_I32) <= seen[(route, "i32")], route
    utf8 = set()
    for n in E.cases_of("general"):
        c = E.case(n)
        for k, arr in enumerate(M.key_arrays(c.table().slice(0, 0), c.order_by)):
            if arr.type == pa.string():
                utf8.update(key_values(c, k))
    assert {s.encode() for s in E.POOL_UTF8} <= utf8
    lengths = {len(s.encode()) for s in E.POOL_UTF8}
    assert set(range(18)) | {24} <= lengths


@pytest.mark.parametrize("name", RANGE_CASES)
def test_boundary_cases_have_the_range_they_are_named_for(name):
    c = E.case(name)
    v = key_values_np(c)
    assert int(v.max()) - int(v.min()) == c.props["range"], (name, int(v.max()) - int(v.min()))
    assert (c.route == "wide") == (c.props["range"] > 0xFFFFFFFF)


def field_bits(c):
    total = 0
    for arr in M.key_arrays(c.table(), c.order_by):
        raw = np.frombuffer(arr.buffers()[1], dtype=np.int64 if arr.type == pa.int64() else np.int32, count=len(arr))  # (every slot: NULL ones too)
        span = int(raw.max()) - int(raw.min())
        total += span.bit_length() + (1 if arr.null_count else 0)
    return total


@pytest.mark.parametrize("name", FIELD_BITS_CASES)
def test_composite_cases_have_the_field_widths_they_are_named_for(name):
    c = E.case(name)
    assert field_bits(c) == c.props["field_bits"], (name, field_bits(c))
    assert (c.route == "composite") == (c.props["field_bits"] <= 64)


def test_the_other_named_properties_hold():
    c = E.case("comp_constant_key_among_others")
    assert len(set(key_values(c, c.props["constant_key"]))) == 1
    c = E.case("comp_garbage_under_nulls_widens_the_range")
    arr = M.key_arrays(c.table(), c.order_by)[0]
    raw = np.frombuffer(arr.buffers()[1], dtype=np.int64, count=len(arr))
    assert int(raw.min()) == E.I64_MIN and int(raw.max()) == E.I64_MAX and key_values_np(c).min() >= 0 and key_values_np(c).max() < 1000
    assert field_bits(c) > 64
    for name in ("nsplit_exactly_2p21_rows_2p20_valid", "nsplit_one_valid_row_short"):
        c = E.case(name)
        assert c.rows == 1 << 21 and len(key_values_np(c)) == c.props["valid_rows"] and field_bits(c) == 65
        assert (c.route == "null_split") == (c.props["valid_rows"] >= 1 << 20)
    c = E.case("nsplit_f64_desc_validity_flips_every_64_rows")
    arr = M.key_arrays(c.table(), c.order_by)[0]
    valid = np.asarray(arr.is_valid())
    assert all(valid[i] != valid[i + 64] for i in range(0, 4096)) and len(set(valid[:64].tolist())) == 1
    vb = np.frombuffer(arr.buffers()[0], dtype=np.uint8)
    assert c.rows % 64 and len(vb) * 8 > c.rows and np.unpackbits(vb, bitorder="little")[c.rows:].all()   # padding bits set
    assert len(key_values_np(c)) >= 1 << 20
    named = {"range": [], "field_bits": [], "decision": []}
    for name in CASES:
        c = E.case(name)
        named["range"] += [name] if "range" in c.props else []
        named["field_bits"] += [name] if "field_bits" in c.props else []
        named["decision"] += [name] if c.route == "general" and c.props.keys() & {"declined", "ignored", "field_bits", "garbage", "valid_rows"} else []
        if "heavy" in c.props:
            assert int((key_values_np(c) == np.uint64(c.props["heavy"])).sum()) >= 0.25 * c.rows, name
        if "cluster12" in c.props:
            v = key_values_np(c)
            assert int(((v >> np.uint64(12)) == np.uint64(E.ONE >> 12)).sum()) >= 5000, name
        if "outlier_rows" in c.props:   # chunks of 2048 rows, every 16th is read, and the last 2048 rows
            for r in c.props["outlier_rows"]:
                assert (r // 2048) % 16 != 0 and r < c.rows - 2048, (name, r)
            assert c.env.get("SQLRS_ORDER_SAMPLE") == "1"
    assert named["range"] == RANGE_CASES and sorted(named["field_bits"]) == sorted(FIELD_BITS_CASES)
    assert sorted(named["decision"]) == sorted(GENERAL_BY_DECISION)


@pytest.mark.parametrize("name", E.cases_of("topk"))
def test_every_topk_case_has_its_limit_on_the_candidate_side_of_its_threshold(name):
    c = E.case(name)
    kind, t = c.props["threshold"]
    arr = M.key_arrays(c.table(), c.order_by)[0]
    img = M.image(arr)
    probe = pa.array(E.f64_of([t]), from_pandas=False) if kind == "f64" else pa.array([t], type=arr.type)
    timg = int(M.image(probe)[0])
    side = int((img <= np.uint64(timg)).sum()) if c.order_by[0].asc else int((img >= np.uint64(timg)).sum())
    assert c.offset + c.limit <= side < c.rows // 2, (name, side)
    assert (c.env == {"SQLRS_ORDER_TOPK": "1"} and c.rows >= 1 << 17) or (c.env == {} and c.rows >= 1 << 20 and c.offset + c.limit <= c.rows // 16)


# ---- planted faults ----------------------------------------------------------------------------------------------------------------
def test_compare_rejects_planted_faults():
    c = E.case("gen_f64_pool_nullable_desc_4096")     # (its columns: the key and a row id)
    exp = M.expected(c.batches, c.order_by)
    M.compare(exp, exp, "identity")
    key = exp.column(0).chunk(0)
    bits = np.frombuffer(key.buffers()[1], dtype=np.uint64, count=len(key)).copy()
    valid = np.asarray(key.is_valid())

    def with_key(b, v=valid):
        return exp.set_column(0, "k0", E.with_validity(E.f64_of(b), v))

    i = int(np.nonzero(valid & (bits == 0x8000000000000000))[0][0])      # -0.0 taken for +0.0
    b2 = bits.copy(); b2[i] = 0
    with pytest.raises(AssertionError):
        M.compare(with_key(b2), exp, "-0.0 as +0.0")
    i = int(np.nonzero(valid & (bits == 0x7FF8000000000123))[0][0])      # a NaN that lost its payload
    b2 = bits.copy(); b2[i] = 0x7FF8000000000000
    with pytest.raises(AssertionError):
        M.compare(with_key(b2), exp, "NaN payload")
    v2 = valid.copy(); v2[int(np.nonzero(~valid)[0][0])] = True           # a NULL that became valid
    with pytest.raises(AssertionError):
        M.compare(with_key(bits, v2), exp, "validity")
    b2 = bits.copy(); b2[~valid] ^= np.uint64(0xFFFF)                      # what sits under a NULL is not looked at
    M.compare(with_key(b2), exp, "under NULL")
    p = M.perm_fast(c.batches, c.order_by)                                 # two tied rows swapped: only the row ids show it
    t = c.table()
    kk = np.frombuffer(t.column(0).chunk(0).buffers()[1], dtype=np.uint64, count=t.num_rows)
    j = next(j for j in range(len(p) - 1) if valid[j] and valid[j + 1] and kk[p[j]] == kk[p[j + 1]])
    p2 = p.copy(); p2[j], p2[j + 1] = p[j + 1], p[j]
    with pytest.raises(AssertionError):
        M.compare(M.take(t, p2), exp, "tie order")
    c = E.case("gen_utf8_every_pool_string_once")
    exp = M.expected(c.batches, c.order_by)
    vals = exp.column(0).to_pylist()
    b = vals.index("a\x00")
    a = b - 1
    assert vals[a] == "a"
    vals[a], vals[b] = vals[b], vals[a]
    with pytest.raises(AssertionError):
        M.compare(exp.set_column(0, "k0", pa.array(vals, type=pa.string())), exp, "zero padding")


# ---- the route every case is made for ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.cases_of("narrow", "wide", "in_order", "composite", "null_split", "topk") + GENERAL_BY_DECISION)
def test_the_restated_dispatch_puts_every_case_on_its_route(name):
    """order_plan.py restates the host-side dispatch over the case's data; the GPU file asserts the library's witnesses against
    it — here, that the plan itself says what the case is named for (a case that drifted off its route fails without a GPU)"""
    import order_plan as P
    c = E.case(name)
    got = P.plan(c)
    assert not P.intended(c, got), (name, P.intended(c, got), dict(got))
    off = P.plan(c, {"SQLRS_ORDER_FAST": "0"})
    assert off["general"] == 1 and not (set(off) - {"general", "utf8_key", "topk", "topk_ignored"}), (name, dict(off))
