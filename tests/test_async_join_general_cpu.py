"""sqlrs_hash_join_set_async_general off the GPU: a backend without the entry point (the oracle) runs a HashJoinExecutor
with ``async_general=True`` unchanged, and abi.py declares the function as the header does."""
import inspect
import os
import re

import numpy as np
import pyarrow as pa

from sqlrs_amd import abi
from sqlrs_amd.executor import HashJoinExecutor
from sqlrs_amd.expr import InputRef, JoinCondition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_runs_unchanged_with_the_flag(oracle):
    assert getattr(oracle.lib, oracle.prefix + "hash_join_set_async_general", None) is None
    rng = np.random.default_rng(1)
    lb = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 40, 100)), pa.array(rng.random(100), mask=rng.random(100) < 0.1)], names=["k", "x"])
    rbs = [pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 60, n)), pa.array(rng.random(n))], names=["k", "v"]) for n in (64, 0, 100)]
    sch = pa.schema([pa.field(f"l.{f.name}", f.type) for f in lb.schema] + [pa.field(f"r.{f.name}", f.type) for f in rbs[0].schema])
    cond = JoinCondition([(InputRef(0), InputRef(0))])
    for jt in ("inner", "left", "right", "full"):
        exp = list(HashJoinExecutor(oracle, [lb], rbs, jt, cond, sch, 2).execute())
        for depth in (0, 3):
            got = list(HashJoinExecutor(oracle, [lb], rbs, jt, cond, sch, 2, depth=depth, async_general=True).execute())
            assert len(got) == len(exp) and all(g.equals(e) for g, e in zip(got, exp))


def test_abi_declares_the_setter_with_the_headers_arity():
    header = open(os.path.join(ROOT, "include", "sqlrs_hip.h")).read()
    m = re.search(r"\bint\s+sqlrs_hash_join_set_async_general\s*\(([^)]*)\)\s*;", header)
    assert m, "the header declares sqlrs_hash_join_set_async_general"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 2 and params[0].startswith("sqlrs_hash_join_t *") and params[1].startswith("int ")
    d = re.search(r'"hash_join_set_async_general":\s*\((\w+),\s*\[([^\]]*)\]\)', inspect.getsource(abi.Backend._declare))
    assert d, "abi.py declares hash_join_set_async_general"
    assert d.group(1) == "i" and [a.strip() for a in d.group(2).split(",")] == ["vp", "C.c_int"]
