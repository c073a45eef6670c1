"""Seeded, named cases of row movement and of the operators made of nothing else, for tests/test_move_model_cpu.py (the model
against pyarrow and the CPU oracle, planted faults, what the library claims about itself) and tests/test_gpu_move_edges.py
(every device route).  numpy, pyarrow and the model (tests/move_model.py) only; the last three helpers hand a case to an executor.

A batch carries all five types plus a row id: columns i64, i32, f64, b, s, rid.  A column comes in four NULL modes:
  none     no validity buffer           n10   about 10 % NULLs
  all      every row NULL               allset  a validity buffer with every bit set
Values: the ends of Int64 / Int32; +-0.0, +-inf and NaNs of both signs with payloads; Booleans; Utf8 with empty strings, 2- and
4-byte UTF-8 and one 300-byte string (`utf8="empty"`: every string empty, zero data bytes).

Families (the `family` attribute; `names(family=...)`):
  a  concat    parts of chosen lengths through the cross join's build side (`via="cross"`) or an identity ORDER BY on the row id
               (`via="order"`); forms host | owned | lent | window
  b  slice     LimitExecutor over batches of BATCH_SIZES rows, (offset, limit) pairs; forms host | owned | lent; `gather<n>`: a
               slice of BLOCK_LENGTHS rows out of the 4097-row batch
  c  product   CrossJoinExecutor, L left rows over batches [a, 0, b], right batches [R, 2]; `per_call`: whole | one | mid
  d  project   pass-through columns in permuted order and constants; forms host | owned | lent | window
  e  compact   FilterExecutor over a Boolean mask column (the synchronous route); kept: none | all | half | last | row4096 | first
  f  one group SimpleAggExecutor; shapes one | split | empty | nobatch
  g  text      sqlrs_batch_to_string
  h  arrow     Arrow C Data Interface: slices at ARROW_OFFSETS x ARROW_LENGTHS and four special children

Input forms: host (pyarrow), owned (a library DEVICE batch), lent (a caller-built DEVICE batch over the descriptors of a library
batch, owner NULL), window (as lent, but rows [WINDOW_LEAD, WINDOW_LEAD + m) of a longer batch: pointers advanced, Utf8 offsets
advanced with `values` unchanged, so offsets[0] > 0).  Row counts are the smallest at which each kernel can go wrong: around one
ballot word (64), one block (256), one gather_plain block (2048), one compaction tile (4096); nothing above 8200 rows."""
import functools
import itertools

import numpy as np

import move_model as M
from sqlrs_amd.expr import Constant, InputRef

I64_MIN, I64_MAX, I32_MIN, I32_MAX = -(2 ** 63), 2 ** 63 - 1, -(2 ** 31), 2 ** 31 - 1
POOL_I64 = [I64_MIN, I64_MIN + 1, -1, 0, 1, 2 ** 31, 2 ** 53 + 1, I64_MAX - 1, I64_MAX]
POOL_I32 = [I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX]
F64_BITS = {"+0": 0, "-0": 1 << 63, "+inf": 0x7ff << 52, "-inf": 0xfff << 52, "nan": 0x7ff8 << 48, "-nan": 0xfff8 << 48,
            "nan_payload": 0x7ff0000000000001, "-nan_payload": 0xfff4dead0000beef, "snan_payload": 0x7ff4000000c0ffee,
            "min_sub": 1, "max": 0x7fefffffffffffff, "one": 0x3ff << 52, "-1.5": 0xbff8 << 48}
POOL_F64 = list(F64_BITS.values())
LONG = ("x" * 299 + "y").encode()
POOL_UTF8 = [b"", b"a", "é".encode(), "\U0001f600".encode(), "né\U0001f600x".encode(), b"ab", b" ", b"NULL"]
NULL_MODES = ("none", "n10", "all", "allset")
COLS = ("i64", "i32", "f64", "b", "s", "rid")
DTYPES = (M.I64, M.I32, M.F64, M.BOOL, M.UTF8, M.I64)
ROW_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097]
MAX_ROWS = 8200
WINDOW_LEAD, WINDOW_TAIL = 64, 7
CONCAT_OFFS = (0, 1, 31, 32, 33, 63)
CONCAT_LENS = (0, 1, 63, 64, 65, 129)
BATCH_SIZES = [65, 0, 64, 1, 130, 4097]
# NULL modes of the Limit family's batches; the 4097-row one mixes plain and nullable columns (gather_plain_kernel and gather_kernel)
LIMIT_MODES = ("n10", "all", "all", "allset", "n10", ("none", "n10", "none", "n10", "n10"))
BLOCK_LENGTHS = (255, 256, 257, 2047, 2048, 2049)    # gathers of one 256-thread block / one gather_plain block of 256 x 8 rows
ARROW_OFFSETS = (0, 1, 7, 8, 9, 63, 64, 65)
ARROW_LENGTHS = (0, 1, 64, None)


# ---- the palette --------------------------------------------------------------------------------------------------------------------
def _values(rng, n, utf8="mixed"):
    """n cells per value column, no NULLs yet: pool members at a third of the rows, ordinary values elsewhere"""
    use = rng.random((5, n)) < 0.34
    i64 = [POOL_I64[j] if u else int(v) for j, u, v in zip(rng.integers(0, len(POOL_I64), n), use[0], rng.integers(-10 ** 12, 10 ** 12, n))]
    i32 = [POOL_I32[j] if u else int(v) for j, u, v in zip(rng.integers(0, len(POOL_I32), n), use[1], rng.integers(-10 ** 6, 10 ** 6, n))]
    rnd = (rng.standard_normal(n) * 1000).view(np.uint64)
    f64 = [POOL_F64[j] if u else int(v) for j, u, v in zip(rng.integers(0, len(POOL_F64), n), use[2], rnd)]
    b = [bool(v) for v in rng.integers(0, 2, n)]
    if utf8 == "empty":
        s = [b""] * n
    else:
        s = [POOL_UTF8[j] if u else f"s{int(v)}".encode() for j, u, v in zip(rng.integers(0, len(POOL_UTF8), n), use[4], rng.integers(0, 5000, n))]
        if n > 2:
            s[int(rng.integers(0, n))] = LONG
    return [i64, i32, f64, b, s]


def _null(rng, cells, mode):
    n = len(cells)
    if mode == "all":
        return [None] * n
    if mode == "n10":
        z = rng.random(n) < 0.1
        if n > 1:
            z[1] = True
        return [None if zz else c for c, zz in zip(cells, z)]
    return list(cells)


def palette(seed, n, mode="n10", rid0=0, utf8="mixed"):
    """a model batch of COLS; `mode`: one NULL mode for every value column, or one per column"""
    return [M.Col(c.dtype, c.cells) for c in _palette(seed, n, mode if isinstance(mode, str) else tuple(mode), rid0, utf8)]


@functools.lru_cache(maxsize=None)
def _palette(seed, n, mode, rid0, utf8):
    rng = np.random.default_rng(9000 + seed)
    modes = (mode,) * 5 if isinstance(mode, str) else tuple(mode)
    vals = _values(rng, n, utf8)
    cols = [M.Col(dt, _null(rng, v, m)) for dt, v, m in zip(DTYPES, vals, modes)]
    return cols + [M.Col(M.I64, list(range(rid0, rid0 + n)))]


def arrow_of(batch, mode="n10", names=COLS):
    """the pyarrow form; an `allset` column carries a validity buffer with every bit set"""
    modes = (mode,) * len(batch) if isinstance(mode, str) else tuple(mode) + ("none",) * (len(batch) - len(mode))
    import pyarrow as pa
    arrays = [M.to_arrow(c, "all_set" if m == "allset" else "auto") for c, m in zip(batch, modes)]
    return pa.RecordBatch.from_arrays(arrays, names=list(names)[:len(batch)])


def with_margins(seed, batch):
    """`batch` as rows [WINDOW_LEAD, WINDOW_LEAD + m) of a longer model batch whose first rows hold non-empty strings (so a window's
    Utf8 offsets[0] > 0) and NULLs of their own"""
    lead = palette(seed + 500, WINDOW_LEAD, "n10", rid0=-WINDOW_LEAD)
    lead[4] = M.Col(M.UTF8, [b"before the window"] + lead[4].cells[1:])
    tail = palette(seed + 501, WINDOW_TAIL, "n10", rid0=10 ** 6)
    return M.concat_batches([lead, batch, tail])


# ---- cases --------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, family, name, **attrs):
        self.family, self.name = family, f"{family}-{name}"
        self.__dict__.update(attrs)

    def __repr__(self):
        return self.name


def concat_plan(off):
    """part lengths in which every length of CONCAT_LENS is appended at a bit offset = `off` (mod 64): a lead part of `off` rows, then
    each length followed by the filler that restores the offset"""
    plan = [off] if off else []
    for ln in CONCAT_LENS:
        plan.append(ln)
        if (-ln) % 64:
            plan.append((-ln) % 64)
    return plan


def concat_positions(plan):
    """[(dst_off & 63, length)] of every part"""
    at, out = 0, []
    for ln in plan:
        out.append((at & 63, ln))
        at += ln
    return out


class ConcatCase(Case):
    @functools.cached_property
    def parts(self):
        """the model batches; part k takes NULL mode modes[k % len(modes)]: nullable and non-nullable parts alternate"""
        out, at = [], 0
        for k, ln in enumerate(self.plan):
            out.append(palette(self.seed * 40 + k, ln, self.modes[k % len(self.modes)], rid0=at, utf8=self.utf8))
            at += ln
        return out

    def part_mode(self, k):
        return self.modes[k % len(self.modes)]

    @functools.cached_property
    def expected(self):
        return M.concat_batches(self.parts)


class LimitCase(Case):
    @functools.cached_property
    def batches(self):
        out, at = [], 0
        for k, n in enumerate(BATCH_SIZES):
            out.append(palette(700 + k, n, LIMIT_MODES[k], rid0=at))
            at += n
        return out

    def batch_mode(self, k):
        return LIMIT_MODES[k]

    @functools.cached_property
    def expected(self):
        return M.limit_stream(self.batches, self.limit, self.offset)


LEFT_SPLIT = {0: [0, 0, 0], 1: [1, 0, 0], 3: [1, 0, 2], 65: [64, 0, 1]}


class ProductCase(Case):
    @functools.cached_property
    def left(self):
        out, at = [], 0
        for k, n in enumerate(LEFT_SPLIT[self.L]):
            out.append(palette(800 + self.seed + k, n, "n10", rid0=at))
            at += n
        return out

    @functools.cached_property
    def right(self):
        return [palette(850 + self.seed, self.R, "n10" if self.R != 64 else ("none", "n10", "all", "n10", "n10")), palette(851 + self.seed, 2, "n10")]

    @property
    def max_rows_per_call(self):
        return {"whole": (1 << 31) - 1, "one": 1, "mid": 2 * max(self.R, 1) + 1}[self.per_call]

    @functools.cached_property
    def expected(self):
        return M.cross_join_stream(self.left, self.right)


PROJECT_REFS = [4, 2, 0, 5, 1, 3]


def project_exprs():
    consts = [Constant(-5, M.I32), Constant(I64_MIN, M.I64), Constant(-0.0, M.F64), Constant(float("nan"), M.F64), Constant(True, M.BOOL),
              Constant(False, M.BOOL)]
    nulls = [Constant(None, dt) for dt in (M.I32, M.I64, M.F64, M.BOOL, M.UTF8)]
    return [InputRef(i) for i in PROJECT_REFS] + consts + nulls


class ProjectCase(Case):
    @functools.cached_property
    def batch(self):
        return palette(900 + self.rows, self.rows, self.mode, utf8=self.utf8)

    @property
    def exprs(self):
        return project_exprs()

    @functools.cached_property
    def expected(self):
        return M.project(self.batch, self.exprs)


class CompactCase(Case):
    @functools.cached_property
    def batch(self):
        """columns mask, i64, i32, f64, b, s, rid; the mask has NULLs of its own when it keeps about half"""
        n = self.rows
        rng = np.random.default_rng(4000 + n)
        if self.kept == "none":
            mask = [False] * n
        elif self.kept == "all":
            mask = [True] * n
        elif self.kept == "half":
            mask = [None if z else bool(v) for v, z in zip(rng.integers(0, 2, n), rng.random(n) < 0.1)]
        else:
            row = {"last": n - 1, "row4096": 4096, "first": 0}[self.kept]
            mask = [i == row for i in range(n)]
        return [M.Col(M.BOOL, mask)] + palette(1000 + n, n, "n10")

    @functools.cached_property
    def expected(self):
        return M.keep_batch(self.batch, self.batch[0].cells)


AGG_COLS = ("i64", "i32", "fx", "s", "rid")


def agg_list():
    """[(func, column, distinct)] over AGG_COLS"""
    out = [(f, c, False) for c in (0, 1, 2) for f in ("count", "sum", "min", "max")]
    return out + [("min", 3, False), ("max", 3, False), ("count", 3, False), ("count", 0, True), ("count", 1, True)]


class AggCase(Case):
    @functools.cached_property
    def whole(self):
        """i64, i32, the exact Float64 column fx (integer-valued doubles, |value| <= 2^20: every summation order is exact), s, rid"""
        n = self.rows
        p = palette(1100 + n, n, self.mode)
        rng = np.random.default_rng(1100 + n)
        fx = np.round(rng.integers(-(2 ** 20), 2 ** 20, n).astype(np.float64)).view(np.uint64)
        fxc = M.Col(M.F64, [None if c is None else int(v) for v, c in zip(fx.tolist(), p[2].cells)])
        return [p[0], p[1], fxc, p[4], p[5]]

    @functools.cached_property
    def batches(self):
        n = self.rows
        if self.shape == "nobatch":
            return []
        if self.shape == "split":
            return [M.slice_batch(self.whole, 0, 999), M.slice_batch(self.whole, 999, 0), M.slice_batch(self.whole, 999, n - 999)]
        return [self.whole]

    @functools.cached_property
    def expected(self):
        return M.simple_agg(self.batches, agg_list())


def text_edge_batch():
    f = [5e-324, 1.7976931348623157e308, 1e21, 1e-7, 0.1, -0.0, 2.5e-320, float("nan"), float("inf"), float("-inf"), None, 12000.0, 1100.2]
    bits = [None if v is None else int(np.array([v], dtype=np.float64).view(np.uint64)[0]) for v in f]
    bits[7] = F64_BITS["-nan_payload"]
    n = len(f)
    i64 = [I64_MIN, I64_MAX, None, 0, -1] + list(range(n - 5))
    i32 = [I32_MIN, I32_MAX, 0, None] + list(range(n - 4))
    s = ["é\U0001f600 z".encode(), b"", None, b"a b", LONG] + [f"t{i}".encode() for i in range(n - 5)]
    b = [True, False, None] + [bool(i & 1) for i in range(n - 3)]
    return [M.Col(M.F64, bits), M.Col(M.I64, i64), M.Col(M.UTF8, s), M.Col(M.BOOL, b), M.Col(M.I32, i32)]


class TextCase(Case):
    @functools.cached_property
    def batch(self):
        return text_edge_batch() if self.kind == "edge" else palette(1200, 65, "n10")

    @functools.cached_property
    def expected(self):
        return M.text_form(self.batch)


ARROW_ROWS = 200


class ArrowCase(Case):
    @functools.cached_property
    def base(self):
        if self.kind == "all_empty":
            return palette(1300, ARROW_ROWS, "n10", utf8="empty")
        if self.kind == "validity_no_nulls":
            return palette(1300, ARROW_ROWS, "allset")
        return palette(1300, ARROW_ROWS, "n10")

    @property
    def base_mode(self):
        return "allset" if self.kind == "validity_no_nulls" else "n10"

    @property
    def window(self):
        """(first row, rows) of the base batch that the imported batch describes"""
        ln = ARROW_ROWS - self.offset if self.length is None else self.length
        return self.offset, ln

    @functools.cached_property
    def expected(self):
        return M.slice_batch(self.base, *self.window)


# ---- what both test files drive the operators with ----------------------------------------------------------------------------------
def limit_run(be, batches, limit, offset, out_mem=0):
    """LimitExecutor over `batches` -> (outputs, input batches pulled)"""
    pulled = [0]

    def child():
        for b in batches:
            pulled[0] += 1
            yield b
    from sqlrs_amd.executor import LimitExecutor
    outs = list(LimitExecutor(be, limit, offset, child(), out_mem=out_mem).execute())
    return outs, pulled[0]


def product_schema():
    import pyarrow as pa
    return pa.schema([(f"l.{n}", M.PA_TYPE[t]) for n, t in zip(COLS, DTYPES)] + [(f"r.{n}", M.PA_TYPE[t]) for n, t in zip(COLS, DTYPES)])


def agg_funcs():
    from sqlrs_amd import abi
    from sqlrs_amd.expr import AggFunc
    rt = {"count": lambda dt: abi.INT64, "sum": lambda dt: abi.FLOAT64 if dt == M.F64 else abi.INT64, "min": lambda dt: dt, "max": lambda dt: dt}
    dts = (M.I64, M.I32, M.F64, M.UTF8, M.I64)
    return [AggFunc(f, InputRef(ci), rt[f](dts[ci]), distinct=d) for f, ci, d in agg_list()]


def _cases():
    out = []
    # ---- a. concat ------------------------------------------------------------------------------------------------------------
    rot = [("n10", "none"), ("none", "n10"), ("n10", "none", "allset", "all"), ("all", "none", "n10")]
    plans = [(f"off{o}", concat_plan(o)) for o in CONCAT_OFFS] + [("empties", [0, 65, 0, 1, 129, 0])]
    for k, (pname, plan) in enumerate(plans):
        for form in ("host", "owned", "lent", "window"):
            out.append(ConcatCase("a", f"cross-{pname}-{form}", via="cross", plan=plan, form=form, seed=k, modes=rot[k % 4], utf8="mixed"))
    for k, (pname, plan) in enumerate(plans):
        forms = ("host", "owned", "lent", "window") if pname in ("off33", "empties") else ("host",)
        for form in forms:
            out.append(ConcatCase("a", f"order-{pname}-{form}", via="order", plan=plan, form=form, seed=20 + k, modes=rot[(k + 1) % 4], utf8="mixed"))
    out.append(ConcatCase("a", "cross-all_empty_utf8-window", via="cross", plan=[65, 0, 64, 1], form="window", seed=30, modes=("n10", "all", "none"), utf8="empty"))
    out.append(ConcatCase("a", "cross-all_empty_utf8-host", via="cross", plan=[65, 0, 64, 1], form="host", seed=30, modes=("n10", "all", "none"), utf8="empty"))
    # ---- b. slice -------------------------------------------------------------------------------------------------------------
    pairs = [("nowhere", None, None), ("nowhere_big_limit", None, 10 ** 6), ("inside_first", None, 10), ("on_boundary", None, 65),
             ("from_boundary", 65, None), ("three_batches", 60, 80), ("bit1", 131, 100), ("bit63", 193, 100), ("bit64", 194, 5),
             ("bit65_beyond", 195, 4200), ("beyond", 4000, 1000), ("limit0", 5, 0), ("offset_beyond", 10 ** 6, 5)]
    for pname, off, lim in pairs:
        for form in ("host", "owned", "lent"):
            out.append(LimitCase("b", f"{pname}-{form}", offset=off, limit=lim, form=form))
    for ln in BLOCK_LENGTHS:  # a slice of that many rows out of the 4097-row batch, starting at its bit 3
        out.append(LimitCase("b", f"gather{ln}-host", offset=sum(BATCH_SIZES[:5]) + 3, limit=ln, form="host"))
    # ---- c. product -----------------------------------------------------------------------------------------------------------
    for L, R in itertools.product((0, 1, 3, 65), (0, 1, 63, 64, 65, 257)):
        out.append(ProductCase("c", f"L{L}-R{R}-whole", L=L, R=R, per_call="whole", seed=L * 7 + R))
    for L, R, pc in itertools.product((3, 65), (1, 65), ("one", "mid")):
        out.append(ProductCase("c", f"L{L}-R{R}-{pc}", L=L, R=R, per_call=pc, seed=L * 7 + R))
    # ---- d. pass-through and constants ----------------------------------------------------------------------------------------
    for k, n in enumerate((0, 1, 64, 65, 4097)):
        for form in ("host", "owned", "lent", "window"):
            out.append(ProjectCase("d", f"n{n}-{form}", rows=n, form=form, mode=("n10", "allset", "n10", "none", "n10")[k], utf8="mixed"))
    out.append(ProjectCase("d", "n65-window-all_empty_utf8", rows=65, form="window", mode="n10", utf8="empty"))
    out.append(ProjectCase("d", "n257-window-all_null", rows=257, form="window", mode="all", utf8="mixed"))
    # ---- e. compaction --------------------------------------------------------------------------------------------------------
    for k, n in enumerate((4095, 4096, 4097, 8193)):
        for kept in ("none", "all", "half", "last", "row4096" if n > 4096 else "first"):
            out.append(CompactCase("e", f"n{n}-{kept}", rows=n, kept=kept, form=("host", "owned")[k % 2]))
    # ---- f. one group ---------------------------------------------------------------------------------------------------------
    for shape, mode, n, form in (("one", "n10", 2500, "host"), ("one", "none", 2500, "owned"), ("split", "n10", 2500, "host"),
                                 ("split", "allset", 2500, "owned"), ("one", "all", 2500, "host"), ("split", "all", 2500, "owned"),
                                 ("one", "n10", 65, "lent"), ("empty", "n10", 0, "host"), ("nobatch", "n10", 0, "host")):
        out.append(AggCase("f", f"{shape}-{mode}-n{n}-{form}", shape=shape, mode=mode, rows=n, form=form))
    # ---- g. text form ---------------------------------------------------------------------------------------------------------
    out.append(TextCase("g", "edge", kind="edge"))
    out.append(TextCase("g", "palette", kind="palette"))
    # ---- h. Arrow C Data Interface --------------------------------------------------------------------------------------------
    for off, ln in itertools.product(ARROW_OFFSETS, ARROW_LENGTHS):
        out.append(ArrowCase("h", f"slice-o{off}-l{'end' if ln is None else ln}", kind="slice", offset=off, length=ln))
    out.append(ArrowCase("h", "null_count_unknown", kind="null_count_unknown", offset=9, length=None))
    out.append(ArrowCase("h", "validity_no_nulls", kind="validity_no_nulls", offset=1, length=130))
    out.append(ArrowCase("h", "all_empty_utf8", kind="all_empty", offset=7, length=64))
    out.append(ArrowCase("h", "struct_slice", kind="struct_slice", offset=65, length=70))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = {}
    for c in _cases():
        assert c.name not in cases, c.name
        cases[c.name] = c
    return cases


def case(name) -> Case:
    return all_cases()[name]


def names(**attrs):
    return [c.name for c in all_cases().values() if all(getattr(c, k, None) == v for k, v in attrs.items())]
