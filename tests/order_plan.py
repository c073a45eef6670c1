"""The host-side dispatch of ORDER BY (ops.hip: sqlrs_order_finish, order_topk, order_null_split; order_fast.hip: order_fast,
order_fast_impl, order_wide, order_composite) restated over the DATA of a case: which `order_*` route witnesses one call must
move, and by how much ("Route witnesses of ORDER BY").  numpy only; nothing here is an expectation about values — the
images, the sampled rows and the splitters are restated to predict DECISIONS (key range, key bits, largest group, heavy values,
candidates of a threshold), the way tests/test_gpu_join_edges.py restates the join's.

`plan(case, env)` -> Counter keyed by the witness names without their `order_` prefix."""
import math
from collections import Counter

import numpy as np
import pyarrow as pa

import order_model as M
from sqlrs_amd.expr import InputRef

COUNTERS = ("general", "utf8_key", "narrow", "narrow_hbm_only", "form_lookback", "form_counting", "rec12", "rec16", "wide",
            "wide_declined", "wide_pure_copy", "wide_finish2", "wide_finish3", "heavy_to_wide", "range_sampled", "range_missed",
            "in_order", "composite", "composite_nullable", "composite_too_wide", "null_split", "topk", "topk_ignored", "alloc_declined")
FIN_WG, FIN_CAP = 256, 6144          # order_kernels.hpp
HEAVY_SAMPLES, HEAVY_MIN = 2048, 6
NUM_CUS = 256                        # MI355X (the sampled key range reads one 2048-row chunk per block up to 8 x CUs blocks)
_ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
_U = np.uint64


def read_counters(be) -> dict:
    """every entry of sqlrs_ctx_profile_read as name -> count (launches of a scope, value of a witness)"""
    import ctypes as C
    cap = 512
    names, ms, n_l = (C.c_char_p * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)()
    n = be.fn("ctx_profile_read")(be.ctx, cap, names, ms, n_l)
    assert n <= cap
    return {names[k].decode(): n_l[k] for k in range(n)}


def mix64_np(x: np.ndarray) -> np.ndarray:
    """key_hash.hpp mix64 over uint64 (the jitter of the sampled rows)"""
    x = x.astype(np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> _U(33))
        x = x * _U(0xff51afd7ed558ccd)
        x = x ^ (x >> _U(33))
        x = x * _U(0xc4ceb9fe1a85ec53)
        x = x ^ (x >> _U(33))
    return x


def jittered_rows(n: int, samples: int, stride: int) -> np.ndarray:
    i = np.arange(samples, dtype=np.uint64)
    return np.minimum(_U(n - 1), i * _U(stride) + mix64_np(i) % _U(stride)).astype(np.int64)


def hook_off(env, name):            # `e && e[0] == '0'`
    return env.get(name, "")[:1] == "0"


def hook_int_zero(env, name):       # `e && atoi(e) == 0`
    return name in env and int(env[name] or 0) == 0


class Plan:
    def __init__(self, env):
        self.env, self.c = dict(env), Counter()

    # ---- sqlrs_order_finish --------------------------------------------------------------------------------------------------
    def finish(self, table: pa.Table, order_by, hint: int = 0):
        env, c, n = self.env, self.c, table.num_rows
        refs = [isinstance(ob.expr, InputRef) for ob in order_by]
        tk = int(env["SQLRS_ORDER_TOPK"]) if "SQLRS_ORDER_TOPK" in env else -1
        if hint > 0 and tk != 0 and refs and refs[0] and ((n >= 1 << 17) if tk == 1 else (n >= 1 << 20 and hint <= n // 16)):
            arr = M._one(table.column(order_by[0].expr.index))
            if arr.type in (pa.int64(), pa.float64(), pa.int32()) and arr.null_count == 0:
                img = M.image(arr) ^ (_U(0) if order_by[0].asc else _ALL)
                S = 65536
                rows = np.minimum(np.arange(S, dtype=np.int64) * (n // S), n - 1)
                q = min(S - 1, math.ceil(hint * S / n * 2.0) + 64)
                keep = img <= np.sort(img[rows])[q]
                if int(keep.sum()) >= hint:
                    self.finish(table.filter(pa.array(keep)).combine_chunks(), order_by)
                    c["topk"] += 1
                    return
                c["topk_ignored"] += 1
        fast_on = not hook_off(env, "SQLRS_ORDER_FAST")
        ncols = table.num_columns

        def carry_of(keys):
            for ci in range(ncols):
                col = M._one(table.column(ci))
                if ci not in keys and col.type in (pa.int64(), pa.float64()) and col.null_count == 0:
                    return ci
            return -1

        if fast_on and len(order_by) == 1 and refs[0]:
            kc = order_by[0].expr.index
            arr = M._one(table.column(kc))
            cc = carry_of([kc])
            want_perm = ncols > (2 if cc >= 0 else 1)
            if arr.type in (pa.int64(), pa.float64(), pa.int32()) and arr.null_count == 0:
                img = M.image(arr) ^ (_U(0) if order_by[0].asc else _ALL)
                r = self.order_fast(img, arr.type == pa.int32(), n, cc >= 0, want_perm)
                if r:
                    return
        if fast_on and 1 <= len(order_by) <= 4 and n >= 1 << 20 and all(refs):
            kcs = [ob.expr.index for ob in order_by]
            others = ncols - len(set(kcs))
            cc = carry_of(kcs)
            if self.composite(table, order_by, cc >= 0, others > (1 if cc >= 0 else 0)):
                return
        if fast_on and len(order_by) == 1 and refs[0] and n >= 1 << 21:
            arr = M._one(table.column(order_by[0].expr.index))
            if arr.type in (pa.int64(), pa.float64(), pa.int32()) and arr.null_count and n - arr.null_count >= 1 << 20:
                kc = order_by[0].expr.index
                inner = table.filter(arr.is_valid()).combine_chunks()
                key = M._one(inner.column(kc))
                inner = inner.set_column(kc, inner.schema.names[kc], pa.Array.from_buffers(key.type, len(key), [None, key.buffers()[1]], offset=key.offset))
                self.finish(inner, order_by)
                c["null_split"] += 1
                return
        c["general"] += 1
        if n > 1:
            c["utf8_key"] += sum(1 for a in M.key_arrays(table.slice(0, 0), order_by) if a.type == pa.string())

    # ---- order_fast / order_fast_impl ------------------------------------------------------------------------------------------
    def order_fast(self, img, is_i32, n, carry, want_perm):
        """img: the key's image with the direction applied; -> True (produced), 'in_order', False"""
        if n < 1 << 20:
            return False
        env, c = self.env, self.c
        optimistic = (int(env["SQLRS_ORDER_SAMPLE"]) != 0) if "SQLRS_ORDER_SAMPLE" in env else n >= 1 << 24
        c["range_sampled"] += optimistic
        args = (img, is_i32, n, carry, want_perm)
        ok, retry, hbm = self.impl(*args, optimistic, True, False)
        if ok or not (retry or hbm):
            return ok
        if retry:
            c["range_missed"] += 1
            ok, retry, hbm = self.impl(*args, False, False, False)
            if ok or not hbm:
                return ok
        return self.impl(*args, False, False, True)[0]

    def impl(self, img, is_i32, n, carry, want_perm, optimistic, in_order_ok, hbm_only, lb_skip=False):
        env, c = self.env, self.c
        heavy_probe = not hbm_only and not hook_off(env, "SQLRS_ORDER_HEAVY_PROBE")
        if in_order_ok and bool((img[:-1] <= img[1:]).all()):
            c["in_order"] += 1
            return "in_order", False, False
        if optimistic:   # every 16th chunk of 2048 rows, one per block, and the last 2048 rows
            blocks = max(1, min(-(-n // (2048 * 16)), 8 * NUM_CUS))
            assert blocks * 16 * 2048 >= n
            rows = (np.arange(blocks, dtype=np.int64)[:, None] * (16 * 2048) + np.arange(2048, dtype=np.int64)[None, :]).ravel()
            rows = np.concatenate([np.minimum(rows, n - 1), np.arange(max(0, n - 2048), n)])
            imin, imax = int(img[rows].min()), int(img[rows].max())
        else:
            imin, imax = int(img.min()), int(img.max())
        rng_ = imax - imin
        if rng_ > 0xFFFFFFFF:
            if is_i32:
                return False, False, False
            return self.wide(img, n, carry, want_perm, 0 if optimistic else imin), False, False
        kbits = 1
        while kbits < 32 and (1 << kbits) <= rng_:
            kbits += 1
        oob = False
        if optimistic:
            win = 1 << kbits
            base = imin & ~(win - 1)
            if imax - base < win:
                imin = base
            elif kbits < 32:
                kbits += 1
                imin -= min((((1 << kbits) - 1) - rng_) // 2, imin)
            else:
                return False, True, False
            off = img - _U(imin)     # (wraps for a key below the window: far outside)
            oob = bool((off >> _U(kbits)).any())
        want = 1
        while want < 16 and (n >> want) > 2048:
            want += 1
        top = kbits if hbm_only else min(kbits, want)
        rbits = kbits - top
        if heavy_probe and rbits > 0:
            stride = max(n // HEAVY_SAMPLES, 1)
            cnt = int(np.unique(img[jittered_rows(n, HEAVY_SAMPLES, stride)], return_counts=True)[1].max())
            if cnt >= HEAVY_MIN:
                c["heavy_to_wide"] += 1
                if self.wide(img, n, carry, want_perm, 0 if optimistic else imin):
                    return True, False, False
        tiled_on, rec_on = not hook_int_zero(env, "SQLRS_ORDER_TILED"), not hook_int_zero(env, "SQLRS_ORDER_REC")
        two_pass_shape = rbits > 0 and 8 < top <= 16
        rec1 = carry and two_pass_shape and tiled_on and rec_on and not hook_off(env, "SQLRS_ORDER_REC1")
        use_tiled = rbits > 0 and tiled_on
        use_rec = use_tiled and carry and rec_on
        lb = two_pass_shape and use_tiled and ((rec1 and use_rec) if carry else True) and not lb_skip and not hook_off(env, "SQLRS_ORDER_LB")
        c["form_lookback" if lb else "form_counting"] += 1
        c["narrow_hbm_only"] += hbm_only
        if lb:
            slim = carry and not want_perm and not hook_off(env, "SQLRS_ORDER_SLIM")
            c["rec12"] += slim
            c["rec16"] += carry and not slim
        else:
            c["rec16"] += bool(rec1 or (use_rec and top > 8))
        if rbits == 0:
            if oob:
                return False, True, False
            c["narrow"] += 1
            return True, False, False
        if lb and env.get("SQLRS_ORDER_LB_TEST_FAIL", "")[:1] in ("1", "2"):   # the attempt is treated as failed: once more, counting
            return self.impl(img, is_i32, n, carry, want_perm, optimistic, False, hbm_only, True)
        if oob:
            return False, True, False
        off = img - _U(imin)
        if int(np.bincount((off >> _U(rbits)).astype(np.int64), minlength=1).max()) > FIN_CAP:
            return False, False, True
        c["narrow"] += 1
        return True, False, False

    # ---- order_wide ------------------------------------------------------------------------------------------------------------
    def wide(self, img, n, carry, want_perm, imin, lb_skip=False):
        env, c = self.env, self.c
        if hook_off(env, "SQLRS_ORDER_WIDE"):
            return False
        top = 9
        while top < 16 and (n >> top) > 2048:
            top += 1
        G = 1 << top
        per_group = max(1, min(256, int(env["SQLRS_ORDER_SAMPLES"]))) if "SQLRS_ORDER_SAMPLES" in env else 16
        S = G * per_group
        if n < S:
            c["wide_declined"] += 1
            return False
        has_pay = bool(want_perm or carry)
        rec1 = has_pay and not hook_off(env, "SQLRS_ORDER_WIDE_REC1")
        lb1 = rec1 and not lb_skip and not hook_off(env, "SQLRS_ORDER_LB")
        c["form_lookback" if lb1 else "form_counting"] += 1
        c["rec16"] += has_pay
        if lb1 and env.get("SQLRS_ORDER_LB_TEST_FAIL", "")[:1] == "1":
            return self.wide(img, n, carry, want_perm, imin, True)
        off = img - _U(imin)
        sub = np.sort(off[jittered_rows(n, S, n // S)])[np.arange(G) * per_group]
        sub[0] = 0
        last = np.searchsorted(sub, off, side="right") - 1          # the last splitter <= off ...
        g = np.where(sub[last] == off, np.searchsorted(sub, off, side="left"), last)   # ... a row equal to one: the first group of its run
        sizes = np.bincount(g, minlength=G)
        pure = np.zeros(G, dtype=bool)
        pure[:-1] = (sub[:-1] == sub[1:]) & (sizes[:-1] > 0)
        max_group = int(sizes[~pure].max())
        if max_group > FIN_CAP:
            c["wide_declined"] += 1
            return False
        c["wide"] += 1
        c["wide_pure_copy"] += bool(pure.any())
        c["wide_finish2"] += max_group > 8 * FIN_WG
        c["wide_finish3"] += max_group > 16 * FIN_WG
        return True

    # ---- order_composite -------------------------------------------------------------------------------------------------------
    def composite(self, table, order_by, carry, want_perm):
        env, c, n = self.env, self.c, table.num_rows
        if hook_off(env, "SQLRS_ORDER_COMPOSITE"):
            return False
        cols = [M._one(table.column(ob.expr.index)) for ob in order_by]
        if any(a.type not in (pa.int64(), pa.int32()) for a in cols):
            return False
        nullable = [a.null_count != 0 for a in cols]
        if len(cols) == 1 and not nullable[0]:
            return False
        imgs, bits, lo, hi = [], [], [], []
        for a in cols:   # over every slot: what sits under a NULL widens the range
            raw = M._raw(a, np.int64 if a.type == pa.int64() else np.int32).astype(np.int64).view(np.uint64) ^ _U(1 << 63)
            imgs.append(raw)
            lo.append(int(raw.min()))
            hi.append(int(raw.max()))
            bits.append((hi[-1] - lo[-1]).bit_length())
        if sum(bits) + sum(nullable) > 64:
            c["composite_too_wide"] += 1
            return False
        comp = np.zeros(n, dtype=np.uint64)
        for a, ob, img, b, l, h, nl in zip(cols, order_by, imgs, bits, lo, hi, nullable):
            fb = b + nl
            if fb == 0:
                continue
            field = (img - _U(l)) if ob.asc else (_U(h) - img)
            if nl:
                field = np.where(M._valid(a), field | _U(1 << b), _U(0))
            comp = ((comp << _U(fb)) if fb < 64 else _U(0)) | field
        r = self.order_fast(comp, False, n, carry, want_perm)
        if r == "in_order":
            return True
        if r:
            c["composite"] += 1
            c["composite_nullable"] += any(nullable)
        return bool(r)


def plan(case, env=None, hinted=True) -> Counter:
    p = Plan({**case.env, **(env or {})})
    hint = (case.offset + case.limit) if (case.limit is not None and hinted) else 0
    p.finish(case.table(), case.order_by, hint)
    return Counter({k: int(v) for k, v in p.c.items() if v})


def intended(case, c: Counter):
    """does the plan put the case on the route (and through the decisions) it is named for?  -> list of complaints"""
    bad = []
    lead = {"general": "general", "narrow": "narrow", "wide": "wide", "in_order": "in_order", "composite": "composite",
            "null_split": "null_split", "topk": "topk"}[case.route]
    if c[lead] != 1:
        bad.append(f"{lead} moves by {c[lead]}")
    if case.route in ("general", "narrow", "wide", "in_order"):
        for other in ("composite", "null_split", "topk") + tuple(r for r in ("general", "narrow", "wide", "in_order") if r != lead):
            if c[other]:
                bad.append(f"{other} moves too")
    if c["general"] + c["narrow"] + c["wide"] + c["in_order"] != 1:
        bad.append("not exactly one of general / narrow / wide / in_order")
    p = case.props
    for prop, name, want in (("hbm_only", "narrow_hbm_only", 1), ("heavy_to_wide", "heavy_to_wide", 1), ("declined", "wide_declined", 1),
                             ("ignored", "topk_ignored", 1), ("sampled", "range_sampled", 1), ("nullable", "composite_nullable", 1)):
        if p.get(prop) and c[name] != want:
            bad.append(f"{name} moves by {c[name]}")
    if "missed" in p and c["range_missed"] != int(p["missed"]):
        bad.append(f"range_missed moves by {c['range_missed']}")
    if p.get("field_bits", 0) > 64 and c["composite_too_wide"] != 1:
        bad.append("composite_too_wide at rest")
    if "heavy" in p and not c["wide_pure_copy"]:
        bad.append("wide_pure_copy at rest")
    return bad
