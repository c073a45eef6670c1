"""Cases and the numpy model of the ordering of pre-aggregated groups stored as 32-byte rows (hashagg_op.hip
emit_pending_group_rows, sort.hip radix_sort_gather_rows_u32), shared by test_group_order_packed_cpu.py and
test_gpu_group_order_packed.py.

THE RULE (`ordered_rows`): the groups of one batch leave in the order of their first rows — a stable argsort of the first rows
applied to the rows.  First rows are distinct, so the order is fully determined.

THE DEVICE'S WAY (`device_order`), restated pass by pass so that the ways it can go wrong can be planted:
  records (first row << 32 | index of the group row), `passes` = max(2, ceil(bits / 8)) stable counting passes over the
  digits of the first row, 4096 records a tile; the last pass writes no record: output position g takes the row named by the LOW
  word of the record ranked g.  Positions of a tile at or beyond G hold no record and must not store.
"""
import numpy as np

RS_TILE = 4096
GROUP_COUNTS = [1, 2, 63, 64, 65, 4095, 4096, 4097, 8193, 70_001]
# rows of the batch -> passes its first rows need (bits = smallest b with rows_seen < 2^b): 1, 2, 3 and 4 digits
PASS_ROWS = {200: 1, 40_000: 2, (1 << 20) + 5: 3, (1 << 24) + 5: 4}


def bits_of(rows_seen: int) -> int:
    """hashagg_op.hip: `while (bits < 32 && (1 << bits) <= max(rows_seen, 1)) bits++`"""
    bits = 1
    while bits < 32 and (1 << bits) <= max(rows_seen, 1):
        bits += 1
    return bits


def digits_of(rows_seen: int) -> int:
    return max(1, (min(bits_of(rows_seen), 32) + 7) // 8)


def group_rows(G: int, rows_seen: int, seed: int):
    """(first u32[G], rows u64[G, 4]) in bucket order: distinct first rows below rows_seen with 0 and rows_seen - 1 among them
    (from two groups on), rows {key, cell 0 = a count, cell 1 = the bits of a double, first row}"""
    assert 1 <= G <= rows_seen
    rng = np.random.default_rng(seed)
    if G >= rows_seen // 2:
        first = rng.permutation(rows_seen)[:G]
    else:
        first = np.unique(rng.integers(0, rows_seen, 2 * G + 64))
        first = rng.permutation(first)[:G]
    first = first.astype(np.uint32)
    if G >= 2:  # a first row of 0 and one of rows_seen - 1 (in place of the smallest / largest drawn: still distinct)
        first[np.argmin(first)] = 0
        first[np.argmax(first)] = rows_seen - 1
    assert len(np.unique(first)) == G
    rows = np.empty((G, 4), np.uint64)
    rows[:, 0] = rng.integers(-(1 << 62), 1 << 62, G).astype(np.int64).view(np.uint64)
    rows[:, 1] = rng.integers(1, 1 << 40, G).astype(np.uint64)
    rows[:, 2] = rng.standard_normal(G).view(np.uint64)
    rows[:, 3] = first
    return first, rows


def ordered_rows(first, rows):
    """the rule: [key, cell 0, cell 1] of every group in first-seen order"""
    return rows[np.argsort(first, kind="stable")][:, :3]


def device_order(first, rows, bits, fault=None):
    """[key, cell 0, cell 1] per output position the device's way; positions no record stored to hold ~0.
    fault  None
           "top_digit"   the last pass ranks by digit 0 again instead of the top digit
           "wrong_half"  the row index is taken from the high word of the record (the key half)
           "tail"        the last tile is not cut at G: its empty positions store as well (they hold a copy of record G - 1, as
                         the clamped loads of the kernel give them, and land behind the tile's last position)"""
    G = len(first)
    passes = max(2, (min(bits, 32) + 7) // 8)
    rec = (first.astype(np.uint64) << np.uint64(32)) | np.arange(G, dtype=np.uint64)
    for pi in range(passes):
        last = pi + 1 == passes
        shift = 32 + 8 * (0 if (last and fault == "top_digit") else pi)
        digit = ((rec >> np.uint64(shift)) & np.uint64(255)).astype(np.int64)
        order = np.argsort(digit, kind="stable")  # (per-tile histograms + scan + stable ranks = one stable counting pass)
        if not last:
            rec = rec[order]
            continue
        out = np.full((G + RS_TILE, 3), ~np.uint64(0), np.uint64)
        pos = np.empty(G, np.int64)
        pos[order] = np.arange(G)
        idx = (rec >> np.uint64(32) if fault == "wrong_half" else rec & np.uint64(0xFFFFFFFF)).astype(np.int64)
        idx = np.minimum(idx, G - 1)  # (the model stays inside its arrays; the device would not)
        out[pos] = rows[idx, :3]
        if fault == "tail" and G % RS_TILE:
            # the empty positions of the last tile behave like record G - 1 once more each: ranked behind it, stored behind it
            extra = RS_TILE - G % RS_TILE
            out[pos[G - 1] + 1 + np.arange(extra)] = rows[idx[G - 1], :3]
        return out
    raise AssertionError


def sort_cases():
    """(label, first, rows, bits) over every group count x every pass count the batch sizes give"""
    out = []
    for rows_seen, want in PASS_ROWS.items():
        assert digits_of(rows_seen) == want
        for G in GROUP_COUNTS:
            if G > rows_seen:
                continue
            first, rows = group_rows(G, rows_seen, seed=G + want)
            out.append((f"G{G}_rows{rows_seen}", first, rows, bits_of(rows_seen)))
    return out
