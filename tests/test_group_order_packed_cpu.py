"""The ordering of pre-aggregated groups stored as 32-byte rows, on the CPU: the rule (a stable argsort of the first rows applied
to the rows) against the device's way restated in numpy (group_order_packed_cases.device_order), over every group count x every
pass count of the shared cases — and the three ways the last pass can go wrong, planted and rejected.

A planted fault is only asked to show where it can:
  top_digit   needs first rows that differ above digit 0 and enough groups for two of them to disagree (from 63 groups on, and a
              batch of more than 256 rows: below that the top digit is zero everywhere and ranking by digit 0 twice is harmless)
  wrong_half  needs groups whose first row is not their own index (from 63 groups on)
  tail        needs a last tile with empty positions (G no multiple of 4096); shown from 63 groups on, by a store behind
              position G - 1 or over another group's position
"""
import numpy as np
import pytest

import group_order_packed_cases as P

CASES = P.sort_cases()
IDS = [c[0] for c in CASES]


def settled(out, G):
    """rows the device's way stored, after checking that nothing was stored behind the last group"""
    assert (out[G:] == ~np.uint64(0)).all(), "a position at or behind G was stored to"
    return out[:G]


def test_the_cases_cover_what_the_issue_names():
    assert sorted({P.digits_of(r) for r in P.PASS_ROWS}) == [1, 2, 3, 4]
    assert {4095, 4096, 4097} <= set(P.GROUP_COUNTS) and P.RS_TILE == 4096
    assert 70_001 % P.RS_TILE and 70_001 // P.RS_TILE > 16  # a ragged last tile behind more than 16 full ones
    for _, first, _, bits in CASES:
        if len(first) >= 2:
            assert first.min() == 0 and int(first.max()) + 1 < (1 << bits)
    assert any(int(first.max()) == (1 << 24) + 4 for _, first, _, _ in CASES)  # a first row of rows - 1


@pytest.mark.parametrize("label,first,rows,bits", CASES, ids=IDS)
def test_device_order_is_the_rule(label, first, rows, bits):
    G = len(first)
    want = P.ordered_rows(first, rows)
    assert (rows[np.argsort(first, kind="stable")][:, 3] == np.sort(first)).all()
    got = settled(P.device_order(first, rows, bits), G)
    assert (got == want).all(), label


@pytest.mark.parametrize("fault", ["top_digit", "wrong_half", "tail"])
@pytest.mark.parametrize("label,first,rows,bits", CASES, ids=IDS)
def test_planted_fault_is_rejected(label, first, rows, bits, fault):
    G = len(first)
    can_show = G >= 63
    if fault == "top_digit":
        can_show &= bits > 8
    if fault == "tail":
        can_show &= G % P.RS_TILE != 0
    out = P.device_order(first, rows, bits, fault)
    same = (out[G:] == ~np.uint64(0)).all() and (out[:G] == P.ordered_rows(first, rows)).all()
    if can_show:
        assert not same, f"{label}: the fault {fault} went unnoticed"
    elif fault == "tail" and G % P.RS_TILE == 0:
        assert same  # (no empty position: nothing to mask)
