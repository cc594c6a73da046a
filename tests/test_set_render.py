"""Interval strings (jepsen.util/integer-interval-set-str) from run lists, as
lincheck.setcheck renders lc_set_result.runs."""
import numpy as np
import pytest

import set_helpers as SH
from lincheck.setcheck import interval_str

BIG = SH.I64_MAX


@pytest.mark.parametrize("runs,want", [
    ([], "#{}"),
    ([(5, 5)], "#{5}"),
    ([(3, 3), (20, 20)], "#{3 20}"),
    ([(7, 8)], "#{7..8}"),
    ([(0, 2), (4, 8)], "#{0..2 4..8}"),
    ([(-9, -7), (-1, 1)], "#{-9..-7 -1..1}"),
    ([(-BIG, -BIG), (BIG - 1, BIG)], f"#{{{-BIG} {BIG - 1}..{BIG}}}"),
    ([(BIG, BIG)], f"#{{{BIG}}}"),
])
def test_interval_strings(runs, want):
    assert interval_str(runs) == want
    assert interval_str(np.array(runs, np.int64).reshape(len(runs), 2).tolist()) == want
    # and the restatement's own rendering of the same elements agrees
    if all(b - a < 1000 for a, b in runs):
        assert SH.interval_str({x for a, b in runs for x in range(a, b + 1)}) == want
