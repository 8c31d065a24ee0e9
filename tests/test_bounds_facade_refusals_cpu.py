"""The eight bounds facades refuse what they refused, with the words they used, and for a call with two faults the one
they named first: the table of tests/helpers/bounds_refusal_cases.py replayed against tests/golden/bounds_facade_refusals.json,
which tools/capture_bounds_refusals.py wrote at the commit before the facades were put on shared argument checks."""
import json
import os

import pytest

from helpers import bounds_refusal_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "bounds_facade_refusals.json")) as f:
    GOLDEN = json.load(f)


def test_the_table_covers_the_eight_facades_with_the_recorded_sets():
    assert list(rc.FACADES) == ["price_american_bounds", "price_american_bounds_heston", "price_american_bounds_jumps",
                                "price_american_bounds_dividends", "price_barrier_bounds", "price_american_basket_bounds",
                                "price_bermudan_bounds", "price_american_bounds_checked"]
    assert sorted(GOLDEN["facades"]) == sorted(rc.FACADES)
    assert len(GOLDEN["commit"]) >= 7
    assert len(GOLDEN["messages"]) == len({tuple(m) for m in GOLDEN["messages"]})
    for name, (_, sets) in rc.FACADES.items():
        n = len(sets)
        assert GOLDEN["facades"][name]["sets"] == list(sets), name  # none dropped, none reordered
        assert len(GOLDEN["facades"][name]["first"]) == n + n * (n - 1) // 2 == len(list(rc.calls(name))), name


@pytest.mark.parametrize("facade", list(rc.FACADES))
def test_every_set_alone_is_refused(facade):
    """each set hits a check: alone, none of them reaches the context -- but the few that are there to say so"""
    no_sigma = {"heston-no-sigma"}  # (sigma only sets defaults under Heston: in the table for its pairs)
    passing = {"price_american_basket_bounds": {"correlation"},  # (the library's check of the matrix comes with the context)
               "price_american_bounds": {"given-short"},         # (the context method's check of the shape)
               "price_american_bounds_jumps": no_sigma, "price_american_bounds_dividends": no_sigma,
               "price_barrier_bounds": no_sigma,
               "price_bermudan_bounds": {"heston"}, "price_american_bounds_checked": {"heston", "policy", "option-type"}}
    first = GOLDEN["facades"][facade]["first"]
    for i, name in enumerate(rc.FACADES[facade][1]):
        assert (GOLDEN["messages"][first[i]] == rc.REACHED) == (name in passing.get(facade, ())), name


@pytest.mark.parametrize("facade", list(rc.FACADES))
def test_facade_raises_what_it_raised_first(facade):
    first = GOLDEN["facades"][facade]["first"]
    wrong = []
    for (name, kwargs), i in zip(rc.calls(facade), first):
        got = rc.outcome(facade, kwargs)
        if got != GOLDEN["messages"][i]:
            wrong.append((name, got, GOLDEN["messages"][i]))
    assert not wrong, (len(wrong), wrong[:5])
