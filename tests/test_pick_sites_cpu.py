"""Every call site of an ability's random pick, on the host (tests/pick_sites.py: the case table, the plain model, the
reference): sixteen sites, every list length the table gives a site, every index r the draw can give, both local orders, the
ascending and the descending list wherever a step reaches them.

reference() asserts on the recursive oracle that every case is what it is named after -- the element the step changed is the
plain model's list[r], the stream's cursor stands where the model's draw leaves it, an empty list draws nothing (or raises, for
u017; the bot's cannot be reached) -- and finds the stream positions that are kept, at most 64 walked per state.  Here the host build of the
product core (Oracle(core="product"), which compiles the pick on the hit mask) must give the oracle's fault code, canonical
hash, bot action and decision for every kept (state, position).  The same cases on the device: tests/test_pick_sites_gpu.py."""
import numpy as np
import pytest

import pick_sites as P


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def test_every_site_is_covered_and_is_what_it_is_named_after():
    """reference() asserts each case against the plain model; check_coverage() that no site, length, index or order is missing."""
    n = P.check_coverage()
    assert n == len(P.reference()["cases"]) > 0
    for site, (states, kept) in P.counts().items():
        print(site, states, kept)


def test_the_table_of_orders_is_whole():
    """Each (site, order) pair is either reached by one of the site's modes or declared unreachable with a reason; the
    descending order is reached for exactly the me / arg sites that run in the other player's turn (and s012, whose order is
    its caster's ORDER)."""
    cases = P.reference()["cases"]
    desc = {c["site"] for c in cases if not c["asc"]}
    assert desc == {"u007", "u111", "ud01", "ue01", "s012"}, desc
    assert {c["site"] for c in cases if c["asc"]} == set(P.SITES)
    assert {site for site, asc in P.UNREACHABLE} == set(P.SITES) - desc and all(not asc and why for (_, asc), why in P.UNREACHABLE.items())
    for (site, mode, n), why in P.LENGTHS_OUT.items():
        assert mode in P.SITES[site]["modes"] and n not in P.lengths(site, mode) and why


def test_empty_lists():
    """u017 raises at an empty list; every other site steps clean and leaves the stream to the rest of the step (reference()
    holds the cursor to the model).  The bot's empty list cannot be reached: P.LENGTHS_OUT says why."""
    cases = [c for c in P.reference()["cases"] if c["n"] == 0]
    assert {c["site"] for c in cases} == set(P.SITES) - {"u018", "bot"}
    for c in cases:
        assert c["fault"] == (P.FAULT_PY_EXCEPTION if c["site"] == "u017" else 0), c["name"]


def test_base_elements():
    """u018's list ends in the enemy base at every length: the last index lands on it, no other does.  (No site's descriptor
    holds two bases, so a base is never second to last; u306's descriptor has no include_base, so its list holds none.)"""
    for c in P.reference()["cases"]:
        if c["site"] == "u018":
            assert (c["element"] == ("base", 1 - c["lo"])) == (c["r"] == c["n"] - 1), c["name"]
        else:
            assert not isinstance(c["element"], tuple), c["name"]


@pytest.mark.parametrize("site", list(P.SITES))
def test_product_core_on_the_host_equals_the_oracle(site):
    """One test per site, so that a failure says where."""
    ref, prod = P.reference(), P.reference("product")
    assert len(ref["cases"]) == len(prod["cases"])
    pairs = [(a, b) for a, b in zip(ref["cases"], prod["cases"]) if a["site"] == site]
    assert len(pairs) == P.counts()[site][1] > 0
    for a, b in pairs:
        name = a["name"]
        assert (a["name"], a["pos"], a["seed"]) == (b["name"], b["pos"], b["seed"])
        assert a["fault"] == b["fault"] and (a["fault"] or a["hash"] == b["hash"]), name
        assert a.get("bot_action") == b.get("bot_action") and a.get("bot_fault") == b.get("bot_fault"), name
        da, db = a["decision"], b["decision"]
        assert da["action"] == db["action"] and da["fault"] == db["fault"] and (da["fault"] or da["hash"] == db["hash"]), name
        nan = np.isnan(da["scores"])
        assert np.array_equal(nan, np.isnan(db["scores"])) and np.array_equal(_bits(da["scores"])[~nan], _bits(db["scores"])[~nan]), name
