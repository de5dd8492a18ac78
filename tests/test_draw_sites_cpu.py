"""The random draws of the rules that are no Pick, on the host (tests/draw_sites.py: the case table, the plain model written from
the reference's card text, the reference): choice over a list the card builds, shuffle and slice, sort by (key, random()) and
a drawn value, from described states, on every index, rank, winner and value the table demands, for both local orders.

reference() asserts on the recursive oracle, at every stream position it walks (at most 64 per state), that the board after
the step, both bases, the fault code and the stream's cursor are the model's.  Here the host build of the product core
(Oracle(core="product")) must give the oracle's fault code, canonical hash, decision action and score bits for every kept
(state, position).  The same cases on the device: tests/test_draw_sites_gpu.py."""
import numpy as np
import pytest

import draw_sites as D


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def test_every_site_is_covered_and_is_what_the_model_says():
    """reference() asserts each walked position against the plain model; check_coverage() that no atom, order or state is missing."""
    n = D.check_coverage()
    assert n == len(D.reference()["cases"]) > 0
    for site, (states, kept) in D.counts().items():
        print(site, states, kept)


def test_the_table_of_orders_is_whole():
    """Every site whose list reads a point of view is in ORDERS; each of its two orders is either reached by a kept case or
    declared in UNREACHABLE with a reason; a site whose table entry says "none" reads no point of view and is in neither."""
    with_pov = {site for site, s in D.SITES.items() if not s["pov"].startswith("none") and s["form"] != "value"} | {"s003"}
    assert set(D.ORDERS) == with_pov - {"u040"}, (sorted(D.ORDERS), sorted(with_pov))     # (u040's selector has no target: no order)
    cases = D.reference()["cases"]
    for site in D.ORDERS:
        reached = {asc for c in cases if c["site"] == site for asc in c["orders"]}
        assert reached == D.ORDERS[site], (site, reached)
        for asc in (True, False):
            assert (asc in reached) != ((site, asc) in D.UNREACHABLE), (site, asc)
    assert all(why for why in D.UNREACHABLE.values())
    assert {site for site, _ in D.UNREACHABLE} <= set(D.ORDERS)
    for site in D.SITES:
        if site not in D.ORDERS:
            assert not any(c["orders"] for c in cases if c["site"] == site), site


ISSUE_SITES = {"b006", "u040", "u071", "u217", "u406", "ua03", "ua04", "ue03", "s013", "s021", "ua20",     # choice
               "b009", "u017", "u316", "u403", "u411", "ue22", "s004", "s302",                                # shuffle
               "b002", "b104", "b008", "s101",                                                                # sort
               "s003", "u211", "ua07", "confused"}                                                            # value


def test_every_site_of_the_four_forms_is_in_the_table():
    """The cards the issue lists, each a site; u061 is the confused step on play, ue22-own the ascending list of ue22."""
    assert set(D.SITES) == ISSUE_SITES | {"u061", "ue22-own"}
    assert set(D.CONFUSED_ON_PLAY_OUT) == {1, 3} and all(D.CONFUSED_ON_PLAY_OUT.values())


def test_lengths_out():
    """A length the table declares out is in no state's name; a site declared never empty has no empty state."""
    names = {st["name"] for st in D.states()}
    for (site, n), why in D.LENGTHS_OUT.items():
        assert site in D.SITES and why and not any(x.startswith(f"{site}-n{n}-") for x in names), (site, n)
    for site, why in D.NEVER_EMPTY.items():
        assert why and not any(st["empty"] for st in D.states() if st["site"] == site), site


def test_empty_lists():
    """A state whose list is empty draws nothing and steps clean, but for s101, which raises (targets[0] of an empty list);
    the model holds the cursor of each to where the step's other draws leave it."""
    cases = [c for c in D.reference()["cases"] if c["empty"]]
    assert {c["site"] for c in cases} == set(D.SITES) - set(D.NEVER_EMPTY)
    for c in cases:
        assert all(a[0] == "pre" for a in c["atoms"]), c["name"]
        assert c["fault"] == (D.FAULT_PY_EXCEPTION if c["site"] == "s101" else 0), c["name"]
    assert all(c["fault"] == 0 for c in D.reference()["cases"] if not c["empty"])


def test_a_sorted_list_of_one_draws_and_a_choice_over_one_does_not():
    """s101, b002 and b104 at one element: the cursor moves by the two words of one random(), and by six at b008's three
    confused units; ua03 alone in a full row and u217 with one free tile draw no word.  (reference() has held every cursor
    to the model; this names the two rules.)"""
    by_state = {c["state"]: c for c in D.reference()["cases"] if not c["alt"]}
    for name, moved in (("s101-g1-more0-lo0", 2), ("b104-top1-more0-lo1", 2), ("b002-top1-more0-lo0", 2), ("b008-g1-lo0", 6),
                        ("ua03-n1-lo0", 0), ("u217-n1-lo1", 0)):
        c = by_state[name]
        st = next(s for s in D.states() if s["name"] == name)
        m = D.model_step(st, D.P.stream_words(D.oracle_lib.lib(), c["seed"], D.POS0 + D.CAP + 96), c["pos"])
        assert m.rng.cur - (c["pos"] + st["pre"]) == moved, (name, m.rng.cur)


@pytest.mark.parametrize("site", list(D.SITES))
def test_product_core_on_the_host_equals_the_oracle(site):
    """One test per site, so that a failure names the card."""
    ref, prod = D.reference(), D.reference("product")
    assert len(ref["cases"]) == len(prod["cases"])
    pairs = [(a, b) for a, b in zip(ref["cases"], prod["cases"]) if a["site"] == site]
    assert len([1 for a, _ in pairs if not a["alt"]]) == D.counts()[site][1] > 0
    for a, b in pairs:
        name = a["name"]
        assert (a["name"], a["pos"], a["seed"]) == (b["name"], b["pos"], b["seed"])
        assert a["fault"] == b["fault"] and (a["fault"] or a["hash"] == b["hash"]), name
        if a["ext"]:     # ua20 on the standard record: the oracle's fault code and hash there
            assert a["std"]["fault"] == b["std"]["fault"] and (a["std"]["fault"] or a["std"]["hash"] == b["std"]["hash"]), name
        da, db = a["decision"], b["decision"]
        assert da["action"] == db["action"] and da["fault"] == db["fault"] and (da["fault"] or da["hash"] == db["hash"]), name
        nan = np.isnan(da["scores"])
        assert np.array_equal(nan, np.isnan(db["scores"])) and np.array_equal(_bits(da["scores"])[~nan], _bits(db["scores"])[~nan]), name
