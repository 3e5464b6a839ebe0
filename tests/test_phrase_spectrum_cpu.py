"""The phrase-ladder fixtures of tests/phrase_spectrum.py, proven on the CPU before a GPU sees them: the case table names every rung,
every designed doc has the freqs, the pool sum, the place in its term's position stream (block, value index, kind of the block and
of the one behind it), the 16-bit values and the candidate counts its case names - recomputed here from the postings - and the
oracle alone answers every case: a hit (the designed doc and the ordinary doc both) wherever a case is meant to match, the docs a
refused call would have found included, and no hit where the two-phase rule says so."""
import numpy as np
import pytest

import phrase_spectrum as ps


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


RUNGS = (["freq-%d" % f for f in (1, 10, 11, 128, 129, 1024, 1025)] + ["pool-%d" % n for n in (256, 257, 2048, 2049)] +
         ["rpt-pool-%d" % n for n in (256, 257, 2048, 2049)] + ["distinct-6", "distinct-7", "distinct-16", "groups-1", "groups-2", "groups-3", "terms-17"] +
         ["end-%d-behind-%s" % (e, b) for e in (127, 128, 129) for b in ("packed", "equal", "trailing")] + ["end-128-behind-nothing", "first-value-0"] +
         ["skip-packed-docs-tail", "skip-packed-doc-block", "skip-through-equal"] +
         ["singleton-%s-%d" % (w, f) for f in (1, 10, 11) for w in ("first", "last")] +
         ["i16-pos-32767", "i16-pos-32768", "i16-gap-32767", "i16-gap-32768", "i16-offset-minus-32768", "i16-offset-minus-32769",
          "i16-last-of-ten-32767", "i16-last-of-ten-40000"])
# (exact level, slop-1 level) of the rungs the issue words: restated here by hand, not through phrase_spectrum.level
LEVELS = {"freq-1": ("lanes", "lanes"), "freq-10": ("lanes", "lanes"), "freq-11": ("left", "left"), "freq-128": ("left", "left"),
          "freq-129": ("wide", "left"), "freq-1024": ("wide", "wide"), "freq-1025": (None, "wide"),
          "pool-256": ("left", "left"), "pool-257": ("wide", "wide"), "pool-2048": ("wide", "wide"), "pool-2049": (None, None),
          "rpt-pool-256": ("left", "left"), "rpt-pool-257": ("left", "wide"), "rpt-pool-2048": ("wide", "wide"), "rpt-pool-2049": ("wide", None),
          "distinct-6": ("lanes", "lanes"), "distinct-7": ("lanes", "left"), "distinct-16": ("lanes", "left"), "terms-17": (None, None),
          "groups-1": ("lanes", "lanes"), "groups-2": ("lanes", "lanes"), "groups-3": ("lanes", "lanes"),
          "end-128-behind-trailing": ("lanes", "lanes"), "end-128-behind-nothing": ("lanes", "lanes"), "end-128-behind-equal": ("lanes", "lanes"),
          "end-129-behind-packed": ("lanes", "lanes"), "end-129-behind-equal": ("left", "left"), "end-129-behind-trailing": ("left", "left"),
          "skip-packed-docs-tail": ("lanes", "lanes"), "skip-packed-doc-block": ("lanes", "lanes"), "skip-through-equal": ("left", "left"),
          "singleton-first-1": ("left", "left"), "singleton-last-10": ("left", "left"),
          "i16-pos-32767": ("lanes", "lanes"), "i16-pos-32768": ("lanes", "left"), "i16-offset-minus-32768": ("lanes", "lanes"),
          "i16-offset-minus-32769": ("lanes", "left"), "i16-last-of-ten-32767": ("lanes", "lanes"), "i16-last-of-ten-40000": ("lanes", "left")}


def test_the_case_table_names_every_rung():
    cases = dict((c.name, c) for _, c in ps.all_cases())
    assert sorted(cases) == sorted(RUNGS) and len(ps.all_cases()) == len(RUNGS)
    for name, c in cases.items():
        assert [q.slop for q in c.queries] == [0, 1], name          # every rung as an exact and as a slop-1 phrase
        assert all((q.level is None) == (q.error is not None) for q in c.queries), name
    for name, want in LEVELS.items():
        assert tuple(q.level for q in cases[name].queries) == want, (name, [q.level for q in cases[name].queries])
    assert [q.error for q in cases["freq-1025"].queries] == [ps.UNSUPPORTED, None]
    assert [q.error for q in cases["pool-2049"].queries] == [ps.UNSUPPORTED, ps.UNSUPPORTED]
    assert [q.error for q in cases["rpt-pool-2049"].queries] == [None, ps.UNSUPPORTED]
    assert [q.error for q in cases["terms-17"].queries] == [ps.ILLEGAL_ARGUMENT, ps.ILLEGAL_ARGUMENT]
    for name, c in cases.items():   # a phrase that names a term twice is told so (k_sloppy_groups, k_sloppy_rpt_lanes)
        assert [q.rpt for q in c.queries] == [False, len(set(c.queries[1].terms)) < len(c.queries[1].terms)], name
    assert ps.CHUNK_NS == (8191, 8192, 8193, 16385) and ps.KS == (1, 10, 64, 65, 128, 129, 300)
    assert [ps.chunks(n).first for n in ps.CHUNK_NS] == [[0, 8190], [0, 8191], [0, 8191, 8192], [0, 8191, 8192, 8193, 16384]]


@pytest.mark.parametrize("name", list(ps.BUILDERS))
def test_fixtures_have_the_shape_their_names_say(name):
    s = ps.segment(name)
    assert s.max_doc <= 20_000 and s.doc_count == s.max_doc == len({d for pl in s.postings for d, _ in pl})
    holders = {}
    for t, pl in enumerate(s.postings):
        assert [d for d, _ in pl] == sorted({d for d, _ in pl})
        for d, positions in pl:
            holders.setdefault(d, {})[t] = positions
    special = {c.designed for c in s.cases} | {c.ordinary for c in s.cases}
    assert all(len(h) == 1 for d, h in holders.items() if d not in special)     # a filler doc holds one term alone
    used = [t for c in s.cases for t in set(c.queries[0].terms)]
    assert len(used) == len(set(used)) == len(s.postings)                       # every case has terms of its own
    for c in s.cases:
        sh, q = c.shape, c.queries[0]
        freqs = {t: len(holders[c.designed][t]) for t in set(q.terms)}
        assert freqs == sh["freqs"], c.name
        together = set.intersection(*[{d for d, _ in s.postings[t]} for t in set(q.terms)])
        if len(set(q.terms)) > 1:   # the phrase's terms occur together in the designed doc and the ordinary doc only
            assert together == ({c.designed} if "singleton" in sh else {c.designed, c.ordinary}), c.name
            if "singleton" not in sh:
                assert all(len(holders[c.ordinary][t]) == q.terms.count(t) for t in set(q.terms)), c.name
        else:                       # [x, x]: every doc of x is a candidate; but for the designed doc they hold it four times at most
            assert all(len(positions) <= 4 for d, positions in s.postings[q.terms[0]] if d != c.designed), c.name
        for t in set(q.terms) - {sh.get("singleton")}:   # the 64-candidate kernels can take the ordinary doc: inside packed blocks, one block
            if len(set(q.terms)) > 1 or c.name == "groups-1":
                pl = ps.place(s.postings[t], c.ordinary)
                assert set(pl["between"]) == {"packed"} and (pl["block"] == pl["last_block"] or pl["behind"] == "packed"), (c.name, t)
        if c.rung in ("freq", "pool", "terms"):          # so can they the designed doc, as far as its place goes
            for t in set(q.terms):
                pl = ps.place(s.postings[t], c.designed)
                assert set(pl["between"]) == {"packed"} and pl["ttf"] >= ps.BLOCK, (c.name, t, pl)
        if c.rung == "freq":
            f = int(c.name.split("-")[1])
            assert sorted(freqs.values()) == sorted([1, f]) and q.terms.count(q.terms[0]) == 1, c.name
        if "pool" in sh:
            assert sum(freqs[t] for t in q.terms) == sh["pool"] == int(c.name.split("-")[-1]), c.name
            assert (len(set(q.terms)) < len(q.terms)) == c.name.startswith("rpt"), c.name
        if "first_candidate" in sh:
            x = sh["first_candidate"]
            assert q.terms == [x, x] and s.postings[x][0][0] == c.designed and freqs[x] in (ps.SMALL_CAP, ps.LIST_CAP), c.name
        if "n_terms" in sh:
            assert len(q.terms) == sh["n_terms"] and len(set(q.terms)) == (sh["groups"] if "groups" in sh else min(sh["n_terms"], ps.MAX_TERMS)), c.name
        if c.name == "groups-1":   # no trailing block: every candidate of [x, x] lies in packed blocks
            assert ps.place(s.postings[q.terms[0]], c.designed)["ttf"] % ps.BLOCK == 0
        if "placed" in sh:
            pl = ps.place(s.postings[sh["placed"]], c.designed)
            assert (pl["block"], pl["skip"], pl["kind"]) == (sh["block"], sh["skip"], sh["kind"]) and pl["freq"] <= ps.LANE_CAP, (c.name, pl)
            assert pl["df"] > 1 and pl["ttf"] >= ps.BLOCK
            if "end" in sh:
                assert pl["skip"] + pl["freq"] == sh["end"] and pl["last_block"] - pl["block"] == (1 if sh["end"] > ps.BLOCK else 0), (c.name, pl)
            if "behind" in sh:
                assert pl["behind"] == sh["behind"] == c.name.split("-")[-1], (c.name, pl)
                assert (pl["ttf"] % ps.BLOCK == 0 and pl["ttf"] == ps.BLOCK * (pl["block"] + 1)) == (sh["behind"] == "nothing"), (c.name, pl)
            if "kernel_skip_min" in sh:
                assert pl["kernel_skip"] >= sh["kernel_skip_min"] and len(pl["skipped"]) >= 1, (c.name, pl)
                assert sh["through"] is None or pl["skipped"] == sh["through"], (c.name, pl)
                assert ("equal" in pl["skipped"]) == (c.name == "skip-through-equal")
            other = [t for t in q.terms if t != sh["placed"]][0]   # the other term does not decide the case: inside one packed block
            po = ps.place(s.postings[other], c.designed)
            assert po["kind"] == "packed" and po["block"] == po["last_block"], (c.name, po)
        if "singleton" in sh:
            x = sh["singleton"]
            assert len(s.postings[x]) == 1 and s.postings[x][0][0] == c.designed and q.terms.index(x) == (0 if "first" in c.name else 1), c.name
            assert freqs[x] == int(c.name.split("-")[-1])
        if "value" in sh:           # position - phrase offset, per phrase term, in the designed doc
            offs = q.positions or list(range(len(q.terms)))
            values = [p - o for t, o in zip(q.terms, offs) for p in holders[c.designed][t]]
            assert sh["value"] in values and (min(values) >= -32768 and max(values) <= 32767) == sh["fits"], (c.name, values)
            assert sh["value"] in (32767, 32768, -32768, -32769, 40000), c.name
            if "in_range" in sh:    # the last position alone is out of range
                a = holders[c.designed][q.terms[0]]
                assert len(a) == ps.LANE_CAP and a[-1] == sh["value"] and a[-2] == sh["in_range"] <= 32767, c.name
            for t, o in zip(q.terms, offs):   # the ordinary doc fits the 16-bit lists in every case
                assert all(-32768 <= p - o <= 32767 for p in holders[c.ordinary][t]), c.name


@pytest.mark.parametrize("name,version", [("freq", 1), ("terms", 1), ("place", 1), ("place", 0)])
def test_the_oracle_answers_every_case(oracle, name, version):
    """The designed doc and the ordinary doc are hits of the exact and of the slop-1 phrase - of the queries the library refuses
    (1025 positions, a pool of 2049, 17 terms) as well - and the oracle's reader gives back every position of the rung terms."""
    s = ps.segment(name)
    ix = s.index(oracle, version)
    try:
        for c in s.cases:
            for q in c.queries:
                d, sc, total = s.search(ix, q, 1000)
                assert total == d.size >= 1 and c.designed in d.tolist(), (c.name, q.slop, total)
                if "singleton" not in c.shape:
                    assert c.ordinary in d.tolist() and total >= 2, (c.name, q.slop)
                if len(set(q.terms)) > 1:
                    assert total == (1 if "singleton" in c.shape else 2), (c.name, q.slop, total)
                assert np.isfinite(sc).all() and (sc > 0).all()
            for t in set(c.queries[0].terms):
                assert [(dd, p) for dd, _, p in ix.iterate(t)] == [(dd, p) for dd, p in s.postings[t]], (c.name, t)
    finally:
        ix.close()


@pytest.mark.parametrize("n", ps.CHUNK_NS)
def test_chunk_fixtures_and_the_two_phase_rule(oracle, n):
    """n candidates per pair of terms, the first phrase match at the index named; the oracle yields hits iff at most next_limit
    candidates precede the first collected doc (deleted candidates count), exact phrases whatever the limit."""
    fx = ps.chunks(n)
    assert fx.max_doc == n <= 20_000 and len(fx.postings) == 2 * len(fx.first)
    ix = fx.index(oracle)
    try:
        for j, i in enumerate(fx.first):
            p, q = fx.postings[2 * j], fx.postings[2 * j + 1]
            assert len(p) == len(q) == n and [d for d, _ in p] == list(range(n))          # the conjunction: n candidates
            m = fx.matches[j]
            assert int(np.argmax(m)) == i and m[i] and not m[:i].any() and m.sum() == 1 + sum(1 for d in range(i + 1, n) if d % ps.EVERY == 0)
            for d in (i, max(i - 1, 0), n - 1):
                near = any(abs(a - b) <= 2 for a in p[d][1] for b in q[d][1])
                assert near == bool(m[d])
            exact, sloppy, rpt = fx.queries(j)
            for limit in fx.limits(j):
                yields = i <= (ps.DEFAULT_NEXT_LIMIT if limit is None else limit)
                for qq in (exact, sloppy, rpt):
                    d, sc, total = fx.search(ix, qq, 10, next_limit=limit)
                    assert total == (int(m.sum()) if yields or qq.slop == 0 else 0), (n, i, limit, qq.terms, qq.slop, total)
                    assert d.size == min(10, total) and (d.size == 0 or d.min() >= i)
            assert {i - 1, i, i + 1, n - 1, n, 0} - {-1} <= set(fx.limits(j)) and None in fx.limits(j)
        if n > ps.CHUNK:
            # the first chunk's candidates deleted: the first live one is candidate 8192, the deleted ones count as approximations
            alive = np.arange(n) >= ps.CHUNK
            live = fx.live_words(alive)
            assert live.size == (n + 63) // 64 and not live[:ps.CHUNK // 64].any() and int(live[ps.CHUNK // 64]) & 1
            j = fx.first.index(ps.CHUNK)
            for qq in fx.queries(j)[1:]:
                assert fx.search(ix, qq, 10, live_docs=live, next_limit=ps.CHUNK)[2] == int(fx.matches[j].sum())
                assert fx.search(ix, qq, 10, live_docs=live, next_limit=ps.CHUNK - 1)[2] == 0
            for j in range(len(fx.first)):
                for qq in fx.queries(j):
                    want = int((fx.matches[j] & alive).sum())
                    assert fx.search(ix, qq, 10, live_docs=live)[2] == want and (want > 0 or (n == ps.CHUNK + 1 and fx.first[j] != ps.CHUNK))
                    assert fx.search(ix, qq, 10, live_docs=fx.live_words(np.zeros(n, dtype=bool)))[2] == 0
    finally:
        ix.close()
