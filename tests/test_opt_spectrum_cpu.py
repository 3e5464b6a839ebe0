"""The fixtures of tests/opt_spectrum.py, proven on the CPU before a GPU sees them: every sequence has the property it is named for -
where the 101st scored match lies, which docs the reference skips -, the oracle's ReqOptScorer rows are OptRef's bit for bit, with
the rule and with exact=True, on one leaf and on two; every mutant of the rule changes the row of a named fixture; every optional
clause gets the structure the host rules give it; the two searches over the (freq, norm byte) grid find what the module records."""
import math

import numpy as np
import pytest

import and_spectrum as as_
import opt_spectrum as os_
from and_spectrum import ABSENT, C_511, C_512, C_1171, C_1172, C_2344, CORE_LEAD, EDGE_LEAD, EVERY, FP_LEAD, OVF_CAP, OVF_OVER, OVF_SMALL, Q_LEAD, S_LEAD, SPREAD
from opt_spectrum import HIGH, LOW, MID, R_TERM, Query

VARIANTS = [("rank", "none", 1), ("raw", "seeded", 0), ("none", "seeded", 1)]
CPU_KS = (10, 129)
K_ALL = 300                      # every rule fixture has at most 300 hits: the whole sequence is in the row


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


_refs = {}


def _ref(oracle, leaf):
    if leaf.key not in _refs:
        _refs[leaf.key] = os_.OptRef(oracle, leaf, oracle.Searcher([leaf.oracle_segment(oracle)]))
    return _refs[leaf.key]


def _same(a, b):
    return a[2] == b[2] and a[0].tolist() == b[0].tolist() and a[1].view(np.int32).tolist() == b[1].view(np.int32).tolist()


def _pattern(ref, name):
    """-> (the sequence's postings that match, skipped per match, the rule's decisions) of one rule fixture."""
    q, leaf = os_.rule_queries()[name], ref.leaf
    trace = []
    docs, final, skipped, req, opt, _ = ref.walk(q, trace=trace)
    posts = leaf.posts["S100" if name == "OPT_MISS" else name]
    first = leaf.first["S100" if name == "OPT_MISS" else name]
    matched = [posts[int(d) - first] for d in docs]
    return matched, skipped, final, req, opt, trace


def test_the_constants_are_the_kernels():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    read = lambda *p: open(os.path.join(root, *p)).read()   # noqa: E731
    kernel, api = read("rucene_amd", "csrc", "kernels", "search_and.hpp"), read("rucene_amd", "csrc", "rgpu_api.hip")
    dec, ref_rs = read("rucene_amd", "csrc", "kernels", "decode_terms.hpp"), read("oracle", "search.hpp")
    assert int(re.search(r"constexpr int REQ_OPT_THRESHOLD = (\d+);", kernel).group(1)) == os_.THRESHOLD == 100
    assert "constexpr size_t OPT_SCORE_THRESHOLD = 100;" in ref_rs
    assert "if (scores_num > REQ_OPT_THRESHOLD) skip = 2.0f * score < scores_sum / (float)scores_num;" in kernel
    assert "for (int64_t at = i0; at < i1; at += 64)" in kernel and os_.SCAN_STEP == 64
    assert "const int32_t ord = ord0 + 2 * lane;" in kernel and "if (ord + 1 < L.df) rec[1]" in kernel
    assert "constexpr int WG_THREADS = 256;" in dec and "constexpr int WG_WAVES = WG_THREADS / 64;" in dec and os_.WG_WAVES == 4
    assert "blockIdx.x * WG_WAVES) + wave_id()" in kernel                       # one wavefront per query
    # the host: a required disjunction of ten is refused, optional clauses are not counted; membership bits alone are asked for a MUST clause
    assert "(Q.op & RGPU_OP_SHOULD_REQUIRED) && qopt >= 10" in api
    assert "if (qop == RGPU_OP_AND && Q.n_terms >= 2 && c->cfg.and_bitmaps >= 0 && c->memb_only_on" in api
    assert "n_look = Q.n_terms + qopt + qbehind; min_df = min_df_and;" in api
    assert os_.KS == as_.KS and os_.BLOCK == as_.BLOCK


@pytest.mark.parametrize("version", os_.VERSIONS)
def test_the_doc_bytes_decode_to_the_lists(oracle, version):
    for which in "AB":
        leaf = os_.RuleLeaf(version=version, which=which)
        seg = leaf.oracle_segment(oracle)
        assert seg.version == version
        for t, (d, f) in enumerate(leaf.lists):
            gd, gf = seg.decode_term(leaf.seg.terms[t])
            assert (gd == d).all() and (gf == f).all(), os_.R_NAMES[t]


def test_the_rule_leaf_is_laid_out_as_named():
    leaf = os_.RuleLeaf()
    assert leaf.max_doc == 4099 and leaf.max_doc % 32 == 3
    assert all(leaf.df(R_TERM[n]) <= 300 for n in os_.R_NAMES[len(os_.R_FIXED):])
    assert [leaf.df(R_TERM["DF_%d" % n]) for n in os_.DF_SIZES] == list(os_.DF_SIZES) == [1, 2, 127, 128, 129, 257]
    assert leaf.df(R_TERM["EQUAL"]) == leaf.df(R_TERM["F64"]) == os_.SEARCHED_DF
    ranges = sorted((leaf.first[n], leaf.first[n] + len(p)) for n, p in leaf.posts.items())
    assert all(a[1] < b[0] for a, b in zip(ranges, ranges[1:]))              # a doc range of its own each: a doc's norm byte is its level
    assert leaf.has[os_.R_ALL].all() and leaf.df(os_.R_THIRD) == -(-leaf.max_doc // 3)
    for name, posts in leaf.posts.items():
        for i, p in enumerate(posts):
            if p is None:
                continue
            d = leaf.first[name] + i
            assert leaf.norms[d] == p.byte and leaf.has[os_.R_HOLD][d] == (p.dead != "lack") and leaf.has[os_.R_BAN][d] == (p.dead == "not")
            assert os_.RuleLeaf(live="seeded").alive[d] == (p.dead != "del")
    assert np.unique(os_.RuleLeaf("rank").norms).size <= 30 and np.unique(os_.RuleLeaf("raw").norms).size >= 65 and os_.RuleLeaf("none").norms is None
    assert not os_.RuleLeaf(live="seeded").alive.all()
    # the dead postings of the four DEAD fixtures: one kind each, and all three
    kinds = lambda n: {p.dead for p in leaf.posts[n] if p.dead}   # noqa: E731
    assert [kinds(n) for n in ("DEAD_LACK", "DEAD_NOT", "DEAD_DEL", "DEAD_ALL")] == [{"lack"}, {"not"}, {"del"}, {"lack", "not", "del"}]
    assert all(sum(1 for p in leaf.posts[n] if p.dead) == 25 for n in ("DEAD_LACK", "DEAD_NOT", "DEAD_DEL", "DEAD_ALL"))
    # leaf B differs in TWO alone
    b = os_.RuleLeaf(which="B")
    for t in range(len(os_.R_NAMES)):
        same = b.lists[t][0].tolist() == leaf.lists[t][0].tolist() and b.lists[t][1].tolist() == leaf.lists[t][1].tolist()
        assert same == (t != R_TERM["TWO"])


@pytest.mark.parametrize("norms", os_.NORMS)
@pytest.mark.parametrize("live", os_.LIVE)
def test_the_levels_hold_in_every_state(oracle, norms, live):
    """2 * LOW < mean <= 2 * HIGH whenever the rule decides, in every sequence built from the three levels; MID lies on LOW's side
    while the mean is HIGH's."""
    ref = _ref(oracle, os_.RuleLeaf(norms, live))
    decisions = 0
    for name in os_.RULE_NAMES:
        if name in ("EQUAL", "F64"):
            continue
        matched, skipped, final, req, opt, trace = _pattern(ref, name)
        level = lambda lv: [float(r) for p, r in zip(matched, req) if (p.freq, p.byte) == lv]   # noqa: E731
        lows, highs, mids = level(LOW), level(HIGH), level(MID)
        assert highs and len(set(highs)) == 1 and len(set(lows)) <= 1
        for i, num, mean, two in trace:
            decisions += 1
            assert num > 100
            assert 2.0 * highs[0] >= float(mean), (name, num)
            assert not lows or 2.0 * lows[0] < float(mean), (name, num)
            if mids and name != "DF_257":
                assert 2.0 * mids[0] < float(mean)
        if mids and norms != "none":
            assert lows[0] < mids[0] < highs[0]
        assert (opt > 0).all() or name == "OPT_MISS"                      # ALL holds every doc: a doc that is not skipped shows it
        assert ((final > req) == ~skipped).all() or name == "OPT_MISS"
    assert decisions > 500


@pytest.mark.parametrize("norms", os_.NORMS)
def test_every_sequence_is_skipped_where_its_name_says(oracle, norms):
    ref = _ref(oracle, os_.RuleLeaf(norms, "seeded"))
    none = _ref(oracle, os_.RuleLeaf(norms, "none"))
    low = lambda matched, skipped: [bool(s) for p, s in zip(matched, skipped) if (p.freq, p.byte) == LOW]   # noqa: E731
    for n, taking in ((99, 2), (100, 1), (101, 0)):
        matched, skipped = _pattern(ref, "S%d" % n)[:2]
        assert low(matched, skipped) == [False] * taking + [True] * (20 - taking) and not skipped[:n].any(), n
    # KEEPS_STATE: every LOW and every MID skipped, the HIGHs behind them not; the mean the MIDs meet is the one the first LOW met
    matched, skipped, final, req, opt, trace = _pattern(ref, "KEEPS_STATE")
    assert skipped.tolist() == [False] * 101 + [True] * 123 + [False] * 2
    assert len({float(m) for _, _, m, _ in trace[:-2]}) == 1 and {num for _, num, _, _ in trace[:-2]} == {101}
    mid = [r for p, r in zip(matched, req) if (p.freq, p.byte) == MID][0]
    lows = [r for p, r in zip(matched, req) if (p.freq, p.byte) == LOW]
    had_they_entered = (float(trace[0][2]) * 101 + float(np.sum(lows, dtype=np.float64))) / (101 + len(lows))
    assert 2.0 * float(mid) >= had_they_entered                                  # ... and would not be skipped had the LOWs entered the mean
    # DEAD_*: 25 dead lead postings among the 100 HIGH ones, and the first LOW still takes the optional sum
    for name in ("DEAD_LACK", "DEAD_NOT", "DEAD_DEL", "DEAD_ALL"):
        matched, skipped = _pattern(ref, name)[:2]
        assert len(matched) == 120 and not any(p.dead for p in matched) and low(matched, skipped) == [False] + [True] * 19, name
        lead = ref.leaf.lists[R_TERM[name]][0]
        assert lead.size == 145 and ref.records(os_.rule_queries()[name])[1].sum() == 120
    assert len(_pattern(none, "DEAD_DEL")[0]) == 145                             # (without deletions those 25 are HIGH matches like the others)
    # OPT_MISS: two docs in three lack the optional term and count all the same
    matched, skipped, final, req, opt, trace = _pattern(ref, "OPT_MISS")
    hit = ref.records(os_.rule_queries()["OPT_MISS"])[4]
    assert 30 < hit.sum() < 50 and low(matched, skipped) == [False] + [True] * 19 and ((final > req) == (hit & ~skipped)).all()
    # STEP_*: the 101st scored match is lead record 127 .. 193; every LOW behind it is skipped
    for at in os_.STEP_AT:
        q = os_.rule_queries()["STEP_%d" % at]
        match = ref.records(q)[1]
        assert int(np.flatnonzero(match)[100]) == at and not match[:at - 100].any() and match[at - 100:].all()
        matched, skipped = _pattern(ref, "STEP_%d" % at)[:2]
        assert skipped.tolist() == [False] * 101 + [True] * 10
    assert {a % 64 for a in os_.STEP_AT} == {63, 0, 1} and {a // 128 for a in os_.STEP_AT} == {0, 1} and {a % 2 for a in os_.STEP_AT} == {0, 1}
    # DF_*: 101 HIGH in front wherever the list is long enough
    for df in os_.DF_SIZES:
        matched, skipped = _pattern(ref, "DF_%d" % df)[:2]
        assert len(matched) == df and skipped[:101].sum() == 0 and (df <= 101 or skipped[101:201].all())
    assert _pattern(ref, "DF_257")[1].tolist() == [False] * 101 + [True] * 110 + [False] * 46
    leaf = ref.leaf
    assert leaf.seg.terms[R_TERM["DF_1"]]["doc_freq"] == 1 and leaf.df(R_TERM["DF_127"]) // 128 == 0 and leaf.df(R_TERM["DF_128"]) % 128 == 0
    # TWO: leaf B's first 101 scored docs take the optional sum - its scorer is fresh -, the 10 LOWs behind them do not
    a, b = os_.RuleLeaf(norms, "seeded"), os_.RuleLeaf(norms, "seeded", which="B", doc_base=os_.R_MAX_DOC)
    osr = oracle.Searcher([a.oracle_segment(oracle), b.oracle_segment(oracle)])
    ra, rb = os_.OptRef(oracle, a, osr), os_.OptRef(oracle, b, osr)
    q = os_.rule_queries()["TWO"]
    assert ra.walk(q)[2].tolist() == [False] * 101 + [True] * 20 and rb.walk(q)[2].tolist() == [False] * 110 + [True] * 10
    assert rb.walk(q, state=ra.walk(q)[5])[2][:5].all()                            # (carried over, B's LOWs in front would be skipped)


@pytest.mark.parametrize("norms", ("rank", "raw"))
def test_equal_and_f64_are_what_the_searches_found(oracle, norms):
    """EQUAL: 2 * req == sum / num exactly, and the strict `<` keeps the optional sum; F64: the f32 mean skips the doc, an f64 sum's
    would not. Both searches, run again, return the module's constants."""
    ref = _ref(oracle, os_.RuleLeaf(norms, "none"))
    matched, skipped, final, req, opt, trace = _pattern(ref, "EQUAL")
    i, num, mean, two = trace[0]
    assert (i, num) == (101, 101) and two == mean and two.dtype == mean.dtype == np.float32 and not skipped[101] and final[101] > req[101]
    assert ref.walk(os_.rule_queries()["EQUAL"], le=True)[2][101]
    matched, skipped, final, req, opt, trace = _pattern(ref, "F64")
    assert trace[0][:2] == (101, 101) and skipped[101] and not ref.walk(os_.rule_queries()["F64"], f64=True)[2][101]
    w, cache = ref.osr.term_weight(R_TERM["EQUAL"])
    assert np.float32(w) == np.float32(math.log(1.0 + (os_.R_MAX_DOC - os_.SEARCHED_DF + 0.5) / (os_.SEARCHED_DF + 0.5)))
    assert os_.equal_search(w, cache) == os_.EQUAL_FOUND and os_.f64_search(w, cache) == os_.F64_FOUND
    grid = os_.grid_scores(w, cache)                                               # the grid is the oracle's arithmetic
    lead = ref.leaf.lists[R_TERM["EQUAL"]]
    sc = ref.term_scores(R_TERM["EQUAL"])[lead[0]]
    assert all(sc[j].view(np.int32) == grid[f - 1, ref.leaf.norms[d]].view(np.int32) for j, (d, f) in enumerate(zip(*lead)) if f <= 10)


# ---- the oracle against OptRef ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norms", os_.NORMS)
@pytest.mark.parametrize("live", os_.LIVE)
@pytest.mark.parametrize("version", os_.VERSIONS)
def test_the_oracle_is_optref_on_the_rule_fixtures(oracle, norms, live, version):
    leaf = os_.RuleLeaf(norms, live, version)
    ref = _ref(oracle, leaf)
    for name, q in os_.rule_queries().items():
        for k in os_.KS:
            for exact in (False, True):
                assert _same(os_.oracle_row(oracle, ref.osr, q, k, exact), ref.row(q, k, exact)), (name, k, exact)


@pytest.mark.parametrize("norms,live", [("rank", "none"), ("raw", "seeded"), ("none", "seeded")])
def test_the_oracle_is_optref_on_two_leaves(oracle, norms, live):
    a, b = os_.RuleLeaf(norms, live), os_.RuleLeaf(norms, live, which="B", doc_base=os_.R_MAX_DOC)
    osr = oracle.Searcher([a.oracle_segment(oracle), b.oracle_segment(oracle)])
    refs = [os_.OptRef(oracle, a, osr), os_.OptRef(oracle, b, osr)]
    for name, q in os_.rule_queries().items():
        for k in (10, 129, K_ALL):
            for exact in (False, True):
                assert _same(os_.oracle_row(oracle, osr, q, k, exact), os_.index_row(refs, q, k, exact)), (name, k, exact)


@pytest.mark.parametrize("norms,live,version", VARIANTS, ids=["%s-%s-v%d" % v for v in VARIANTS])
def test_the_oracle_is_optref_on_the_families(oracle, norms, live, version):
    """Every query of WITH_OPT and WITH_OPT_NOT and the ten-named-nine-present row: docs, score bits and totals, with the rule and with
    exact=True. The rows of ten or more optional scorers: totals and every skip decision (a wrong one moves a score by far more than
    the 1e-5 the heap order is allowed)."""
    leaf = as_.Leaf(norms, live, version)
    ref = _ref(oracle, leaf)
    for q in os_.ALL_OPT + [os_.TEN_ONE_ABSENT]:
        assert not os_.is_heap_order(leaf, q)
        for k in CPU_KS:
            for exact in (False, True):
                assert _same(os_.oracle_row(oracle, ref.osr, q, k, exact), ref.row(q, k, exact)), (q, k, exact)
    for q in (os_.TEN_PRESENT, os_.SIXTEEN):
        assert os_.is_heap_order(leaf, q)
        docs, final, skipped, req, opt, _ = ref.walk(q)
        od, osc, total = os_.oracle_row(oracle, ref.osr, q, docs.size + 1)
        assert total == docs.size and sorted(od.tolist()) == docs.tolist()
        mine = dict(zip(docs.tolist(), final.astype(np.float64).tolist()))
        assert all(abs(mine[d] - float(s)) <= 1e-5 * float(s) for d, s in zip(od.tolist(), osc.tolist()))
        assert (opt > 0.5 * req).all()                 # (every match holds optional clauses that weigh as much as the required ones)


def test_the_rule_decides_on_the_families(oracle):
    """The families reach the rule: rows where it skips some docs and not others, in every optional set's kind."""
    leaf = as_.Leaf()
    ref = _ref(oracle, leaf)
    both, only_kept = 0, 0
    for q in os_.ALL_OPT + os_.TEN:
        skipped = ref.walk(q)[2]
        both += int(skipped.any() and not skipped.all())
        only_kept += int(skipped.size > 101 and not skipped.any())
    assert both >= 40
    for q in os_.TEN:
        skipped = ref.walk(q)[2]
        assert skipped.sum() >= 20 and (~skipped).sum() >= 100, q
    assert sum(1 for t in os_.TEN_PRESENT.should if leaf.df(t)) == 10 and sum(1 for t in os_.TEN_ONE_ABSENT.should if leaf.df(t)) == 9
    assert len(os_.TEN_ONE_ABSENT.should) == 10 and sum(1 for t in os_.SIXTEEN.should if leaf.df(t)) == 16


# ---- the mutants ------------------------------------------------------------------------------------------------------------------
CAUGHT_BY = {"threshold 99": "S99", "threshold 101": "S101", ">= for >": "S100", "<= for <": "EQUAL", "state updated on a skip": "KEEPS_STATE",
             "state updated only with an optional hit": "OPT_MISS", "dead lead postings counted": "DEAD_ALL", "state reset every 64 records": "STEP_128",
             "state reset every item": "DF_257", "state carried across leaves": "TWO", "sum kept in f64": "F64"}


def test_every_mutant_changes_a_row(oracle):
    """Each mutant of walk_rule changes the row (k = 300: every doc's decision is in it) of the fixture named for it; the table of
    every fixture each mutant changes is printed. `state carried across leaves` shows on two leaves alone."""
    a, b = os_.RuleLeaf("rank", "seeded"), os_.RuleLeaf("rank", "seeded", which="B", doc_base=os_.R_MAX_DOC)
    osr = oracle.Searcher([a.oracle_segment(oracle), b.oracle_segment(oracle)])
    refs = [os_.OptRef(oracle, a, osr), os_.OptRef(oracle, b, osr)]
    assert set(CAUGHT_BY) == set(os_.MUTANTS)
    queries = os_.rule_queries()
    for mutant, flags in os_.MUTANTS.items():
        caught = [name for name, q in queries.items() if not _same(os_.index_row(refs, q, K_ALL), os_.index_row(refs, q, K_ALL, **flags))]
        print("%-42s %s" % (mutant, " ".join(caught)))
        assert CAUGHT_BY[mutant] in caught, (mutant, caught)
    # the three kinds of dead posting, each alone
    for name in ("DEAD_LACK", "DEAD_NOT", "DEAD_DEL"):
        assert not _same(os_.index_row(refs, queries[name], K_ALL), os_.index_row(refs, queries[name], K_ALL, count_dead=True)), name
    # the per-item reset at the item size the GPU test sets (and_blocks_per_item = 1: 128 records)
    one = os_.OptRef(oracle, a, osr)
    assert one.walk(queries["DF_257"], reset_records="item", blocks_per_item=1)[2].tolist() == [False] * 101 + [True] * 27 + [False] * 129


# ---- HAS_OPT at the edges of k_search_and -----------------------------------------------------------------------------------------
def test_optional_clauses_of_every_kind(oracle):
    leaf = as_.Leaf()
    kinds = {t: os_.opt_kind(leaf, t) for t in os_.OPT_KIND_TERMS}
    assert [kinds[t] for t in (C_511, C_512, C_1171, C_1172, C_2344, OVF_SMALL, OVF_CAP, OVF_OVER, SPREAD, EVERY)] == \
        ["walked", "walked", "walked", "bitmap", "nib", "bitmap", "nib", "walked", "walked", "nib"]
    assert leaf.kind(C_512) == leaf.kind(C_1171) == "memb"                       # what a MUST clause behind the lead would get
    assert all(os_.opt_kind(leaf, t, -1) == "walked" for t in os_.OPT_KIND_TERMS)
    assert [leaf.df(t) for t in (as_.SING_EVEN, as_.SING_ODD, as_.SING_MISS, ABSENT)] == [1, 1, 1, 0]
    used = {t for q in os_.WITH_OPT for t in q.should}
    assert set(os_.OPT_KIND_TERMS) <= used and set(os_.NINE) <= used and len(os_.NINE) == 9
    # behind every lead shape of PLAIN, and every set behind some lead
    assert {q.must for q in as_.PLAIN if len(q.must) + 9 <= 64} <= {q.must for q in os_.WITH_OPT}
    assert {q.should for q in os_.WITH_OPT} >= set(os_.OPT_SETS)
    # membership bits alone are never asked for on an optional clause's account: the rule looks at the MUST clauses
    for q in os_.WITH_OPT:
        if as_.wants_memb_only(leaf, Query(must=q.must)):
            assert as_.required(leaf, Query(must=q.must))[1][0] in q.must
    memb_opt = [q for q in os_.WITH_OPT if set(q.should) & {C_512, C_1171} and not as_.wants_memb_only(leaf, Query(must=q.must))]
    assert len(memb_opt) >= 4 and any(leaf.df(as_.lead_of(leaf, Query(must=q.must))) >= 128 for q in memb_opt)
    # freq 14 | 15 and the overflow freqs sit on docs the leads hold: the optional sum reads them
    core = as_.core_docs()
    assert leaf.has[CORE_LEAD][core[[30, 31, 20, 21, 40, 60, 100]]].all()
    # SPREAD under FP_LEAD: filter false positives as optional misses
    blk, hit, fp = as_.probe_outcomes(leaf, FP_LEAD, SPREAD)
    assert hit.sum() >= 70 and fp.sum() >= 60 and Query(must=(FP_LEAD,), should=(SPREAD,)) in os_.WITH_OPT
    # a term that is also a MUST clause, one term twice, the EQ orders
    assert any(set(q.must) & set(q.should) for q in os_.WITH_OPT) and (C_1172, C_1172) in os_.OPT_SETS
    ref = _ref(oracle, leaf)
    rows = [ref.row(Query(must=(CORE_LEAD,), should=s), 200) for s in os_.OPT_SETS[9:12]]
    bits = [dict(zip(r[0].tolist(), r[1].view(np.int32).tolist())) for r in rows]
    assert any(bits[0][d] != bits[1][d] or bits[1][d] != bits[2][d] for d in bits[0])   # the optional sum's order is the query's
    # the bitmaps a fresh segment builds for the families
    assert os_.bitmap_terms(leaf, os_.ALL_OPT)[1] == 1 and os_.bitmap_terms(leaf, os_.ALL_OPT, -1) == (0, 0)
    assert os_.bitmap_terms(leaf, [Query(must=(CORE_LEAD,), should=(C_1172,))]) == (1, 0) and os_.bitmap_terms(leaf, [Query(must=(CORE_LEAD,), should=(C_1171,))]) == (0, 0)


def test_the_survivor_queue_carries_optional_rows():
    """Under req_opt_rule = -1 the batched first probe runs with optional clauses behind it: the queue model names the rows."""
    leaf = as_.Leaf()
    rows = os_.queue_rows(leaf, os_.WITH_OPT)
    leads = {as_.lead_of(leaf, Query(must=os_.WITH_OPT[i].must)) for i in rows}
    assert {Q_LEAD, S_LEAD} | set(as_.G_LEADS) <= leads
    assert max(rows.values()) >= 639 and len(rows) >= 40
    assert os_.queue_rows(leaf, os_.WITH_OPT, -1) == {}
    assert len(os_.queue_rows(leaf, os_.WITH_OPT_NOT)) >= 10


def test_the_nested_rows_cover_what_they_name():
    leaf = as_.Leaf()
    n = os_.NESTED
    assert {r.is_or for r in n} == {True, False} and {r.at for r in n if len(r.musts) == 3} == {0, 1, 2, 3} and {r.at for r in n if len(r.musts) == 1} == {0, 1}
    assert all(0 <= r.at <= len(r.musts) and 1 <= len(r.inner) <= 9 for r in n) and any(r.nots for r in n) and any(len(r.inner) == 9 for r in n)
    kinds = {leaf.kind(t) for r in n for t in r.inner if leaf.df(t) > 1}
    assert kinds == {"walked", "memb", "bitmap", "nib"} and any(ABSENT in r.inner for r in n) and any(as_.SING_MISS in r.inner for r in n)
    # c1_nested: one MUST clause that leads, a nested conjunction of bitmap clauses right behind it
    c1 = [r for r in n if not r.is_or and r.musts == (Q_LEAD,)]
    assert c1 and all(leaf.kind(t) in ("bitmap", "nib") for t in c1[0].inner) and leaf.df(Q_LEAD) < min(leaf.df(t) for t in c1[0].inner)
    # need_any: candidates that no clause of the nested disjunction holds
    na = [r for r in n if r.is_or and r.musts == (EDGE_LEAD,)][0]
    neigh = as_.neigh_docs()
    assert leaf.has[EDGE_LEAD][neigh].all() and not any(leaf.has[t][neigh].any() for t in na.inner)


def test_the_heap_order_rule_for_required_plus_optional_rows(oracle):
    """oracle/parity.py check_heap_order_opt_row: OptRef's clause-order rows of ten and sixteen optional clauses pass it against the
    oracle's complete heap-order rows; a row with one skip decision turned, a missing hit, a foreign doc or a wrong total does not."""
    from oracle import parity
    leaf = as_.Leaf()
    ref = _ref(oracle, leaf)
    for q in (os_.TEN_PRESENT, os_.SIXTEEN):
        docs, final, skipped, req, opt, _ = ref.walk(q)
        full = os_.oracle_row(oracle, ref.osr, q, docs.size + 1)
        assert not _same(full, ref.row(q, docs.size + 1)) or q is os_.SIXTEEN          # heap order and clause order really differ in bits
        for k in (10, 129, 300):
            d, sc, total = ref.row(q, k)
            row = np.zeros(k, dtype=[("doc", np.int32), ("score", np.float32)])
            row["doc"] = -1
            row["doc"][:d.size], row["score"][:d.size] = d, sc
            assert parity.check_heap_order_opt_row(full[0], full[1], row["doc"], row["score"], total, k) == 0
            with pytest.raises(parity.HeapOrderParityError):
                parity.check_heap_order_opt_row(full[0], full[1], row["doc"], row["score"], total + 1, k)
            turned = row.copy()
            i = int(np.flatnonzero(~skipped[np.searchsorted(docs, d)])[-1])            # the lowest doc that took the optional sum: leave it out
            turned["score"][i] = req[np.searchsorted(docs, d[i])]
            with pytest.raises(parity.HeapOrderParityError):
                parity.check_heap_order_opt_row(full[0], full[1], turned["doc"], turned["score"], total, k)
            foreign = row.copy()
            foreign["doc"][0] = 7                                                       # SING_MISS's doc: in no CORE list
            with pytest.raises(parity.HeapOrderParityError):
                parity.check_heap_order_opt_row(full[0], full[1], foreign["doc"], foreign["score"], total, k)
