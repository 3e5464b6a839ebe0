"""Fixtures and the reference for MUST + SHOULD trees with exact PhraseQuery clauses on either side (+a +b "a b", +"a b" c,
+"a b" +c "b c" d -n #f: rgpu_search_phrase_opt_batch). Plain Python / numpy; tests/test_phrase_opt_cpu.py proves them,
tests/test_gpu_phrase_opt.py runs them on the device.

The reference is composed from the helpers of tests/phrase_bool.py and tests/opt_spectrum.py, none of them changed:
  * the required side: phrase_bool.Index.clause_scores per clause, intersected; the f32 sum in the leaf's stable cost order
    (cost_order, sum_in_order). For the docs that are hits the sum is leaf_rows' (asserted bit for bit); a doc that holds every
    required clause but is deleted or held by a MUST_NOT clause is a DEAD record: it keeps its place in the stream and must not move
    the rule's state;
  * the optional side: 0.0f + s_i ... in np.float32 over the optional clauses that exist in the leaf and hold the doc, in clause order;
  * the rule: opt_spectrum.walk_rule over the leaf's records in doc order, a fresh state per leaf, with its mutant flags.
`exact=True` is rgpu_config.req_opt_rule = -1: req + opt wherever an optional clause holds the doc.

Fixtures: phrase_bool.main() (700 docs), groups() (400 docs) and leaves() as they are, and
  join()   700 docs. X, Y as in groups() (docs 0..299). Required leads R63 .. R129 (63, 64, 65, 127, 128, 129 docs from doc 300 on),
           optional terms O1 (the singleton doc 310), O63 / O64 / O65 (every second doc from 300 on: a required odd doc lies between two
           neighbouring optional entries), BEFORE (docs 200..250: wholly in front of the required docs), BEHIND (500..550), ENDS (300
           and 362: R63's first and last doc), ZERO (in no doc).
  rule()   leaf A, 700 docs: X at 1 and Y at 2 in EVERY doc (the optional phrase "X Y" holds every doc, the skipped ones too). Lead
           terms at three (freq, norm byte) levels - HIGH (10, 124), LOW (1, 100), MID (4, 112) - S99 / S100 / S101: 99 | 100 | 101
           HIGH docs, then 20 LOW: the 100th | 101st | 102nd scored doc in front of a LOW one; DEAD: 100 HIGH with a dead doc (HIGH too) behind
           every fourth (deleted, or held by BAN, in turn), then 20 LOW: the first LOW is the 101st scored doc and still takes the
           optional sum; KEEP: 101 HIGH, 30 LOW (skipped), 3 MID (skipped: 2 * MID is under HIGH, and the LOWs never entered the mean -
           had they, it would have sunk below 2 * MID), 2 HIGH. OPT60: every second doc of S101's range (61 docs: an optional term the oracle can walk).
           Leaf B (same docs): S101's range reads 5 LOW, 105 HIGH, 10 LOW - its scorer is fresh.
  equal()  200 docs, fixed statistics: the lead EQ ends its first 101 docs in a state whose mean is exactly twice the 102nd doc's score."""
import collections

import numpy as np

import opt_spectrum as osp
import phrase_bool as pb
import phrase_rescore as pr
from phrase_bool import Ph

f32 = np.float32
UNSUPPORTED, ILLEGAL_ARGUMENT, ILLEGAL_STATE = -5, -2, -1
CANDIDATES = "k_search_and(phrase-opt candidates)"
JOIN, SCAN, SEED, SCORE, FANOUT = "k_req_opt_join", "k_req_opt_scan", "k_phrase_opt_seed", "k_phrase_bool_score", "k_phrase_bool_fanout"


class Q(pb.Q):
    """musts / filters / shoulds: term ids (int) and Ph clauses, in query order; must_nots: term ids."""

    def __init__(self, musts, shoulds, must_nots=(), filters=(), name="", msm=0):
        pb.Q.__init__(self, musts, must_nots, filters, name)
        self.shoulds, self.msm = list(shoulds), msm

    def req(self):
        """the required side as a tests/phrase_bool.py query"""
        return pb.Q(self.musts, self.must_nots, self.filters, self.name)

    def has_phrase(self):
        return any(isinstance(c, Ph) for c in self.musts + self.filters + self.shoulds)

    def build(self):
        import rucene_amd
        T, B, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery

        def mk(c):
            return P(c.terms, c.positions, boost=c.boost) if isinstance(c, Ph) else T(c)
        return B.build([mk(c) for c in self.musts], [mk(c) for c in self.shoulds], filters=[mk(c) for c in self.filters],
                       must_nots=[T(t) for t in self.must_nots], min_should_match=self.msm)

    def __repr__(self):
        return "Q(%s+%r ?%r -%r #%r)" % (self.name + ": " if self.name else "", self.musts, self.shoulds, self.must_nots, self.filters)


def present(fx, q):
    """the optional clauses that exist in the leaf, in clause order"""
    return [c for c in q.shoulds if pb.clause_cost(fx, c) > 0]


def leaf_records(ix, li, q, opt_order=None):
    """[(local doc, match, req, opt, opt_hit)] in doc order: every doc of leaf li that holds every required clause. opt_order: indexes
    into present() (default: clause order)."""
    fx = ix.fxs[li]
    req = q.required()
    if any(pb.clause_cost(fx, c) == 0 for c, _ in req):
        return []
    per = [ix.clause_scores(li, c, scoring) for c, scoring in req]
    docs = set(per[0])
    for p in per[1:]:
        docs &= set(p)
    order = pb.cost_order(fx, q)
    hits = ix.leaf_rows(li, q.req())
    opts = [ix.clause_scores(li, c) for c in present(fx, q)]
    if opt_order is not None:
        opts = [opts[i] for i in opt_order]
    recs = []
    for d in sorted(docs):
        r = pb.sum_in_order([per[i][d] for i in order])
        match = d + ix.bases[li] in hits
        if match:
            assert f32(r).view(np.uint32) == f32(hits[d + ix.bases[li]]).view(np.uint32)
        opt, hit = f32(0.0), False
        for scores in opts:
            if d in scores:
                opt, hit = f32(opt + f32(scores[d])), True
        recs.append((d, match, f32(r), opt, hit))
    assert sum(m for _, m, _, _, _ in recs) == len(hits)
    return recs


def leaf_rows(ix, li, q, exact=False, state=None, trace=None, opt_order=None, **flags):
    """-> ({global doc: f32 final score} of leaf li, the rule's state afterwards)"""
    recs = leaf_records(ix, li, q, opt_order)
    final, _skipped, st = osp.walk_rule([(m, r, o, h) for _, m, r, o, h in recs], exact=exact, state=state, trace=trace, **flags)
    return {d + ix.bases[li]: f32(final[i]) for i, (d, m, _, _, _) in enumerate(recs) if m}, st


def rows(ix, q, exact=False, carry=False, **flags):
    """-> (docs, scores) of every hit, canonical order. carry: the mutant that keeps the rule's state from leaf to leaf."""
    scored, st = {}, None
    for li in range(len(ix.fxs)):
        part, after = leaf_rows(ix, li, q, exact=exact, state=st if carry else None, **flags)
        st = after
        scored.update(part)
    return pb.rank(scored)


def traces(ix, q):
    """the rule's decisions per leaf: [(record, num, mean, 2 * req)]"""
    out = []
    for li in range(len(ix.fxs)):
        t = []
        leaf_rows(ix, li, q, trace=t)
        out.append(t)
    return out


def skipped_docs(ix, q):
    """global docs the rule skips (they score `req` alone)"""
    out = []
    for li in range(len(ix.fxs)):
        recs = leaf_records(ix, li, q)
        _f, skipped, _s = osp.walk_rule([(m, r, o, h) for _, m, r, o, h in recs])
        out += [recs[i][0] + ix.bases[li] for i in np.flatnonzero(skipped)]
    return out


# ---- queries over phrase_bool.main() ------------------------------------------------------------------------------------------------
PA, PB, PC, S, R20, T40, T129, D600, N1, N2, N3, ABSENT, R30 = range(13)
AB, BC, ABC, ABA, GAP = pb.AB, pb.BC, pb.ABC, pb.ABA, pb.GAP
AB0 = Ph((PA, PB), None, 0.0)
DEAD_PHRASE = Ph((PA, ABSENT))
SHAPES = [
    Q([T129], [AB], name='+t "a b"'),
    Q([PA, PB], [AB], name='+a +b "a b"'),
    Q([AB], [T40], name='+"a b" c'),
    Q([AB, D600], [BC, T129], [N1], [T40], name='+"a b" +c "b c" d -n #f'),
    Q([], [T129], filters=[AB], name='#"a b" c'),
    Q([D600], [AB, T40, R20], name="optional phrase first"),
    Q([D600], [T40, AB, R20], name="optional phrase in the middle"),
    Q([D600], [T40, R20, AB], name="optional phrase last"),
    Q([AB, BC], [T40], name="two required phrases"),
    Q([AB, BC, ABC, GAP], [D600], name="four required phrases"),
    Q([D600], [AB, BC], name="two optional phrases"),
    Q([PB], [AB, BC, ABC, GAP], name="four optional phrases"),
    Q([AB, BC], [ABC, GAP, R30], name="two phrases on each side"),
    Q([PB], [ABA], name="optional repeated-term phrase"),
    Q([D600], [GAP], name="optional gapped phrase"),
    Q([T129, AB], [T129], name="the same term required and optional"),
    Q([AB], [AB], name="the same phrase required and optional"),
    Q([D600], [AB0, T40], name="optional phrase of weight 0"),
    Q([D600], [S, AB], name="optional singleton"),
]
PRESENCE = [
    Q([AB, D600], [ABSENT, T40], name="an absent optional term"),
    Q([AB, D600], [DEAD_PHRASE, T40], name="an optional phrase lacking a term"),
    Q([AB, D600], [ABSENT, DEAD_PHRASE], name="every optional clause absent"),
    Q([AB, ABSENT], [T40], name="an absent required term"),
    Q([DEAD_PHRASE, D600], [T40], name="a required phrase lacking a term"),
    Q([AB, D600], [T40], [ABSENT], name="MUST_NOT absent"),
    Q([AB, D600], [T40], [N1, N3], name="MUST_NOT present"),
]
NINE = Q([D600], [T40, R20, R30, T129, S, PC, PB, PA, AB], name="nine optional clauses")
TEN = Q([D600], [T40, R20, R30, T129, S, PC, PB, PA, AB, N1], name="ten optional clauses")
MAIN_QUERIES = SHAPES + PRESENCE + [NINE]
# three optional addends (their f32 sum depends on the order) beside a required sum whose cost order differs between two leaves
ARITH = Q([T129, AB, D600], [T40, R30, PC], name="three optional addends")
LEAF_QUERIES = [ARITH, Q([R20, AB], [BC, T40], name="a leaf without the MUST term"), Q([AB, D600], [BC, R20], [N1], [T40], name="the full tree over three leaves")]
# (PHRASELESS_WALKED: every clause the oracle's scorers would advance() has fewer than 128 docs - the oracle's plain Segment does not
# parse a positions field's skip data, tests/phrase_bool.py - so its own ReqOptScorer can be asked about them)
PHRASELESS_WALKED = [Q([T129], [T40], name="+t u"), Q([T40, R30], [R20, S], [N1], name="+t +u v w -n"), Q([T40], [ABSENT], name="+t absent"),
                     Q([ABSENT], [T40], name="+absent u"), Q([S], [T40], name="+singleton u"), Q([R30, T40], [R20, T40, R30], name="+t +u v t u")]
PHRASELESS = PHRASELESS_WALKED + [Q([T129, D600], [T40, R30], [N1], name="+t +dense v w -n"), Q([D600], [T129], filters=[T40], name="+t #f u"),
                                  Q([S], [D600], name="+singleton dense")]

# ---- queries over phrase_bool.groups() ----------------------------------------------------------------------------------------------
X, Y, L63, L64, L65, L192, LZ, LK = range(8)
XY = pb.XY
GROUP_QUERIES = [Q([L63], [XY], name="63 required, optional phrase"), Q([L64], [XY], name="64 required, optional phrase"),
                 Q([L65], [XY], name="65 required, optional phrase"), Q([XY, L192], [L63, L64], name="required phrase, a group without survivors"),
                 Q([XY], [LZ], name="optional run behind every required doc"), Q([XY, LK], [L65], name="236 hits"),
                 Q([LZ], [XY], name="no optional doc among the required")]

# ---- join() -------------------------------------------------------------------------------------------------------------------------
JX, JY, R63, R64, R65, R127, R128, R129, O1, O63, O64, O65, BEFORE, BEHIND, ENDS, ZERO = range(16)
JOIN_DOCS, JOIN_TERMS = 700, 16
JXY = Ph((JX, JY))


def join():
    if "po-join" not in pr._built:
        h = {}
        for d in range(300):
            h[d] = {JX: [1, 5] if d % 9 == 0 else [1], JY: ([2, 6] if d % 9 == 0 else [2]) if pb._xy_matches(d) else [3]}
        lists = ((R63, range(300, 363)), (R64, range(300, 364)), (R65, range(300, 365)), (R127, range(300, 427)), (R128, range(300, 428)),
                 (R129, range(300, 429)), (O1, [310]), (O63, range(300, 426, 2)), (O64, range(300, 428, 2)), (O65, range(300, 430, 2)),
                 (BEFORE, range(200, 251)), (BEHIND, range(500, 551)), (ENDS, [300, 362]))
        for t, docs in lists:
            for d in docs:
                h.setdefault(d, {})[t] = [9] if d % 4 else [9, 10]
        fx = pr.Fixture("po-join", JOIN_DOCS, JOIN_TERMS, h, 31)
        assert [len(fx.postings[t]) for t in (R63, R64, R65, R127, R128, R129, O1, O63, O64, O65, ZERO)] == [63, 64, 65, 127, 128, 129, 1, 63, 64, 65, 0]
        pr._built["po-join"] = fx
    return pr._built["po-join"]


JOIN_QUERIES = ([Q([r], [o], name="required %d x optional %d" % (r, o)) for r in (R63, R64, R65, R127, R128, R129) for o in (O63, O65)] +
                [Q([R64], [O64], name="64 x 64"), Q([R129], [ZERO], name="optional run of 0"), Q([R129], [O1], name="optional run of 1"),
                 Q([R63], [ENDS], name="first and last entry"), Q([R65], [BEFORE], name="wholly before"), Q([R65], [BEHIND], name="wholly behind"),
                 Q([R128], [BEFORE, O63, ZERO, O1, ENDS, BEHIND, O64, O65], name="eight runs"),
                 Q([R129], [JXY, O65], name="optional phrase wholly before"), Q([JXY], [R63, BEFORE], name="required phrase, term run partly before")])


# ---- rule() -------------------------------------------------------------------------------------------------------------------------
RX, RY, S99, S100, S101, DEAD, KEEP, BAN, EVERY, OPT60 = range(10)
RULE_DOCS, RULE_TERMS = 700, 10
RXY = Ph((RX, RY))
HIGH, LOW, MID = (10, 124), (1, 100), (4, 112)
RULE_FIRST = {S99: 1, S100: 125, S101: 250, DEAD: 375, KEEP: 520}
DEAD_DELETED, DEAD_BANNED = [], []


def _seq(which):
    run = osp._run
    seqs = collections.OrderedDict()
    for t, n in ((S99, 99), (S100, 100), (S101, 101)):
        seqs[t] = run(HIGH, n) + run(LOW, 20)
    if which == "B":
        seqs[S101] = run(LOW, 5) + run(HIGH, 105) + run(LOW, 10)
    dead, j = [], 0
    for i in range(100):
        dead.append(osp.Post(*HIGH))
        if i % 4 == 3:
            dead.append(osp.Post(HIGH[0], HIGH[1], ("del", "not")[j % 2]))
            j += 1
    seqs[DEAD] = dead + run(LOW, 20)
    seqs[KEEP] = run(HIGH, 101) + run(LOW, 30) + run(MID, 3) + run(HIGH, 2)
    return seqs


def rule(which="A"):
    """-> (fixture, deleted docs)"""
    key = "po-rule-" + which
    if key not in pr._built:
        h = {d: {RX: [1], RY: [2], EVERY: [3]} for d in range(RULE_DOCS)}
        byte, deleted, banned = {}, [], []
        for t, posts in _seq(which).items():
            for i, p in enumerate(posts):
                d = RULE_FIRST[t] + i
                h[d][t] = list(range(20, 20 + p.freq))
                byte[d] = p.byte
                if p.dead == "del":
                    deleted.append(d)
                if p.dead == "not":
                    banned.append(d)
        for d in banned + [699]:
            h[d][BAN] = [60]
        for d in range(RULE_FIRST[S101], RULE_FIRST[S101] + 121, 2):
            h[d][OPT60] = [61]
        fx = pr.Fixture(key, RULE_DOCS, RULE_TERMS, h, 41)
        fx.norms[:] = 118
        for d, b in byte.items():
            fx.norms[d] = b
        pr._built[key] = (fx, deleted)
    return pr._built[key]


RULE_QUERIES = collections.OrderedDict([
    ("S99", Q([S99], [RXY], name="S99")), ("S100", Q([S100], [RXY], name="S100")), ("S101", Q([S101], [RXY], name="S101")),
    ("DEAD", Q([DEAD], [RXY], [BAN], name="DEAD")), ("KEEP", Q([KEEP], [RXY, EVERY], name="KEEP")),
    ("REQ_PHRASE", Q([S101], [EVERY], filters=[RXY], name="REQ_PHRASE")),
])
RULE_PHRASELESS = Q([S101], [OPT60], name="S101 without a phrase")

# ---- equal() ------------------------------------------------------------------------------------------------------------------------
# A leaf of its own, 200 docs, for the one edge no level of rule() can show: a doc whose doubled required score IS the f32 mean, which
# the strict `<` does not skip and a `<=` would. Its statistics are fixed (sum_total_term_freq = 40 * max_doc whatever the holdings),
# so that the (freq, norm byte) levels opt_spectrum.equal_search found for a lead of 112 docs stay right: EQ reads (1, 116) 40 times,
# (9, 138) 61 times, then the doc (2, 110), then 10 LOW. tests/test_phrase_opt_cpu.py checks the equality in walk_rule's trace.
EX, EY, EQ = range(3)
EQUAL_DOCS, EQUAL_DF, EQUAL_STTF_PER_DOC = 200, 112, 40
EQUAL_FOUND = ((1, 116), 40, (9, 138), (2, 110))
EXY = Ph((EX, EY))
EQUAL_QUERY = Q([EQ], [EXY], name="EQUAL")
EQUAL_DOC = 1 + 101


def equal():
    if "po-equal" not in pr._built:
        first, n, second, doc = EQUAL_FOUND
        posts = osp._run(first, n) + osp._run(second, 101 - n) + [osp.Post(*doc)] + osp._run(LOW, EQUAL_DF - 102)
        h = {d: {EX: [1], EY: [2]} for d in range(EQUAL_DOCS)}
        for i, p in enumerate(posts):
            h[1 + i][EQ] = list(range(20, 20 + p.freq))
        fx = pr.Fixture("po-equal", EQUAL_DOCS, 3, h, 61)
        fx.norms[:] = 118
        for i, p in enumerate(posts):
            fx.norms[1 + i] = p.byte
        fx.sum_ttf = EQUAL_STTF_PER_DOC * EQUAL_DOCS
        assert len(fx.postings[EQ]) == EQUAL_DF and fx.doc_count == EQUAL_DOCS
        pr._built["po-equal"] = fx
    return pr._built["po-equal"]
