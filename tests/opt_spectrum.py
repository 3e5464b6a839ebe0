"""Fixtures for MUST + SHOULD trees (plain Python, no GPU): k_search_and<..., HAS_OPT> and the sequential scan k_req_opt_scan of
rucene_amd/csrc/kernels/search_and.hpp, which serve "+a b" (ReqOptScorer), "+a +(b c)" (RGPU_OP_SHOULD_REQUIRED) and "+a +(+b +c)"
(RGPU_OP_NESTED_MUST); an independent reference (OptRef) and one model per mistake the scan could make (MUTANTS).

ReqOptScorer::score (req_opt_scorer.rs:41-66) carries an f32 sum and a count of the required scores from doc to doc: once MORE than
100 docs were scored, a doc whose required score, doubled, is below the mean returns the required score alone and leaves the state
as it was. The rule's edges are sequences, so they get a leaf of their own (RuleLeaf, 4099 docs), in which every sequence is a lead
term over a doc range of its own. A doc's level comes from a (freq, norm byte) pair of that term alone:

  HIGH (40, 124), LOW (1, 104), MID (1, 110): 2 * LOW < mean <= 2 * HIGH in every state the sequences reach; MID is skipped while the
  mean is HIGH's and is not once a run of LOWs has entered it. Without norms a posting of freq 1 scores weight * 1.0 whatever
  the byte (LOW = MID there) and one of freq 40 weight * 2.136: the same decisions. Dead lead postings carry HIGH.

  ALL, THIRD, HOLD, BAN   every doc (the optional term: each doc that is not skipped visibly carries its score); every third doc;
                          every doc but the "lack" postings (a second MUST clause); the "not" postings (a MUST_NOT clause)
  S99, S100, S101         99 | 100 | 101 HIGH, then 20 LOW: two | one | none of the LOWs take the optional sum
  KEEPS_STATE             101 HIGH, 120 LOW (all skipped), 3 MID (skipped: the LOWs never entered the mean), 2 HIGH
  DEAD_LACK, DEAD_NOT,    S100 with a dead lead posting behind every fourth HIGH one - docs HOLD lacks | docs BAN holds | docs deleted
  DEAD_DEL, DEAD_ALL      under live = "seeded" | the three kinds in turn: the first LOW still takes the optional sum
  OPT_MISS                S100's lead with THIRD as the optional term: docs THIRD lacks still enter sum and count
  STEP_127 .. STEP_193    BAN postings in front so that the 101st scored match is lead record 127 | 128 | 129 (the scan loads 64 records
                          a step, a lead block is 128 records, a lane of k_search_and writes two) and 191 | 192 | 193 (record 63 | 64 |
                          65 of the second block; a record index below 100 cannot hold the 101st match), then 10 LOW: all skipped
  DF_1 .. DF_257          lead doc_freq 1 (a singleton: TERM + SHOULD), 2, 127 (a VInt tail alone), 128 (one FullBlock and nothing), 129
                          and 257: the `ord + 1 < L.df` edge of the record writer
  EQUAL                   (2, 100) 89 times, (6, 130) 12 times, then a doc (3, 101) for which 2 * req == sum / num exactly in f32 - the
                          strict `<` does not skip it -, found by equal_search() over 256 norm bytes x freqs 1..10; then 10 LOW
  F64                     HIGH 67 times, (1, 93) 34 times, then a doc (10, 103) whose doubled score lies between the mean of the f32
                          sum and that of an f64 sum (f64_search()); then 10 LOW. Both hold with norms alone ("rank", "raw")
  TWO                     leaf A: S101; leaf B (RuleLeaf("B"), searched behind A): 5 LOW, 105 HIGH, 10 LOW - B's scorer is fresh: its
                          first 101 scored docs take the optional sum

On and_spectrum.Leaf (300 007 docs) the family WITH_OPT gives every PLAIN conjunction an optional set, dealt in turn, so that an
optional clause of every kind the probe tells apart - walked, the membership-only range (never built for an optional clause: the
host asks for it for the second cheapest MUST clause alone - such a clause is walked), bitmap, four-bit array with freq 14 | 15,
overflow lists, singletons that hit and miss, ABSENT alone and beside a present term, SPREAD under FP_LEAD, EVERY, a term that is
also a MUST clause, a term twice, EQ_* in three orders, nine clauses - stands behind every lead shape, the survivor queue's
(Q_LEAD, S_LEAD, G_*) included; WITH_OPT_NOT adds MUST_NOT clauses; TEN holds rows of ten, ten-with-one-ABSENT and sixteen
optional clauses; NESTED the "+a +(b c)" / "+a +(+b +c)" trees.

tests/test_opt_spectrum_cpu.py proves every property named here, OptRef against the oracle, and that every mutant changes a row."""
import collections

import numpy as np

import and_spectrum as as_
import segment_spectrum as ss
from and_spectrum import (ABSENT, C_511, C_512, C_1171, C_1172, C_2343, C_2344, CORE_LEAD, EDGE_LEAD, EQ_A, EQ_B, EQ_C, EVERY, FP_LEAD, HALF_B, HALF_N,
                          OVF_CAP, OVF_OVER, OVF_SMALL, Q_C1, Q_LEAD, REG4, S_C1, S_LEAD, SING_EVEN, SING_MISS, SING_ODD, SPREAD, SPREAD_NOTAIL)
from segment_spectrum import Query

THRESHOLD = 100          # OPT_SCORE_THRESHOLD / REQ_OPT_THRESHOLD
SCAN_STEP = 64           # records k_req_opt_scan loads per step
BLOCK = 128
WG_WAVES = 4             # the scan runs one wavefront per query, four to a workgroup
KS = (1, 10, 64, 65, 128, 129, 300)
NORMS = ("rank", "raw", "none")
LIVE = ("none", "seeded")
VERSIONS = (1, 0)
R_MAX_DOC = 4099
STTF_PER_DOC = 60

HIGH, LOW, MID = (40, 124), (1, 104), (1, 110)
FILL_BYTE = 112

Post = collections.namedtuple("Post", "freq byte dead", defaults=(None,))    # dead: None | "lack" | "not" | "del"


def _run(level, n, dead=None):
    return [Post(level[0], level[1], dead)] * n


def _dead_interleaved(kinds):
    """S100 with a dead lead posting (HIGH) behind every fourth HIGH one, of the kinds given in turn."""
    out, j = [], 0
    for i in range(100):
        out.append(Post(*HIGH))
        if i % 4 == 3:
            out.append(Post(HIGH[0], HIGH[1], kinds[j % len(kinds)]))
            j += 1
    return out + _run(LOW, 20)


STEP_AT = (127, 128, 129, 191, 192, 193)
DF_SIZES = (1, 2, 127, 128, 129, 257)
# found by equal_search() / f64_search() (tests/test_opt_spectrum_cpu.py runs both again) for a lead of SEARCHED_DF docs:
# (the level of the first n docs, n, the level of the other 101 - n, the level of the doc that follows them)
SEARCHED_DF = 112
EQUAL_FOUND = ((2, 100), 89, (6, 130), (3, 101))
F64_FOUND = ((40, 124), 67, (1, 93), (10, 103))


def _sequences(which="A"):
    seqs = collections.OrderedDict()
    for n in (99, 100, 101):
        seqs["S%d" % n] = _run(HIGH, n) + _run(LOW, 20)
    seqs["KEEPS_STATE"] = _run(HIGH, 101) + _run(LOW, 120) + _run(MID, 3) + _run(HIGH, 2)
    seqs["DEAD_LACK"] = _dead_interleaved(["lack"])
    seqs["DEAD_NOT"] = _dead_interleaved(["not"])
    seqs["DEAD_DEL"] = _dead_interleaved(["del"])
    seqs["DEAD_ALL"] = _dead_interleaved(["lack", "not", "del"])
    for at in STEP_AT:
        seqs["STEP_%d" % at] = _run(HIGH, at - THRESHOLD, "not") + _run(HIGH, 101) + _run(LOW, 10)
    for df in DF_SIZES:
        seqs["DF_%d" % df] = (_run(HIGH, 101) + _run(LOW, 100) + _run(MID, 10) + _run(HIGH, 46))[:df]
    for name, found in (("EQUAL", EQUAL_FOUND), ("F64", F64_FOUND)):
        if found is not None:
            first, n, second, doc = found
            seqs[name] = _run(first, n) + _run(second, 101 - n) + [Post(*doc)] + _run(LOW, SEARCHED_DF - 102)
    two = _run(HIGH, 101) + _run(LOW, 20) if which == "A" else _run(LOW, 5) + _run(HIGH, 105) + _run(LOW, 10)
    seqs["TWO"] = two + [None] * (121 - len(two))      # (the same doc range in both leaves)
    return seqs


R_FIXED = ["ALL", "THIRD", "HOLD", "BAN"]
R_ALL, R_THIRD, R_HOLD, R_BAN = range(4)
R_NAMES = R_FIXED + list(_sequences())
R_TERM = {name: i for i, name in enumerate(R_NAMES)}


def rule_query(name):
    """The query a sequence is searched with."""
    t = R_TERM[name]
    if name == "DEAD_LACK":
        return Query(must=(t, R_HOLD), should=(R_ALL,))
    if name == "DEAD_ALL":
        return Query(must=(t, R_HOLD), should=(R_ALL,), must_not=(R_BAN,))
    if name == "DEAD_NOT" or name.startswith("STEP_"):
        return Query(must=(t,), should=(R_ALL,), must_not=(R_BAN,))
    return Query(must=(t,), should=(R_ALL,))


RULE_NAMES = [n for n in R_NAMES[len(R_FIXED):]] + ["OPT_MISS"]


def rule_queries():
    """{fixture name: query} over RuleLeaf."""
    out = collections.OrderedDict((n, rule_query(n)) for n in R_NAMES[len(R_FIXED):])
    out["OPT_MISS"] = Query(must=(R_TERM["S100"],), should=(R_THIRD,))
    return out


_rule_built = {}


class RuleLeaf:
    """The rule fixtures' leaf, with the attributes and_spectrum.Leaf has. which = "B": TWO's other sequence, for the two-leaf index."""

    def __init__(self, norms="rank", live="none", version=1, which="A", doc_base=0):
        assert norms in NORMS and live in LIVE and version in VERSIONS and which in "AB"
        key = (which, norms, version)
        if key not in _rule_built:
            _rule_built[key] = self._build(which, norms, version)
        self.lists, self.norms, self.seg, self.has, self.posts, self.first = _rule_built[key]
        self.key = ("rule",) + key + (live, doc_base)
        self.max_doc, self.norms_kind, self.live, self.version, self.doc_base, self.sttf = R_MAX_DOC, norms, live, version, doc_base, STTF_PER_DOC * R_MAX_DOC
        self.big = False
        self.alive = np.ones(R_MAX_DOC, bool)
        if live == "seeded":
            used = max(self.first[n] + len(p) for n, p in self.posts.items())
            self.alive[used:] = np.random.default_rng([R_MAX_DOC, 13]).random(R_MAX_DOC - used) < 0.85     # the background alone, at random ...
            for name, posts in self.posts.items():                                                             # ... and the postings named "del"
                for i, p in enumerate(posts):
                    if p is not None and p.dead == "del":
                        self.alive[self.first[name] + i] = False
        self.live_docs = None if live == "none" else ss.live_words(self.alive)

    @staticmethod
    def _build(which, norms, version):
        from rucene_amd import indexgen
        seqs = _sequences(which)
        nb = np.full(R_MAX_DOC, FILL_BYTE, np.uint8)
        lists, first, at = [None] * len(R_NAMES), {}, 1
        lack, ban = [], []
        for name, posts in seqs.items():
            first[name] = at
            docs = [at + i for i, p in enumerate(posts) if p is not None]
            for i, p in enumerate(posts):
                if p is None:
                    continue
                nb[at + i] = p.byte
                if p.dead == "lack":
                    lack.append(at + i)
                if p.dead == "not":
                    ban.append(at + i)
            lists[R_TERM[name]] = (np.array(docs, np.int32), np.array([p.freq for p in posts if p is not None], np.int32))
            at += len(posts) + 3
        assert at + as_.RAW_BYTES.size + 40 <= R_MAX_DOC, at
        if norms == "raw":
            nb[at:at + as_.RAW_BYTES.size] = as_.RAW_BYTES        # 65 or more distinct bytes: raw mode
        every = np.arange(R_MAX_DOC, dtype=np.int32)
        one = lambda d: (np.asarray(d, np.int32), np.ones(len(d), np.int32))   # noqa: E731
        lists[R_ALL] = one(every)
        lists[R_THIRD] = one(every[::3])
        lists[R_HOLD] = one(np.setdiff1d(every, lack))
        lists[R_BAN] = one(sorted(ban + [at + 5, at + 9, R_MAX_DOC - 1]))
        norms_arr = None if norms == "none" else nb
        seg = indexgen.build_explicit(R_MAX_DOC, lists, norms=norms_arr, version=version)
        assert [int(x) for x in seg.terms["doc_freq"]] == [d.size for d, _ in lists]
        has = np.zeros((len(lists), R_MAX_DOC), bool)
        for t, (d, _) in enumerate(lists):
            has[t, d] = True
        return lists, norms_arr, seg, has, seqs, first

    def oracle_segment(self, oracle):
        return oracle.Segment(self.seg.doc_bytes, self.norms, self.max_doc, self.seg.terms, doc_base=self.doc_base, live_docs=self.live_docs,
                              sum_total_term_freq=self.sttf)

    def df(self, t):
        return int(self.lists[t][0].size)

    def docs_of_level(self, name, level, dead=None):
        """Local doc ids of the sequence's postings of one level."""
        return np.array([self.first[name] + i for i, p in enumerate(self.posts[name]) if p is not None and (p.freq, p.byte) == level and p.dead == dead], np.int64)


# ---- the reference ------------------------------------------------------------------------------------------------------------------
MUTANTS = collections.OrderedDict([
    ("threshold 99", dict(threshold=99)), ("threshold 101", dict(threshold=101)), (">= for >", dict(ge=True)), ("<= for <", dict(le=True)),
    ("state updated on a skip", dict(update_on_skip=True)), ("state updated only with an optional hit", dict(only_with_opt=True)),
    ("dead lead postings counted", dict(count_dead=True)), ("state reset every 64 records", dict(reset_records=SCAN_STEP)),
    ("state reset every item", dict(reset_records="item")), ("state carried across leaves", dict(carry=True)), ("sum kept in f64", dict(f64=True))])


class _State:
    def __init__(self, f64=False):
        self.sum, self.num, self.f64 = (np.float64(0) if f64 else np.float32(0)), 0, f64

    def add(self, req):
        self.sum = self.sum + (np.float64(req) if self.f64 else np.float32(req))
        self.num += 1

    def mean(self):
        return np.float32(self.sum) / np.float32(self.num) if not self.f64 else np.float32(self.sum / np.float64(self.num))


def walk_rule(recs, exact=False, state=None, threshold=THRESHOLD, ge=False, le=False, update_on_skip=False, only_with_opt=False, count_dead=False,
              reset_records=None, f64=False, blocks_per_item=1, trace=None, **_):
    """req_opt_scorer.rs:41-66 in f32 over one leaf's lead postings in doc order. recs: (match, req, opt, opt_hit) per lead posting
    (match False: a dead posting - another MUST clause lacks the doc, a MUST_NOT clause holds it, or it is deleted; req is then
    the lead's own score). -> (final score per record - NaN for the dead ones -, skipped per record, the state afterwards).
    trace: a list that takes (record, num, mean, 2 * req) of every decision the rule makes."""
    st = state or _State(f64)
    if exact and not (count_dead or reset_records):          # no rule: nothing is carried
        match = np.array([r[0] for r in recs], bool)
        req, opt = np.array([r[1] for r in recs], np.float32), np.array([r[2] for r in recs], np.float32)
        hit = np.array([r[3] for r in recs], bool)
        final = np.where(hit, (req + opt).astype(np.float32), req).astype(np.float32)
        final[~match] = np.nan
        return final, np.zeros(len(recs), bool), st
    every = None if reset_records is None else (blocks_per_item * BLOCK if reset_records == "item" else reset_records)
    final, skipped = np.full(len(recs), np.nan, np.float32), np.zeros(len(recs), bool)
    for i, (match, req, opt, hit) in enumerate(recs):
        if every is not None and i % every == 0:
            st = _State(f64)
        req = np.float32(req)
        if not match:
            if count_dead:
                st.add(req)
            continue
        skip = False
        if not exact and (st.num >= threshold if ge else st.num > threshold):
            two = np.float32(2.0) * req
            skip = bool(two <= st.mean()) if le else bool(two < st.mean())
            if trace is not None:
                trace.append((i, st.num, st.mean(), two))
        if skip:
            final[i], skipped[i] = req, True
            if update_on_skip:
                st.add(req)
            continue
        if not only_with_opt or hit:
            st.add(req)
        final[i] = np.float32(req + np.float32(opt)) if hit else req
    return final, skipped, st


class OptRef(as_.AndRef):
    """The hit set and the required score are AndRef's; the optional score is the f32 sum 0.0f + s_0 + s_1 ... of the oracle's per-term
    scores, in clause order, over the optional clauses present in the leaf that hold the doc; the rule is walk_rule's. `osr` may
    search several leaves (weights are the index's): the leaf's doc_base is added for it."""

    def __init__(self, oracle, leaf, osr=None):
        as_.AndRef.__init__(self, oracle, leaf, osr)
        self._rows = {}

    def term_scores(self, t):
        if t not in self._scores:
            docs = self.leaf.lists[t][0]
            docs = docs[self.leaf.alive[docs]].astype(np.int32)
            scores, matched = self.osr.score_docs(self.oracle.OP_TERM, [t], docs + np.int32(self.leaf.doc_base))
            assert matched.all(), ("the oracle's TermScorer does not hold a live doc of the fixture's list", t)
            dense = np.zeros(self.leaf.max_doc, np.float32)
            dense[docs] = scores
            dense.setflags(write=False)
            self._scores[t] = dense
        return self._scores[t]

    def present(self, q):
        return [t for t in q.should if self.leaf.lists[t][0].size > 0]

    def records(self, q):
        """One record per lead posting: (doc, match, req, opt, opt_hit) arrays."""
        base = Query(must=q.must, filt=q.filt, must_not=q.must_not)
        if as_.matches_nothing(self.leaf, base):
            z = np.zeros(0)
            return z.astype(np.int64), z.astype(bool), z.astype(np.float32), z.astype(np.float32), z.astype(bool)
        lead = self.leaf.lists[as_.lead_of(self.leaf, base)][0].astype(np.int64)
        docs, req = as_.AndRef.scores(self, base)
        match = np.zeros(lead.size, bool)
        at = np.searchsorted(lead, docs)
        match[at] = True
        r = self.term_scores(as_.lead_of(self.leaf, base))[lead].astype(np.float32)      # a dead posting: the lead's own score
        r[at] = req
        opt, hit = np.zeros(lead.size, np.float32), np.zeros(lead.size, bool)
        for t in self.present(q):                                                        # clause order, from 0.0f
            h = self.leaf.has[t][lead]
            opt = np.where(h, (opt + self.term_scores(t)[lead]).astype(np.float32), opt)
            hit |= h
        return lead, match, r, opt, hit

    def walk(self, q, exact=False, state=None, **flags):
        """-> (docs, final scores, skipped, required scores, optional sums, the state afterwards) of the leaf's matches, in doc order."""
        lead, match, req, opt, hit = self.records(q)
        if not self.present(q):
            exact = True           # no optional scorer in this leaf: the required scorer alone, no ReqOptScorer
        final, skipped, st = walk_rule(list(zip(match, req, opt, hit)), exact=exact, state=state, **flags)
        return lead[match] + self.leaf.doc_base, final[match], skipped[match], req[match], opt[match], st

    def row(self, q, k, exact=False, **flags):
        key = (q, exact, tuple(sorted(flags.items())))
        if key not in self._rows:
            self._rows[key] = self.walk(q, exact, **flags)[:2]
        docs, sc = self._rows[key]
        order = np.lexsort((docs, -sc.astype(np.float64)))[:k]
        return docs[order].astype(np.int32), sc[order], int(docs.size)


def index_row(refs, q, k, exact=False, **flags):
    """The row of a multi-leaf index: every leaf has a scorer of its own (flags carry=True: it has not)."""
    st, docs, scores = None, [], []
    for ref in refs:
        d, s, _, _, _, st_out = ref.walk(q, exact, state=st if flags.get("carry") else None, **flags)
        st = st_out
        docs.append(d)
        scores.append(s)
    docs, sc = np.concatenate(docs), np.concatenate(scores)
    order = np.lexsort((docs, -sc.astype(np.float64)))[:k]
    return docs[order].astype(np.int32), sc[order], int(docs.size)


def oracle_row(oracle, osr, q, k, exact=False):
    assert q.must and not q.filt
    return osr.search_opt(oracle.OP_TERM if len(q.must) == 1 else oracle.OP_AND, list(q.must), list(q.should), k, must_not_ids=list(q.must_not), exact=exact)


# ---- the searches over the (freq, norm byte) grid -------------------------------------------------------------------------------------
def grid_scores(weight, cache, has_norms=True):
    """bm25_compute_score in f32, left to right, for freqs 1..10 x 256 norm bytes -> [10, 256]."""
    f = np.arange(1, 11, dtype=np.float32)[:, None]
    norm = cache.astype(np.float32)[None, :] if has_norms else np.float32(1.2)
    return ((np.float32(weight) * np.float32(2.2)) * f / (f + norm)).astype(np.float32)


def _level_score(weight, cache, level):
    f = np.float32(level[0])
    return np.float32((np.float32(weight) * np.float32(2.2)) * f / (f + np.float32(cache[level[1]])))


SEARCH_BYTES = range(80, 140)        # docs of 1 to 10^8 tokens


def state_search(weight, cache, want, firsts):
    """States of 101 scored docs - one level of `firsts` n times, then one grid level 101 - n times, n = 1..100 - summed in f32 and
    in f64, each against every doc of the grid (freqs 1..10 x 256 norm bytes); want(mean32[:, None, None], mean64[...], doubled
    grid scores) -> the docs that qualify. The first hit as (the first level, n, the second level, the doc's level), or None."""
    grid = grid_scores(weight, cache)
    two = (np.float32(2.0) * grid).astype(np.float32)
    n = np.arange(1, 101)
    head = np.arange(101)[None, :] < n[:, None]
    for first in firsts:
        a = _level_score(weight, cache, first)
        for freq in range(1, 11):
            for byte in SEARCH_BYTES:
                seq = np.where(head, a, grid[freq - 1, byte]).astype(np.float32)
                s32 = np.cumsum(seq, axis=1, dtype=np.float32)[:, -1]                 # (one f32 add per doc, in doc order)
                s64 = np.cumsum(seq.astype(np.float64), axis=1)[:, -1]
                m32, m64 = (s32 / np.float32(101)).astype(np.float32), (s64 / np.float64(101)).astype(np.float32)
                ok = want(m32[:, None, None], m64[:, None, None], two[None])
                if ok.any():
                    i, f, b = np.argwhere(ok)[0]
                    return first, int(n[i]), (freq, byte), (int(f) + 1, int(b))
    return None


def equal_search(weight, cache, firsts=None):
    """A doc whose doubled score IS the f32 mean of a state."""
    return state_search(weight, cache, lambda m32, m64, two: two == m32, firsts or [HIGH] + [(f, b) for f in (1, 2, 5, 10) for b in range(100, 128, 2)])


def f64_search(weight, cache):
    """A doc whose doubled score lies between the f32 and the f64 mean of a state."""
    return state_search(weight, cache, lambda m32, m64, two: (two < m32) != (two < m64), [HIGH])


# ---- HAS_OPT at the edges of k_search_and ---------------------------------------------------------------------------------------------
NINE = (C_511, C_512, C_1172, C_2344, OVF_SMALL, SING_EVEN, EQ_A, EVERY, SPREAD)
OPT_SETS = ((C_511,), (C_512, C_1171), (C_1172,), (C_2344,), (OVF_SMALL, OVF_CAP, OVF_OVER), (SING_EVEN, SING_ODD, SING_MISS), (ABSENT,), (ABSENT, C_1172),
            (EVERY,), (EQ_A, EQ_B, EQ_C), (EQ_C, EQ_A, EQ_B), (EQ_B, EQ_C, EQ_A), (C_1172, C_1172), NINE, (SPREAD, EVERY))
OPT_KIND_TERMS = (C_511, C_512, C_1171, C_1172, C_2344, OVF_SMALL, OVF_CAP, OVF_OVER, SING_EVEN, SING_ODD, SING_MISS, ABSENT, SPREAD, EVERY)


def _with_opt():
    qs = [Query(must=q.must, should=OPT_SETS[i % len(OPT_SETS)]) for i, q in enumerate(as_.PLAIN) if len(q.must) + 9 <= 64]
    qs += [Query(must=(FP_LEAD,), should=(SPREAD,)), Query(must=(FP_LEAD, EVERY), should=(SPREAD, SPREAD_NOTAIL)), Query(must=(FP_LEAD, EVERY), should=(SPREAD,)),
           Query(must=(CORE_LEAD, C_1172), should=(C_1172,)), Query(must=(CORE_LEAD,), should=(CORE_LEAD,)), Query(must=(CORE_LEAD, C_511), should=(CORE_LEAD, C_511)),
           Query(must=(Q_LEAD, Q_C1), should=(EVERY,)), Query(must=(Q_LEAD, Q_C1), should=NINE), Query(must=(S_LEAD, S_C1), should=(C_2344, EVERY)),
           Query(must=(Q_LEAD,), should=(Q_C1,)), Query(must=(S_LEAD,), should=(S_C1, ABSENT)), Query(must=(as_.CONST,), should=(EVERY,)),
           Query(must=(as_.CONST, EVERY), should=(REG4,)), Query(must=(SING_EVEN,), should=(EVERY,)), Query(must=(SING_MISS,), should=(C_1172, EVERY)),
           Query(must=(as_.TAIL_2,), should=(C_2344,)), Query(must=(EDGE_LEAD,), should=(C_512,)), Query(must=(EDGE_LEAD, EVERY), should=(C_1171,)),
           Query(must=(as_.LEAD_128, EVERY), should=(C_512,)), Query(must=(ABSENT,), should=(EVERY,)), Query(must=(CORE_LEAD, ABSENT), should=(EVERY,))]
    qs += [Query(must=(CORE_LEAD,), should=(t,)) for t in OPT_KIND_TERMS] + [Query(must=(EDGE_LEAD, C_1172), should=(t,)) for t in OPT_KIND_TERMS]
    return qs


def _with_opt_not(with_opt):
    qs = [Query(must=q.must, should=q.should, must_not=as_.NOT_SETS[i % len(as_.NOT_SETS)]) for i, q in enumerate(with_opt) if i % 3 == 0 and len(q.must) + 12 <= 64]
    qs += [Query(must=(FP_LEAD,), should=(EVERY,), must_not=(SPREAD,)), Query(must=(Q_LEAD, Q_C1), should=(EVERY, C_2344), must_not=(S_C1, as_.G_C1)),
           Query(must=(CORE_LEAD, C_1172), should=(SING_ODD,), must_not=(SING_EVEN,)), Query(must=(EVERY,), should=(C_1172,), must_not=(REG4,)),
           Query(must=(CORE_LEAD, EVERY), should=(C_1172,), must_not=(EVERY,)), Query(must=(S_LEAD,), should=(EVERY,), must_not=(S_C1,))]
    return qs


WITH_OPT = _with_opt()
WITH_OPT_NOT = _with_opt_not(WITH_OPT)
TEN_SET = (C_511, C_512, C_1171, C_1172, C_2343, C_2344, EQ_A, EQ_B, EQ_C, EVERY)
TEN_PRESENT = Query(must=(EQ_A, C_511), should=TEN_SET)
TEN_ONE_ABSENT = Query(must=(EQ_A, C_511), should=TEN_SET[:4] + (ABSENT,) + TEN_SET[5:])
SIXTEEN = Query(must=(EQ_B,), should=TEN_SET + (OVF_SMALL, OVF_CAP, OVF_OVER, HALF_B, HALF_N, REG4))
TEN = [TEN_PRESENT, TEN_ONE_ABSENT, SIXTEEN]
OPT_FAMILIES = {"opt": WITH_OPT, "opt-not": WITH_OPT_NOT}
ALL_OPT = WITH_OPT + WITH_OPT_NOT


def is_heap_order(leaf, q):
    """Ten or more optional scorers in the leaf: the reference's DisjunctionSumScorer sums them in heap order."""
    return sum(1 for t in q.should if leaf.df(t) > 0) >= 10


def mixed():
    """The optional families dealt into one batch with and_spectrum's plain, NOT and FILTER ones -> (queries, {family: row indexes})."""
    fams = dict(as_.FAMILIES)
    fams.update(OPT_FAMILIES)
    out, rows = [], {name: [] for name in fams}
    for i in range(max(len(f) for f in fams.values())):
        for name, fam in fams.items():
            if i < len(fam):
                rows[name].append(len(out))
                out.append(fam[i])
    return out, rows, fams


def bitmap_terms(leaf, queries, and_bitmaps=0):
    """and_spectrum.bitmap_terms with the optional clauses counted: every clause of a tree of two or more, optional ones included."""
    return as_.bitmap_terms(leaf, [Query(must=q.must + q.should, filt=q.filt, must_not=q.must_not) for q in queries], and_bitmaps)


def opt_kind(leaf, t, and_bitmaps=0):
    """How an optional clause is answered: never through membership bits alone (ensure_memb_only_locked is asked for a MUST clause)."""
    kind = leaf.kind(t, and_bitmaps)
    return "walked" if kind == "memb" else kind


def queue_rows(leaf, queries, and_bitmaps=0):
    """The rows of `queries` whose batched first probe carries survivors (and_spectrum.queue_trace): two or more MUST clauses, the
    lead with a FullBlock, the clause behind it with a bitmap or membership bits -> {row: survivors queued}."""
    out = {}
    for i, q in enumerate(queries):
        if len(q.must) < 2 or as_.matches_nothing(leaf, q) or q.filt:
            continue
        req = as_.required(leaf, Query(must=q.must))
        lead, c1 = req[0][0], req[1][0]
        kind = leaf.kind(c1, and_bitmaps)
        if leaf.full_blocks(lead) and (kind in ("bitmap", "nib") or (kind == "memb" and leaf.df(lead) >= as_.MEMB_MIN_LEAD)):
            n = sum(sum(tr["survivors"]) for tr in as_.queue_trace(leaf, lead, c1, as_.AUTO_ITEM_BLOCKS))
            if n:
                out[i] = n
    return out


# ---- nested shapes ------------------------------------------------------------------------------------------------------------------
Nested = collections.namedtuple("Nested", "musts inner is_or nots at")
INNER_KINDS = ((C_511, C_512), (C_1171, C_1172), (C_2344, OVF_SMALL), (OVF_CAP, OVF_OVER), (SING_EVEN, SING_MISS), (ABSENT, C_1172), (EVERY, C_1172),
               (EQ_A, EQ_B, EQ_C), (EQ_C, EQ_B, EQ_A), (SPREAD, SPREAD_NOTAIL))
NINE_INNER = (C_511, C_512, C_1171, C_1172, C_2343, C_2344, EQ_A, EQ_B, EQ_C)


def _nested():
    rows = []
    for is_or in (True, False):
        for i, inner in enumerate(INNER_KINDS):
            musts = (FP_LEAD,) if SPREAD in inner else (CORE_LEAD,)
            rows.append(Nested(musts, inner, is_or, (), i % 2))
            rows.append(Nested(musts, inner, is_or, as_.NOT_SETS[i % len(as_.NOT_SETS)], (i + 1) % 2))
        for at in range(4):                              # the nested child at every index among three MUST clauses
            rows.append(Nested((CORE_LEAD, C_1172, EVERY), (C_2344, EQ_A), is_or, (), at))
            rows.append(Nested((EQ_A, EQ_B, EDGE_LEAD), (EQ_C, C_511), is_or, (HALF_B,), at))
        for at in (0, 1):
            rows.append(Nested((CORE_LEAD,), NINE_INNER, is_or, (), at))
            rows.append(Nested((Q_LEAD,), (Q_C1, EVERY), is_or, (), at))                # c1_nested: a one-clause prefix, nested clauses with bitmaps
            rows.append(Nested((S_LEAD,), (S_C1, C_2344), is_or, (), at))
            rows.append(Nested((EDGE_LEAD,), (C_512, C_1172), is_or, (), at))          # need_any: NEIGH docs are in none of the nested clauses
    return rows


NESTED = _nested()
