"""Fixtures and the reference model for ordered SpanNearQuery over SpanTermQuery clauses (tests/test_span_near_cpu.py proves them,
tests/test_gpu_span_near.py runs them through rgpu_search_span_near_batch).

The oracle has no span scorer, so the expectation is composed here, as tests/required_set.py and tests/phrase_bool.py do: the walk
is restated twice, independently -

  walk_reference    statement for statement NearSpansOrdered (query/spans/span_near.rs:725-852: two_phase_current_doc_matches,
                    next_start_position, stretch_to_order) over TermSpans (span_term.rs:170-200) and Spans::advance_position
                    (span.rs:214-219), driven by SpanScorer::set_freq_current_doc (span.rs:489-519): explicit cursors and flags;
  walk_lower_bound  per position p0 of clause 0, per later clause the lower bound of end(i - 1) in its list (bisect); the first p0
                    whose chain finds none ends the doc

- both add compute_slop_factor(width) = 1 / (width + 1) (bm25_similarity.rs:65-67) as np.float32 in the order the spans come out;
score() restates BM25SimScorer::score (bm25_similarity.rs:151-177) over the weight and norm cache of rucene_amd._lib.bm25_compute_weight;
search() restates BulkScorer's two-phase loop (scorer/bulk_scorer.rs:97-113, :132-150) and TopDocsCollector over a leaf's postings.

Fixtures are built through oracle.PositionsIndex with the helpers of tests/phrase_spectrum.py: one designed doc per case plus an
ordinary doc (the clauses' terms side by side), fillers that put the designed doc's positions inside packed position blocks."""
import bisect
from collections import namedtuple

import numpy as np

import phrase_spectrum as ps

K1, B = 1.2, 0.75
NO_MORE_POSITIONS = 0x7fffffff
LANES = "k_span_near_lanes"
LEFT = "k_span_near(left by the 64-candidate kernel)"
WIDE = "k_span_near(wide lists)"
ONE = "k_span_near"
CANDIDATES = "k_search_and(span candidates)"
NAMES = (LANES, LEFT, WIDE, ONE)
NEXT_LIMIT_ZERO = -2   # RGPU_NEXT_LIMIT_ZERO

# One query of a case. positions: None (phrase_spectrum.Segment.lay reads it); level: "lanes" | "left" | "wide" | None (refused with
# `error`); want: the designed doc's span freq written out by hand (0.0: a candidate, never a hit; None: not stated).
SQ = namedtuple("SQ", "terms positions slop level error want")


def sq(terms, slop, level="lanes", want=None, error=None):
    return SQ(list(terms), None, int(slop), None if error is not None else level, error, want)


def f32sum(widths):
    f = np.float32(0.0)
    for w in widths:
        f = np.float32(f + np.float32(1.0) / np.float32(np.float32(w) + np.float32(1.0)))
    return f


# ---- restatement 1: the reference's objects ---------------------------------------------------------------------------------------------
class _TermSpans:
    """span_term.rs TermSpans over one doc's positions of one term"""

    def __init__(self, positions):
        self.positions, self.freq, self.count, self.position = positions, len(positions), 0, -1

    def next_start_position(self):
        if self.count == self.freq:
            assert self.position != NO_MORE_POSITIONS
            self.position = NO_MORE_POSITIONS
            return self.position
        self.position = self.positions[self.count]
        self.count += 1
        return self.position

    def start_position(self):
        return self.position

    def end_position(self):
        if self.position == -1:
            return -1
        return self.position + 1 if self.position != NO_MORE_POSITIONS else NO_MORE_POSITIONS

    def advance_position(self, position):   # Spans::advance_position
        while self.start_position() < position:
            self.next_start_position()
        return self.start_position()


class _NearSpansOrdered:
    def __init__(self, allowed_slop, sub_spans):
        self.sub_spans, self.allowed_slop = sub_spans, allowed_slop
        self.match_start = self.match_end = self.match_width = -1
        self.first_in_current_doc = self.one_exhausted_in_current_doc = False

    def stretch_to_order(self):
        self.match_start = self.sub_spans[0].start_position()
        self.match_width = 0
        for i in range(1, len(self.sub_spans)):
            prev_end_position = self.sub_spans[i - 1].end_position()
            if self.sub_spans[i].advance_position(prev_end_position) == NO_MORE_POSITIONS:
                self.one_exhausted_in_current_doc = True
                return False
            self.match_width += self.sub_spans[i].start_position() - prev_end_position
        self.match_end = self.sub_spans[-1].end_position()
        return True

    def two_phase_current_doc_matches(self):
        self.one_exhausted_in_current_doc = False
        while self.sub_spans[0].next_start_position() != NO_MORE_POSITIONS and not self.one_exhausted_in_current_doc:
            if self.stretch_to_order() and self.match_width <= self.allowed_slop:
                self.first_in_current_doc = True
                return True
        return False

    def next_start_position(self):
        if self.first_in_current_doc:
            self.first_in_current_doc = False
            return self.match_start
        self.one_exhausted_in_current_doc = False
        while self.sub_spans[0].next_start_position() != NO_MORE_POSITIONS and not self.one_exhausted_in_current_doc:
            if self.stretch_to_order() and self.match_width <= self.allowed_slop:
                return self.match_start
        self.match_start = self.match_end = NO_MORE_POSITIONS
        return NO_MORE_POSITIONS


def walk_reference(lists, slop):
    """lists[i]: clause i's positions in the doc, ascending -> (the doc matches, span freq as np.float32, widths in span order)"""
    spans = _NearSpansOrdered(slop, [_TermSpans(list(ps_)) for ps_ in lists])
    if not spans.two_phase_current_doc_matches():
        return False, np.float32(0.0), []
    freq, widths = np.float32(0.0), []   # SpanScorer::set_freq_current_doc
    start_pos = spans.next_start_position()
    assert start_pos != NO_MORE_POSITIONS
    while start_pos != NO_MORE_POSITIONS:
        freq = np.float32(freq + np.float32(1.0) / np.float32(np.float32(spans.match_width) + np.float32(1.0)))
        widths.append(spans.match_width)
        start_pos = spans.next_start_position()
    return True, freq, widths


# ---- restatement 2: lower bounds ----------------------------------------------------------------------------------------------------------
def walk_lower_bound(lists, slop):
    freq, widths = np.float32(0.0), []
    for p0 in lists[0]:
        end, width = p0 + 1, 0
        for later in lists[1:]:
            at = bisect.bisect_left(later, end)
            if at == len(later):
                return bool(widths), freq, widths   # this chain ran out of positions: so does every later one
            width += later[at] - end
            end = later[at] + 1
        if width <= slop:
            freq = np.float32(freq + np.float32(1.0) / np.float32(np.float32(width) + np.float32(1.0)))
            widths.append(width)
    return bool(widths), freq, widths


# ---- scoring and the search loop ----------------------------------------------------------------------------------------------------------
def weight_of(doc_freqs, max_doc, doc_count, sum_ttf, boost=1.0):
    """(weight, cache[256]) of BM25Similarity::compute_weight over every clause's doc_freq, repeats included"""
    from rucene_amd import _lib
    w, _idf, cache = _lib.bm25_compute_weight(K1, B, max_doc, doc_count, sum_ttf, list(doc_freqs), boost)
    return np.float32(w), cache


def score(weight, cache, freq, norm_byte):
    """BM25SimScorer::score: weight * (k1 + 1) * freq / (freq + cache[norm]); norm_byte None: the field has no norms (k1)"""
    wk = np.float32(np.float32(weight) * np.float32(np.float32(K1) + np.float32(1.0)))
    norm = np.float32(K1) if norm_byte is None else np.float32(cache[int(norm_byte)])
    f = np.float32(freq)
    return np.float32(np.float32(wk * f) / np.float32(f + norm))


def doc_lists(postings, terms):
    """{doc: [clause i's positions]} over the docs that hold every clause's term (the conjunction's matches)"""
    by_term = {t: dict(postings[t]) for t in set(terms)}
    docs = set.intersection(*(set(by_term[t]) for t in set(terms))) if terms else set()
    return {d: [by_term[t][d] for t in terms] for d in sorted(docs)}


def is_live(live_words, doc):
    return live_words is None or bool((int(live_words[doc >> 6]) >> (doc & 63)) & 1)


def live_words(alive):
    """a bool per doc -> the FixedBitSet's u64 words"""
    return np.packbits(np.concatenate([alive, np.zeros(-alive.size % 64, dtype=bool)]), bitorder="little").view(np.uint64).copy()


def search(postings, norms, max_doc, doc_count, sum_ttf, q, k, live=None, next_limit=None, boost=1.0, walk=walk_lower_bound, doc_base=0,
           stats=None):
    """One leaf of IndexSearcher::search(SpanNearQuery, TopDocsCollector(k)) -> (docs, scores, total hits). next_limit: None = no
    limit, else the number of approximations that may go by uncollected. stats: (doc_freqs, max_doc, doc_count, sum_ttf) of the
    statistics leaf when it is not this one."""
    if any(not postings[t] for t in q.terms):
        return np.zeros(0, np.int32), np.zeros(0, np.float32), 0
    dfs, smax, scount, sttf = stats if stats is not None else ([len(postings[t]) for t in q.terms], max_doc, doc_count, sum_ttf)
    weight, cache = weight_of(dfs, smax, scount, sttf, boost)
    rows, nxt = [], 0
    for doc, lists in doc_lists(postings, q.terms).items():   # score_range_in_docs_set / score_range_all
        if is_live(live, doc):
            hit, freq, _ = walk(lists, q.slop)
            if hit:
                rows.append((doc, score(weight, cache, freq, None if norms is None else norms[doc])))
        nxt += 1
        if not rows and next_limit is not None and nxt > next_limit:
            break
    rows.sort(key=lambda r: (-float(r[1]), r[0]))
    top = rows[:k]
    return (np.array([d + doc_base for d, _ in top], np.int32), np.array([s for _, s in top], np.float32), len(rows))


def search_case(fx, q, k, **kw):
    return search(fx.postings, fx.norms, fx.max_doc, fx.doc_count, fx.sum_ttf, q, k, **kw)


def launches(q, legacy=False):
    """{launch name: must it appear} for a batch that holds this query alone"""
    out = {n: False for n in NAMES}
    out[ps.COLLECT] = out[CANDIDATES] = True
    if legacy:
        out.update({ONE: True, WIDE: q.level == "wide"})
    else:
        out.update({LANES: True, LEFT: q.level != "lanes", WIDE: q.level == "wide"})
    return out


# ---- the walk cases -------------------------------------------------------------------------------------------------------------------------
ORDER_WIDTHS = (2, 0, 6, 1, 9, 3, 12, 5, 7)   # nine spans whose f32 sum differs in its bits when added in reverse


def build_walk(salt=0, without=()):
    """without: case names whose terms this leaf does not hold (the four-leaf fixture)"""
    s = ps.Segment("walk-%d" % salt)

    def case(name, n_terms, queries_of, designed_of):
        ts = s.terms(n_terms)
        for t in ts:   # few, long filler docs keep the leaf at a few hundred docs
            s.per_doc[t] = 40 + (t + salt) % 7
        if name in without:
            s.cases.append(ps.Case(name, "absent", queries_of(ts), None, None, {}))
            return
        s.lay(name, "walk", queries_of(ts), designed_of(ts))

    case("adjacent", 2, lambda t: [sq(t, 0, want=f32sum([0]))], lambda t: {t[0]: [7], t[1]: [8]})
    case("width-2", 2, lambda t: [sq(t, 1, want=0.0), sq(t, 2, want=f32sum([2]))], lambda t: {t[0]: [7], t[1]: [10]})
    case("wrong-order", 2, lambda t: [sq(t, 5, want=0.0)], lambda t: {t[1]: [7], t[0]: [8]})
    case("shared-later-position", 2, lambda t: [sq(t, 3, want=f32sum([3, 1]))], lambda t: {t[0]: [1, 3], t[1]: [5]})
    case("wide-then-match", 2, lambda t: [sq(t, 0, want=f32sum([0]))], lambda t: {t[0]: [1, 20], t[1]: [15, 21]})
    case("cut-off-by-exhaustion", 2, lambda t: [sq(t, 5, want=f32sum([1]))], lambda t: {t[0]: [1, 10], t[1]: [3]})
    case("three-widths-add", 3, lambda t: [sq(t, 2, want=0.0), sq(t, 3, want=f32sum([3]))], lambda t: {t[0]: [1], t[1]: [3], t[2]: [6]})
    case("x-x", 1, lambda t: [sq(t * 2, 0, level="left", want=f32sum([0])), sq(t * 2, 2, level="left", want=f32sum([0, 2]))], lambda t: {t[0]: [1, 2, 5]})
    case("x-y-x", 2, lambda t: [sq([t[0], t[1], t[0]], 1, want=f32sum([1])), sq([t[0], t[1], t[0]], 3, want=f32sum([1, 3]))],
         lambda t: {t[0]: [1, 4, 9], t[1]: [2, 6]})
    pa = [100 * (i + 1) for i in range(len(ORDER_WIDTHS))]
    case("sum-order", 2, lambda t: [sq(t, max(ORDER_WIDTHS), want=f32sum(ORDER_WIDTHS))],
         lambda t: {t[0]: pa, t[1]: [p + 1 + w for p, w in zip(pa, ORDER_WIDTHS)]})
    return s.finish(300 + salt)


# ---- the ladder ------------------------------------------------------------------------------------------------------------------------------
FREQS = (1, 10, 11, 128, 129, 1024, 1025)


def freq_level(f):
    return "lanes" if f <= ps.LANE_CAP else "left" if f <= ps.SMALL_CAP else "wide" if f <= ps.LIST_CAP else None


def build_freq():
    """A clause's term f times in the doc: as clause 0 (the chains' list) and, for the rungs' upper sides, as clause 1 (the searched
    list). Slop 0: only the last position of the long list is followed at once by the other term; slop 4000: every p0 has a span."""
    s = ps.Segment("span-freq")
    for f in FREQS:
        a, b = s.terms(2)
        s.per_doc[a], s.per_doc[b] = 60, 61
        pa = ps.alt(f)
        lv = freq_level(f)
        err = ps.UNSUPPORTED if lv is None else None
        widths = [pa[-1] - p for p in pa]
        s.lay("first-%d" % f, "freq", [sq([a, b], 0, lv, f32sum([0]), err), sq([a, b], 4000, lv, f32sum(widths), err)], {a: pa, b: [pa[-1] + 1]})
    for f in (11, 129, 1025):
        b, a = s.terms(2)
        s.per_doc[a], s.per_doc[b] = 62, 63
        pa = ps.alt(f, first=4)
        lv = freq_level(f)
        err = ps.UNSUPPORTED if lv is None else None
        s.lay("second-%d" % f, "freq", [sq([b, a], 0, lv, f32sum([0]), err), sq([b, a], 4000, lv, f32sum([0]), err)], {b: [3], a: pa})
    return s.finish(301)


def build_terms():
    s = ps.Segment("span-terms")
    for n in (ps.LANE_TERMS, ps.LANE_TERMS + 1, ps.MAX_TERMS):
        ts = s.terms(n)
        for t in ts:
            s.per_doc[t] = 64
        lv = "lanes" if n <= ps.LANE_TERMS else "left"
        # clause i at 20 + 2 i: n - 1 gaps of width 1
        s.lay("clauses-%d" % n, "terms", [sq(ts, n - 2, lv, 0.0), sq(ts, n - 1, lv, f32sum([n - 1]))], {t: [20 + 2 * i] for i, t in enumerate(ts)},
              shape=dict(n_terms=n))
    ts = s.terms(ps.MAX_TERMS + 1)
    for t in ts:
        s.per_doc[t] = 64
    s.lay("clauses-17", "terms", [sq(ts, 20, None, f32sum([16]), ps.ILLEGAL_ARGUMENT)], {t: [20 + 2 * i] for i, t in enumerate(ts)},
          shape=dict(n_terms=ps.MAX_TERMS + 1))
    return s.finish(302)


def build_place():
    """Where the positions lie: 16-bit cells, the edge of a packed position block, a singleton term."""
    s = ps.Segment("span-place")
    for name, pos, lv in (("pos-32767", 32766, "lanes"), ("pos-32768", 32767, "left")):   # the second clause's position is pos + 1
        a, b = s.terms(2)
        s.per_doc[a], s.per_doc[b] = 60, 61
        s.lay(name, "int16", [sq([a, b], 0, lv, f32sum([0]))], {a: [pos], b: [pos + 1]}, shape=dict(value=pos + 1))
    f = 7
    for end, behind, lv in ((ps.BLOCK - 1, "packed", "lanes"), (ps.BLOCK, "packed", "lanes"), (ps.BLOCK + 1, "packed", "lanes"),
                            (ps.BLOCK + 1, "trailing", "left")):
        a, b = s.terms(2)
        s.per_doc[a], s.per_doc[b] = 4, 61
        after = list(ps.BEHIND[behind])
        if end < ps.BLOCK:
            after = [("packed", ps.BLOCK - end)] + after
        pa = ps.alt(f)
        s.lay("end-%d-behind-%s" % (end, behind), "straddle", [sq([a, b], 0, lv, f32sum([0])), sq([a, b], 50, lv, f32sum([pa[-1] - p for p in pa]))],
              {a: pa, b: [pa[-1] + 1]}, at={a: (2, end - f)}, after={a: after}, shape=dict(placed=a, block=2, skip=end - f, behind=behind, end=end))
    x, b = s.terms(2)
    s.per_doc[b] = 61
    s.lay("singleton", "singleton", [sq([x, b], 0, "left", f32sum([0])), sq([b, x], 3, "left", 0.0)], {x: [9], b: [10]}, singletons=(x,),
          shape=dict(singleton=x))
    gone, b = s.terms(2)   # a term no doc of the leaf holds
    s.per_doc[b] = 61
    s.doc({b: [5]})
    s.cases.append(ps.Case("absent-term", "absent", [sq([gone, b], 0, None, None), sq([b, gone], 0, None, None)], None, None, {}))
    return s.finish(303)


BUILDERS = {"walk": build_walk, "freq": build_freq, "terms": build_terms, "place": build_place}
_built = {}


def segment(name):
    if name not in _built:
        _built[name] = BUILDERS[name]()
    return _built[name]


def all_cases():
    return [(name, c) for name in BUILDERS for c in segment(name).cases]


# ---- four leaves with doc bases (the Python mirror) ---------------------------------------------------------------------------------------
def four_leaves():
    """The walk cases on four leaves of different sizes; leaf 1 lacks one case's terms, leaf 3 another's."""
    if "four" not in _built:
        _built["four"] = [build_walk(1, without=()), build_walk(2, without=("adjacent",)), build_walk(3), build_walk(4, without=("sum-order",))]
    return _built["four"]


def search_leaves(fxs, q, k, next_limit=None, boost=1.0):
    """GpuIndexSearcher's view: statistics of the first leaf with the largest max_doc over the summed max_doc (searcher.rs:306-363),
    every leaf's rows merged by (score desc, doc asc)."""
    sl = max(range(len(fxs)), key=lambda i: (fxs[i].max_doc, -i))
    stats = ([len(fxs[sl].postings[t]) for t in q.terms], sum(fx.max_doc for fx in fxs), fxs[sl].doc_count, fxs[sl].sum_ttf)
    rows, total, base = [], 0, 0
    for fx in fxs:
        d, sc, tot = search_case(fx, q, 1 << 30, next_limit=next_limit, boost=boost, doc_base=base, stats=stats)
        rows += list(zip(d.tolist(), sc.tolist()))
        total += tot
        base += fx.max_doc
    rows.sort(key=lambda r: (-r[1], r[0]))
    return np.array([d for d, _ in rows[:k]], np.int32), np.array([s for _, s in rows[:k]], np.float32), total


# ---- seeded random small docs ----------------------------------------------------------------------------------------------------------------
def random_docs(n, seed=77):
    """(lists, slop): 2..5 clauses, 0..12 positions each out of a small range, clauses that repeat a term, slop 0..6"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        n_clauses = int(rng.integers(2, 6))
        n_distinct = int(rng.integers(1, n_clauses + 1))
        span = int(rng.integers(6, 40))
        held = [sorted(set(rng.integers(0, span, size=int(rng.integers(0, 13))).tolist())) for _ in range(n_distinct)]
        clause_terms = list(range(n_distinct)) + rng.integers(0, n_distinct, size=n_clauses - n_distinct).tolist()
        rng.shuffle(clause_terms)
        out.append(([held[t] for t in clause_terms], int(rng.integers(0, 7))))
    return out
