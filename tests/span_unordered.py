"""Fixtures and the reference model for unordered SpanNearQuery over SpanTermQuery clauses (tests/test_span_unordered_cpu.py proves
them, tests/test_gpu_span_unordered.py runs them through rgpu_search_span_unordered_batch).

The oracle has no span scorer, so the expectation is composed here, as tests/span_near.py does for the ordered query. The walk is
restated twice, independently -

  walk_reference  (a) the reference's objects, statement for statement: TermSpans (span_term.rs:170-200, tests/span_near.py's),
                  SpansCell with adjust_length / adjust_max (span_near.rs:532-588), the heap as an explicit array with push /
                  sift_up / sift_down_range (util/external/binary_heap.rs:121-190, a copy of the std the reference is pinned to),
                  SpansCellElement's reversed order (:681-696), NearSpansUnordered (:333-528) and SpanScorer's loop
                  (span.rs:489-519). One ReferenceWalk object serves a whole leaf, so max_end_position_cell_idx is carried from doc
                  to doc as the reference carries it.
                  The previous doc's index is harmless: on a fresh doc every TermSpans stands at -1 / -1, so when cell 0 moves to
                  its first position either it IS the max cell (its end is compared with itself, nothing changes, and it holds the
                  only real end) or its end >= 1 beats the max cell's -1. From there on adjust_max keeps the first cell, in clause
                  order, that reaches the largest end - and only that cell's start and end are ever read.
  walk_events     (b) the closed form for docs WITHOUT ties (no position shared by two clauses): the events (p, t) in ascending p;
                  when (p, t) is the heap's top every other cell stands on its first position > p; the walk ends with the first
                  event that is the last position of its clause.

walk_rule restates the loop with a tie RULE in place of the array ("lowest clause index moves first" / "highest ..."): what a
re-derived order would compute. The fixtures hold docs on which the array and both rules give three different width lists.

Scoring, the two-phase search loop and the leaf merge are tests/span_near.py's (weight_of, score, search, search_leaves)."""
import bisect
from collections import namedtuple

import numpy as np

import phrase_spectrum as ps
import span_near as sn
from span_near import NO_MORE_POSITIONS, f32sum, sq

LANES = "k_span_unordered_lanes"
LEFT = "k_span_unord(left by the 64-candidate kernel)"   # (rgpu_kernel_stat.name holds 47 characters)
WIDE = "k_span_unordered(wide pool)"
ONE = "k_span_unordered"
CANDIDATES = sn.CANDIDATES
NAMES = (LANES, LEFT, WIDE, ONE)
NEXT_LIMIT_ZERO = sn.NEXT_LIMIT_ZERO


# ---- restatement (a): the reference's objects -----------------------------------------------------------------------------------------
class _SpansCell:
    """span_near.rs:532-588"""

    def __init__(self, parent, spans, index):
        self.parent, self.spans, self.index, self.span_length = parent, spans, index, -1

    def adjust_length(self):
        if self.span_length != -1:   # subtract old, possibly from a previous doc
            self.parent.total_span_length -= self.span_length
        assert self.spans.start_position() != NO_MORE_POSITIONS
        self.span_length = self.end_position() - self.start_position()
        assert self.span_length >= 0
        self.parent.total_span_length += self.span_length

    def adjust_max(self):
        max_cell = self.parent.sub_span_cells[self.parent.max_end_position_cell_idx]
        if self.end_position() > max_cell.end_position():
            self.parent.max_end_position_cell_idx = self.index

    def next_start_position(self):
        res = self.spans.next_start_position()
        if res != NO_MORE_POSITIONS:
            self.adjust_length()
        self.adjust_max()
        return res

    def start_position(self):
        return self.spans.start_position()

    def end_position(self):
        return self.spans.end_position()


def _cmp(a, b):
    """SpansCellElement::cmp (:681-696), reversed for the priority queue: < 0 "less", 0 "equal", > 0 "greater" """
    start1, start2 = a.start_position(), b.start_position()
    if start1 == start2:
        e1, e2 = a.end_position(), b.end_position()
        return (e2 > e1) - (e2 < e1)
    return (start2 > start1) - (start2 < start1)


class _BinaryHeap:
    """binary_heap.rs: the heap IS its array. disturbed: "take the left child on equal" - not the reference, the CPU test's proof
    that the fixtures can see the array."""

    def __init__(self, disturbed=False):
        self.data, self.disturbed = [], disturbed

    def clear(self):
        self.data = []

    def peek(self):
        return self.data[0]

    def push(self, item):   # :131-135
        old_len = len(self.data)
        self.data.append(item)
        self.sift_up(0, old_len)

    def sift_up(self, start, pos):   # :149-163 (the hole: the element is taken out and put back where the loop stops)
        element = self.data[pos]
        while pos > start:
            parent = (pos - 1) // 2
            if _cmp(element, self.data[parent]) <= 0:
                break
            self.data[pos] = self.data[parent]
            pos = parent
        self.data[pos] = element
        return pos

    def sift_down_range(self, pos, end):   # :167-185
        element = self.data[pos]
        child = 2 * pos + 1
        while child < end:
            right = child + 1
            # compare with the greater of the two children
            if right < end and (_cmp(self.data[child], self.data[right]) < 0 if self.disturbed else _cmp(self.data[child], self.data[right]) <= 0):
                child = right
            if _cmp(element, self.data[child]) >= 0:   # if we are already in order, stop
                break
            self.data[pos] = self.data[child]
            pos = child
            child = 2 * pos + 1
        self.data[pos] = element

    def sift_down(self, pos):   # :187-190; PeekMut::drop (:29-35) calls sift_down(0)
        self.sift_down_range(pos, len(self.data))


class _NearSpansUnordered:
    """span_near.rs:333-528 over TermSpans clauses. The object lives as long as the leaf's scorer: start_doc puts every clause's
    TermSpans on a fresh doc (start -1, end -1), everything else - max_end_position_cell_idx, total_span_length, the cells'
    span_length - is what the previous doc left."""

    def __init__(self, allowed_slop, n_clauses, disturbed=False):
        self.allowed_slop = allowed_slop
        self.sub_span_cells = [_SpansCell(self, sn._TermSpans([]), i) for i in range(n_clauses)]
        self.span_position_queue = _BinaryHeap(disturbed)
        self.total_span_length = 0
        self.max_end_position_cell_idx = 0
        self.first_in_current_doc = self.one_exhausted_in_current_doc = False
        self.span_position_queue.push(self.sub_span_cells[0])   # single_cell_to_positions_queue (:386-391)

    def start_doc(self, lists):
        for cell, positions in zip(self.sub_span_cells, lists):
            cell.spans = sn._TermSpans(list(positions))

    def sub_span_cells_to_positions_queue(self):   # :393-404
        self.span_position_queue.clear()
        for cell in self.sub_span_cells:
            assert cell.start_position() == -1
            cell.next_start_position()
            assert cell.start_position() != NO_MORE_POSITIONS
            self.span_position_queue.push(cell)

    def min_cell(self):
        return self.span_position_queue.peek()

    def at_match(self):   # :406-412
        max_cell = self.sub_span_cells[self.max_end_position_cell_idx]
        return max_cell.end_position() - self.min_cell().start_position() - self.total_span_length <= self.allowed_slop

    def _advance_top(self):
        """peek_mut().unwrap().spans_mut().next_start_position(), then the PeekMut is dropped: sift_down(0)"""
        nxt = self.span_position_queue.peek().next_start_position()
        self.span_position_queue.sift_down(0)
        return nxt

    def two_phase_current_doc_matches(self):   # :428-447
        self.sub_span_cells_to_positions_queue()
        while True:
            if self.at_match():
                self.first_in_current_doc = True
                self.one_exhausted_in_current_doc = False
                return True
            assert self.min_cell().start_position() != NO_MORE_POSITIONS
            if self._advance_top() == NO_MORE_POSITIONS:   # exhausted a sub_span in current doc
                return False

    def next_start_position(self):   # :451-486
        if self.first_in_current_doc:
            self.first_in_current_doc = False
            return self.min_cell().start_position()
        while self.min_cell().start_position() == -1:   # initially at current doc
            self._advance_top()
        assert self.min_cell().start_position() != NO_MORE_POSITIONS
        while True:
            if self._advance_top() == NO_MORE_POSITIONS:
                self.one_exhausted_in_current_doc = True
                return NO_MORE_POSITIONS
            if self.at_match():
                return self.min_cell().start_position()

    def width(self):   # :512-515
        return self.sub_span_cells[self.max_end_position_cell_idx].start_position() - self.min_cell().start_position()


class ReferenceWalk:
    """walk(lists, slop) for the docs of one leaf in doc order: one NearSpansUnordered for all of them"""

    def __init__(self, disturbed=False):
        self.spans, self.disturbed = None, disturbed

    def __call__(self, lists, slop):
        if self.spans is None or len(self.spans.sub_span_cells) != len(lists) or self.spans.allowed_slop != slop:
            self.spans = _NearSpansUnordered(slop, len(lists), self.disturbed)
        spans = self.spans
        spans.start_doc(lists)
        if not spans.two_phase_current_doc_matches():
            return False, np.float32(0.0), []
        freq, widths = np.float32(0.0), []   # SpanScorer::set_freq_current_doc
        start_pos = spans.next_start_position()
        assert start_pos != NO_MORE_POSITIONS
        while start_pos != NO_MORE_POSITIONS:
            w = spans.width()
            freq = np.float32(freq + np.float32(1.0) / np.float32(np.float32(w) + np.float32(1.0)))
            widths.append(w)
            start_pos = spans.next_start_position()
        return True, freq, widths


def walk_reference(lists, slop, disturbed=False, previous=None):
    """One doc. previous: (lists, slop-compatible) docs the same NearSpansUnordered has seen before (what they leave behind)."""
    walk = ReferenceWalk(disturbed)
    for earlier in previous or ():
        walk(earlier, slop)
    return walk(lists, slop)


# ---- restatement (b): the closed form of a doc without ties ---------------------------------------------------------------------------
def tie_free(lists):
    every = [p for l in lists for p in l]
    return len(every) == len(set(every))


def walk_events(lists, slop):
    assert tie_free(lists)
    n = len(lists)
    freq, widths = np.float32(0.0), []
    for p, t in sorted((p, t) for t, l in enumerate(lists) for p in l):
        top = p
        for u, other in enumerate(lists):
            if u != t:
                top = max(top, other[bisect.bisect_right(other, p)])   # (it exists: the clause's last position would have ended the walk)
        width = top - p
        if width <= slop + n - 1:
            freq = np.float32(freq + np.float32(1.0) / np.float32(np.float32(width) + np.float32(1.0)))
            widths.append(width)
        if p == lists[t][-1]:
            break
    return bool(widths), freq, widths


# ---- the loop under a tie RULE (not the reference) ------------------------------------------------------------------------------------
def walk_rule(lists, slop, highest):
    n = len(lists)
    cur, widths = [0] * n, []
    while True:
        starts = [l[c] for l, c in zip(lists, cur)]
        low = min(starts)
        tied = [t for t in range(n) if starts[t] == low]
        top = tied[-1] if highest else tied[0]
        if max(starts) - low <= slop + n - 1:
            widths.append(max(starts) - low)
        cur[top] += 1
        if cur[top] == len(lists[top]):
            return bool(widths), f32sum(widths), widths


def three_way(lists, slop):
    """the width lists of the heap walk, "lowest index first" and "highest index first" when all three differ, else None"""
    a, b, c = walk_reference(lists, slop)[2], walk_rule(lists, slop, False)[2], walk_rule(lists, slop, True)[2]
    return (a, b, c) if a != b and a != c and b != c else None


ISSUE_EXAMPLE = [[4, 10], [5, 7, 11], [0, 1, 4, 6], [3, 4, 6]]   # slop 0: heap 2, 1, 2 | lowest 2, 1 | highest 2, 1, 2, 2


def seeded_three_way(count, seed=5, n_clauses=4):
    """`count` random docs of four DISTINCT terms (a dozen positions out of 0..11, so terms share positions) at slop 0 on which the
    three tie orders give three different width lists"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        lists = [sorted(set(rng.integers(0, 12, size=int(rng.integers(2, 5))).tolist())) for _ in range(n_clauses)]
        if three_way(lists, 0) is not None and lists != ISSUE_EXAMPLE:
            out.append(lists)
    return out


# ---- the search loop ------------------------------------------------------------------------------------------------------------------
def search(postings, norms, max_doc, doc_count, sum_ttf, q, k, **kw):
    """tests/span_near.py's search with NearSpansUnordered's walk (one scorer per leaf)"""
    kw.setdefault("walk", ReferenceWalk())
    return sn.search(postings, norms, max_doc, doc_count, sum_ttf, q, k, **kw)


def search_case(fx, q, k, **kw):
    return search(fx.postings, fx.norms, fx.max_doc, fx.doc_count, fx.sum_ttf, q, k, **kw)


def search_leaves(fxs, q, k, next_limit=None, boost=1.0):
    """tests/span_near.py's search_leaves with the unordered walk"""
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


def designed_lists(fx, case, q):
    """the designed doc's positions, clause by clause"""
    return [dict(fx.postings[t])[case.designed] for t in q.terms]


def launches(q, legacy=False):
    """{launch name: must it appear} for a batch that holds this query alone"""
    out = {n: False for n in NAMES}
    out[ps.COLLECT] = out[CANDIDATES] = True
    if legacy:
        out.update({ONE: True, WIDE: q.level == "wide"})
    else:
        out.update({LANES: True, LEFT: q.level != "lanes", WIDE: q.level == "wide"})
    return out


USQ = namedtuple("USQ", sn.SQ._fields + ("widths",))   # tests/span_near.py's SQ and the designed doc's hand-written WIDTH LIST


def usq(terms, slop, level="lanes", widths=None, error=None):
    """widths None: not stated; []: a candidate, never a hit"""
    q = sq(terms, slop, level, None if widths is None else (f32sum(widths) if widths else 0.0), error)
    return USQ(*q, None if widths is None else list(widths))


def widths_of(q):
    return q.widths


# ---- the walk cases -------------------------------------------------------------------------------------------------------------------
ORDER_WIDTHS = tuple(w + 1 for w in sn.ORDER_WIDTHS)   # nine spans (widths >= 1: distinct terms side by side) whose f32 sum differs in reverse


def build_walk(salt=0, without=()):
    """without: case names whose terms this leaf does not hold (the four-leaf fixture)"""
    s = ps.Segment("unordered-walk-%d" % salt)

    def case(name, n_terms, queries_of, designed_of):
        ts = s.terms(n_terms)
        for t in ts:   # few, long filler docs keep the leaf at a few hundred docs
            s.per_doc[t] = 40 + (t + salt) % 7
        if name in without:
            s.cases.append(ps.Case(name, "absent", queries_of(ts), None, None, {}))
            return
        s.lay(name, "walk", queries_of(ts), designed_of(ts))

    # (n = 2: a span counts iff width <= slop + 1)
    case("adjacent", 2, lambda t: [usq(t, 0, widths=[1])], lambda t: {t[0]: [7], t[1]: [8]})                     # at_match true at set-up
    case("transposed", 2, lambda t: [usq(t, 0, widths=[1]), usq(t, 5, widths=[1])], lambda t: {t[1]: [7], t[0]: [8]})
    # a@1, a@3, b@5 at slop 3: widths 4, 2 - in either clause order
    case("cross-check", 2, lambda t: [usq(t, 3, widths=[4, 2]), usq(t[::-1], 3, widths=[4, 2])], lambda t: {t[0]: [1, 3], t[1]: [5]})
    case("width-at-the-bound", 2, lambda t: [usq(t, 1, widths=[]), usq(t, 2, widths=[3])], lambda t: {t[0]: [7], t[1]: [10]})
    case("width-at-the-bound-3", 3, lambda t: [usq(t, 2, widths=[]), usq(t, 3, widths=[5])], lambda t: {t[0]: [1], t[2]: [3], t[1]: [6]})
    # clause 0 runs out at its only position; the other two stand side by side further on: a candidate, never a hit
    case("runs-out-in-front", 3, lambda t: [usq(t, 0, widths=[]), usq(t, 5, widths=[])], lambda t: {t[0]: [1], t[1]: [20, 21], t[2]: [22]})
    case("match-only-later", 2, lambda t: [usq(t, 0, widths=[1])], lambda t: {t[0]: [1, 20], t[1]: [21]})       # set-up: width 20
    # (1, 5) 4 | a -> 9: (9, 5) 4 | b -> 12: (9, 12) 3 | a -> 30: (30, 12) 18 | b runs out
    case("alternating", 2, lambda t: [usq(t, 3, widths=[4, 4, 3]), usq(t, 2, widths=[3]), usq(t, 17, widths=[4, 4, 3, 18])],
         lambda t: {t[0]: [1, 9, 30], t[1]: [5, 12]})
    pa = [100 * (i + 1) for i in range(len(ORDER_WIDTHS))]
    case("sum-order", 2, lambda t: [usq(t, max(ORDER_WIDTHS) - 1, widths=ORDER_WIDTHS)],
         lambda t: {t[0]: pa, t[1]: [p + w for p, w in zip(pa, ORDER_WIDTHS)]})
    return s.finish(400 + salt)


# ---- ties -----------------------------------------------------------------------------------------------------------------------------
def build_ties():
    s = ps.Segment("unordered-ties")

    def case(name, n_terms, queries_of, designed_of, **kw):
        ts = s.terms(n_terms)
        for t in ts:
            s.per_doc[t] = 40 + t % 7
        s.lay(name, "ties", queries_of(ts), designed_of(ts), **kw)

    # n distinct terms stacked on the same positions: every state is a tie of all n cells
    case("stacked-2", 2, lambda t: [usq(t, 0, widths=[0, 0]), usq(t, 2, widths=[0, 3, 0])], lambda t: {t[0]: [4, 7], t[1]: [4, 7]})
    case("stacked-3", 3, lambda t: [usq(t, 0, widths=[0, 2, 1]), usq(t, 1, widths=[0, 2, 3, 1])],
         lambda t: {t[0]: [4, 6, 9], t[1]: [4, 6], t[2]: [4, 7, 9]})
    case("stacked-4", 4, lambda t: [usq(t, 0, widths=STACKED_4[0]), usq(t, 2, widths=STACKED_4[0])],
         lambda t: {t[0]: [2, 5, 6], t[1]: [2, 5], t[2]: [2, 3, 6], t[3]: [2, 6, 8]})
    case("stacked-5", 5, lambda t: [usq(t, 0, widths=STACKED_5[0]), usq(t, 1, widths=STACKED_5[0])],
         lambda t: {t[0]: [3, 4, 8], t[1]: [3, 6, 8], t[2]: [3, 4, 7], t[3]: [3, 6], t[4]: [3, 4, 6, 8]})
    # the docs on which the array, "lowest index first" and "highest index first" give three different width lists
    case("three-way-issue", 4, lambda t: [usq(t, 0, widths=[2, 1, 2])], lambda t: {x: l for x, l in zip(t, ISSUE_EXAMPLE)})
    for i, lists in enumerate(seeded_three_way(3)):
        assert three_way(lists, 0) is not None
        case("three-way-%d" % i, 4, lambda t, i=i: [usq(t, 0, widths=THREE_WAY[i])], lambda t, lists=lists: {x: l for x, l in zip(t, lists)})
    # one term under two and under three clauses: both cells walk the same list, always tied or one step apart
    case("same-term-twice", 1, lambda t: [usq(t * 2, 0, "left", widths=[0, 1, 0, 0]), usq(t * 2, 2, "left", widths=[0, 1, 0, 3, 0])],
         lambda t: {t[0]: [1, 2, 5]})
    case("same-term-thrice", 2, lambda t: [usq([t[0], t[1], t[0]], 0, widths=SAME_THRICE[0]), usq([t[0], t[0], t[0]], 1, "left", widths=SAME_THRICE[1])],
         lambda t: {t[0]: [1, 2, 4, 5], t[1]: [2, 6]})
    # both cells stand on 9, their last position, when the first of them runs out
    case("tie-at-the-end", 2, lambda t: [usq(t, 0, widths=[1, 1, 0]), usq(t[::-1], 0, widths=[1, 1, 0])], lambda t: {t[0]: [7, 9], t[1]: [8, 9]})
    return s.finish(410)


# (the short lists in the cases above were worked out by hand from the rules in the module docstring; these longer ones - four and
# five tied cells, three cells on one list, the seeded three-way docs - were written down from restatement (a) once it agreed with the
# hand-worked ones and with the issue's example, and pin it from then on)
STACKED_4 = {0: [0, 3, 3, 3, 3, 1, 1]}
STACKED_5 = {0: [0, 1, 1, 3, 3, 2, 4, 4, 2]}
THREE_WAY = {0: [3, 2, 2, 3], 1: [3, 2, 1, 1, 2], 2: [2, 3, 3, 3]}   # the heap walk's lists of seeded_three_way(3)
SAME_THRICE = {0: [1, 1, 0, 2, 2, 2, 2, 1], 1: [0, 1, 1, 0, 2, 2, 0, 1, 1, 0]}


# ---- the ladder -------------------------------------------------------------------------------------------------------------------------
def pool_level(n_clauses, freqs, fits16=True):
    if n_clauses <= ps.LANE_TERMS and max(freqs) <= ps.LANE_CAP and fits16:
        return "lanes"
    return "left" if sum(freqs) <= ps.SMALL_POOL else "wide" if sum(freqs) <= ps.POOL else None


FREQS = (1, ps.LANE_CAP, ps.LANE_CAP + 1, ps.SMALL_POOL - 1, ps.SMALL_POOL, ps.POOL - 1, ps.POOL)   # + 1 position of the other clause: the pool


def build_pool():
    """Clause 0's term f times in the doc, clause 1's once, behind the last of them: the pool holds f + 1 positions. Slop 0: only the
    last position of the long list has the other term next to it; slop 6000: every position of the long list has a span."""
    s = ps.Segment("unordered-pool")
    for f in FREQS:
        a, b = s.terms(2)
        s.per_doc[a], s.per_doc[b] = 60, 61
        pa = ps.alt(f)
        lv = pool_level(2, [f, 1])
        err = ps.UNSUPPORTED if lv is None else None
        widths = [pa[-1] + 1 - p for p in pa]
        assert widths[0] <= 6000 + 1
        s.lay("pool-%d" % (f + 1), "pool", [usq([a, b], 0, lv, [1], err), usq([b, a], 6000, lv, widths, err)], {a: pa, b: [pa[-1] + 1]}, shape=dict(pool=f + 1))
    return s.finish(401)


def build_terms():
    s = ps.Segment("unordered-terms")
    for n in (ps.LANE_TERMS, ps.LANE_TERMS + 1, ps.MAX_TERMS):
        ts = s.terms(n)
        for t in ts:
            s.per_doc[t] = 64
        lv = "lanes" if n <= ps.LANE_TERMS else "left"
        # clause i at 20 + 2 i: one state, width 2 (n - 1), a span iff 2 (n - 1) <= slop + n - 1
        s.lay("clauses-%d" % n, "terms", [usq(ts, n - 2, lv, []), usq(ts, n - 1, lv, [2 * (n - 1)])], {t: [20 + 2 * i] for i, t in enumerate(ts)},
              shape=dict(n_terms=n))
    ts = s.terms(ps.MAX_TERMS + 1)
    for t in ts:
        s.per_doc[t] = 64
    s.lay("clauses-17", "terms", [usq(ts, 20, None, [32], ps.ILLEGAL_ARGUMENT)], {t: [20 + 2 * i] for i, t in enumerate(ts)},
          shape=dict(n_terms=ps.MAX_TERMS + 1))
    return s.finish(402)


def build_place():
    """Where the positions lie: 16-bit cells, the edge of a packed position block, a singleton term, an absent term."""
    s = ps.Segment("unordered-place")
    for name, pos, lv in (("pos-32767", 32766, "lanes"), ("pos-32768", 32767, "left")):   # the second clause's position is pos + 1
        a, b = s.terms(2)
        s.per_doc[a], s.per_doc[b] = 60, 61
        s.lay(name, "int16", [usq([a, b], 0, lv, [1]), usq([b, a], 0, lv, [1])], {a: [pos], b: [pos + 1]}, shape=dict(value=pos + 1))
    f = 7
    for end, behind, lv in ((ps.BLOCK, "packed", "lanes"), (ps.BLOCK + 1, "packed", "lanes"), (ps.BLOCK + 1, "trailing", "left"),
                            (ps.BLOCK + 1, "equal", "left")):
        a, b = s.terms(2)
        s.per_doc[a], s.per_doc[b] = 4, 61
        after = list(ps.BEHIND[behind])
        if behind == "equal":   # the doc's last delta belongs to the all-equal block
            after = [("equal", 2 * ps.BLOCK - end)] + after[1:]
        pa = ps.alt(f, last=1 if behind == "equal" else None)
        s.lay("end-%d-behind-%s" % (end, behind), "straddle", [usq([a, b], 0, lv, [1]), usq([a, b], 50, lv, [pa[-1] + 1 - p for p in pa])],
              {a: pa, b: [pa[-1] + 1]}, at={a: (2, end - f)}, after={a: after}, shape=dict(placed=a, block=2, skip=end - f, behind=behind, end=end))
    x, b = s.terms(2)
    s.per_doc[b] = 61
    s.lay("singleton", "singleton", [usq([x, b], 0, "left", [1]), usq([b, x], 3, "left", [1])], {x: [9], b: [10]}, singletons=(x,),
          shape=dict(singleton=x))
    gone, b = s.terms(2)   # a term no doc of the leaf holds
    s.per_doc[b] = 61
    s.doc({b: [5]})
    s.cases.append(ps.Case("absent-term", "absent", [usq([gone, b], 0, None, None), usq([b, gone], 0, None, None)], None, None, {}))
    return s.finish(403)


BUILDERS = {"walk": build_walk, "ties": build_ties, "pool": build_pool, "terms": build_terms, "place": build_place}
_built = {}


def segment(name):
    if name not in _built:
        _built[name] = BUILDERS[name]()
    return _built[name]


def all_cases():
    return [(name, c) for name in BUILDERS for c in segment(name).cases]


def four_leaves():
    """The walk cases on four leaves of different sizes; leaf 1 lacks one case's terms, leaf 3 another's."""
    if "four" not in _built:
        _built["four"] = [build_walk(1, without=()), build_walk(2, without=("adjacent",)), build_walk(3), build_walk(4, without=("sum-order",))]
    return _built["four"]


# ---- seeded random small docs -----------------------------------------------------------------------------------------------------------
def random_docs(n, seed, ties):
    """(lists, slop): 2..5 clauses of DISTINCT terms, 1..4 positions each (a dozen at most per doc), slop 0..4. ties: positions out of
    0..11, docs without a shared position dropped | a random split of distinct positions, so no two clauses share one"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        n_clauses = int(rng.integers(2, 6))
        sizes = [int(rng.integers(1, 5)) for _ in range(n_clauses)]
        while sum(sizes) > 12:
            sizes[int(np.argmax(sizes))] -= 1
        if ties:
            lists = [sorted(set(rng.integers(0, 12, size=f).tolist())) for f in sizes]
            if tie_free(lists):
                continue
        else:
            pool = rng.permutation(30)[:sum(sizes)].tolist()
            lists = [sorted(pool[sum(sizes[:i]):sum(sizes[:i + 1])]) for i in range(n_clauses)]
        out.append((lists, int(rng.integers(0, 5))))
    return out
