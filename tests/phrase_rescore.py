"""Fixtures and the reference for rescoring with phrase queries (QueryRescorer + PhraseQuery: rgpu_rescore_phrase_batch). Plain
Python / numpy; tests/test_phrase_rescore_cpu.py proves them, tests/test_gpu_phrase_rescore.py runs them on the device.

The reference, rescore_ref, restates query_rescore + combine_score + combine_docs (search/scorer/rescorer.rs:300-403) in np.float32
over a doc -> second-score map. For a phrase the map is what the oracle's PositionsIndex.phrase_search returns with k = max_doc and
no live docs: every doc the phrase scorer lands on, with the reference's score bits - the rescorer advances that very scorer from hit
to hit (iterative_rescore, :229-298) and consults no live docs.

First-pass rows are hand-made: chosen docs, distinct f32 scores, best first.

Fixtures:
  membership()   three terms of the three kinds the candidate kernel tells apart - S: df 1 (a singleton, kept in the term dictionary
                 entry), T: df 40 (a VInt tail of docs only), B: df 129 (one full block of 128 docs and a tail of one) - and one
                 absent term; docs designed to sit on every side of "every term holds the doc" (DESIGN)
  wide()         500 short docs over a small vocabulary: hundreds of hits for rows of up to 200 hits, phrases of two, three and
                 seven distinct terms, "a b a"
The ladder cases (10 | 11, 128 | 129, 1025 positions, pools of 256 | 257) are those of tests/phrase_spectrum.py."""
from collections import namedtuple

import numpy as np

AVG, MAX, MIN, TOTAL, MULTIPLY = range(5)
MODES = (AVG, MAX, MIN, TOTAL, MULTIPLY)
WINDOW_CAP = 128          # rgpu_rescore_batch and rgpu_rescore_phrase_batch clip a window at min(window_size, k, 128)
UNSUPPORTED, ILLEGAL_ARGUMENT, ILLEGAL_STATE = -5, -2, -1

CANDIDATES = "k_rescore_phrase_candidates"
COMBINE = "k_rescore_phrase_combine"
SORT = "k_rescore_sort"
NEVER = ("k_search_and(phrase candidates)", "k_phrase_collect", "k_sloppy_groups", "k_sloppy_rpt_lanes")

f32 = np.float32


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def combine(mode, first, second):
    """RescoreMode::combine (rescorer.rs:96-116) in f32."""
    a, b = f32(first), f32(second)
    if mode == AVG:
        return f32(f32(a + b) / f32(2.0))
    if mode == MAX:
        return a if a >= b else b
    if mode == MIN:
        return a if a <= b else b
    if mode == TOTAL:
        return f32(a + b)
    return f32(a * b)


def rescore_ref(row, second, window, query_weight, rescore_weight, mode):
    """row: [(doc, first score)] best first; second: {doc: second score} of the docs the second query matches. Returns the rescored
    [(doc, f32 score)]: the first `window` hits combined (a doc outside the map takes first * query_weight) and sorted score
    descending, doc ascending; the hits behind them in their order, score * query_weight."""
    qw, rw = f32(query_weight), f32(rescore_weight)
    n = min(len(row), int(window))
    head = []
    for doc, score in row[:n]:
        first = f32(f32(score) * qw)
        head.append((int(doc), combine(mode, first, f32(f32(second[doc]) * rw)) if doc in second else first))
    head.sort(key=lambda h: (-float(h[1]), h[0]))
    return head + [(int(doc), f32(f32(score) * qw)) for doc, score in row[n:]]


def as_hits(rows, k):
    """[(doc, score)] lists -> the [n][k] hit array of the C ABI (unused slots {-1, 0})."""
    from rucene_amd import _lib as gpu
    out = np.zeros((len(rows), k), dtype=gpu.HIT_DTYPE)
    out["doc"] = -1
    for i, row in enumerate(rows):
        assert len(row) <= k
        for j, (d, s) in enumerate(row):
            out[i, j] = (d, s)
    return out


def assert_rows(got, want, what):
    """got: one row of the hit array; want: rescore_ref's list. Docs and score bits equal, the rest of the row unused."""
    n = len(want)
    wd = np.array([d for d, _ in want], dtype=np.int32)
    ws = np.array([s for _, s in want], dtype=np.float32)
    assert got["doc"][:n].tolist() == wd.tolist(), (what, got["doc"][:n].tolist(), wd.tolist())
    assert got["score"][:n].view(np.uint32).tolist() == ws.view(np.uint32).tolist(), (what, got["score"][:n].tolist(), ws.tolist())
    assert (got["doc"][n:] == -1).all(), what


def make_row(docs, seed, lo=0.5, hi=9.0):
    """A first-pass row over `docs` in the given order: distinct f32 scores, descending."""
    rng = np.random.default_rng(seed)
    scores = np.sort(rng.uniform(lo, hi, size=4 * len(docs) + 4).astype(np.float32))[::-1]
    scores = scores[::4][:len(docs)]
    assert np.unique(scores).size == len(docs)
    return [(int(d), f32(s)) for d, s in zip(docs, scores)]


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
class Fixture:
    """holdings: {doc: {term: [positions]}} -> postings per term, norms, the FieldReader statistics."""

    def __init__(self, name, max_doc, n_terms, holdings, seed, norms=True):
        self.name, self.max_doc = name, max_doc
        self.postings = [[] for _ in range(n_terms)]
        for d in sorted(holdings):
            assert 0 <= d < max_doc
            for t, ps in sorted(holdings[d].items()):
                assert list(ps) == sorted(set(ps)) and ps[0] >= 0
                self.postings[t].append((d, [int(p) for p in ps]))
        rng = np.random.default_rng(seed)
        self.norms = rng.integers(95, 125, size=max_doc).astype(np.uint8) if norms else None
        self.doc_count = len(holdings)
        self.sum_ttf = sum(len(ps) for pl in self.postings for _, ps in pl)

    def docs_of(self, term):
        return [d for d, _ in self.postings[term]]

    def index(self, oracle, version=1, woven=False):
        """woven: the field also stores offsets and payloads (a third file; the trailing VInt blocks carry them between the deltas)."""
        if not woven:
            return oracle.PositionsIndex(self.max_doc, self.postings, version=version)
        postings = [[(d, ps, [(10 * p, 10 * p + 5) for p in ps], [bytes([p % 251]) * (1 + p % 3) for p in ps]) for d, ps in pl] for pl in self.postings]
        return oracle.PositionsIndex(self.max_doc, postings, version=version, offsets=True, payloads=True)

    def second(self, ix, terms, slop=0, positions=None, boost=1.0, stats=None, doc_base=0):
        """{doc: second score} of a phrase: every doc the oracle's phrase scorer matches in this leaf. stats: (max_doc, doc_count,
        sum_total_term_freq) of the collection when this leaf is one of several (its own by default). boost: the oracle scores with
        boost 1; a boost of 0 makes the phrase's weight idf * 0 = 0 and with it every score weight * tf-part = +0.0, the docs stay."""
        assert boost in (0.0, 1.0)
        max_doc, doc_count, sum_ttf = stats or (self.max_doc, self.doc_count, self.sum_ttf)
        docs, scores, total = ix.phrase_search(terms, self.max_doc, self.norms, max_doc, doc_count, sum_ttf, offsets=positions, slop=slop, live_docs=None)
        assert total == docs.size
        return {int(d) + doc_base: (f32(s) if boost else f32(0.0)) for d, s in zip(docs, scores)}


S, T, B, ABSENT, OTHER = 0, 1, 2, 3, 4
B_DOCS = [10 + 2 * i for i in range(129)]                  # 10 .. 266: posting 127 is doc 264, posting 128 (the tail) doc 266
T_ONLY = [21, 270] + [31 + 2 * i for i in range(33)]       # odd docs (and 270, behind B's last doc): T without B
T_DOCS = sorted([20, 30, 100, 264, 266] + T_ONLY)          # df 40
# what the docs of the side-by-side row are there for (phrase [T, B]; rarest term T, most frequent B)
DESIGN = {"match-block-last": 264, "match-tail-only": 266, "match": 100, "terms-no-phrase": 30, "lacks-rarest": 40, "lacks-most-frequent": 21,
          "below-first-postings": 5, "above-last-postings": 280, "below-rarest-first": 12, "above-most-frequent-last": 270}
MATCHES = (100, 264, 266)
SINGLETON_DOC = 100


def _membership_holdings(match_docs=MATCHES):
    h = {}
    for d in B_DOCS:
        h.setdefault(d, {})[B] = [7] if d in match_docs else [7 + d % 3]   # (deltas that differ: packed position blocks)
    for d in T_DOCS:
        h.setdefault(d, {})[T] = [6] if d in match_docs else [3]
    h[SINGLETON_DOC][S] = [5]
    for d in (5, 280, 299):                                # docs that hold none of the phrase's terms
        h.setdefault(d, {})[OTHER] = [0]
    return h


_built = {}


def membership(norms=True):
    key = ("membership", norms)
    if key not in _built:
        _built[key] = Fixture("membership", 300, 5, _membership_holdings(), 11, norms=norms)
    return _built[key]


def side_by_side_row(seed=1):
    return make_row(list(DESIGN.values()), seed)


# three leaves: the membership fixture (the statistics leaf: the first leaf of the largest max_doc), the same docs with other
# matches and norms (so the terms' doc freqs are the statistics leaf's, which is what the phrase's weight is computed from in
# every leaf), and a leaf that lacks T. doc_base 0, 300, 600.
LEAF1_MATCHES = (20, 30, 266)
LEAF_BASES = (0, 300, 600)


def leaves():
    if "leaves" not in _built:
        h2 = {d: {B: [7]} for d in B_DOCS[:60]}
        h2[3] = {OTHER: [0]}
        _built["leaves"] = (membership(), Fixture("leaf1", 300, 5, _membership_holdings(LEAF1_MATCHES), 12), Fixture("leaf2", 200, 5, h2, 13))
    return _built["leaves"]


# wide(): 500 docs of 6 .. 9 tokens over terms 0 .. 2 (no term more than 9 times in a doc: the 64-candidate kernels answer); every
# fifth doc also reads terms 3 .. 9 in a row from position 20 on, every tenth with two neighbours swapped, every twentieth with one
# of them missing.
WIDE_DOCS, SEVEN = 500, [3, 4, 5, 6, 7, 8, 9]


def wide():
    if "wide" not in _built:
        rng = np.random.default_rng(77)
        h = {}
        for d in range(WIDE_DOCS):
            toks = rng.integers(0, 3, size=int(rng.integers(6, 10))).tolist()
            where = {}
            for p, t in enumerate(toks):
                where.setdefault(t, []).append(p)
            if d % 5 == 0:
                run = list(SEVEN)
                if d % 10 == 0:
                    run[2], run[3] = run[3], run[2]
                if d % 20 == 0:
                    run = run[:5] + run[6:]
                for p, t in enumerate(run):
                    where.setdefault(t, []).append(20 + p)
            h[d] = where
        _built["wide"] = Fixture("wide", WIDE_DOCS, 10, h, 78)
    return _built["wide"]


def wide_rows(n_rows, n_hits, seed):
    """n_rows rows of n_hits distinct docs of wide() each."""
    rng = np.random.default_rng(seed)
    return [make_row(rng.choice(WIDE_DOCS, size=n_hits, replace=False).tolist(), seed * 1000 + i) for i in range(n_rows)]


Phrase = namedtuple("Phrase", "terms slop")
WIDE_PHRASES = [Phrase([0, 1], 0), Phrase([1, 2, 0], 0), Phrase([0, 1, 0], 0), Phrase([0, 1], 1), Phrase([2, 0], 2), Phrase([0, 1, 2], 1),
                Phrase([2, 1, 0], 2), Phrase(SEVEN, 2), Phrase(SEVEN, 0)]


def leaf_of(ix, fx, doc_base=0, live_docs=None, woven=False):
    """The oracle writer's files as a rucene_amd.LeafReader with its positions (and, woven, its third file) attached."""
    import rucene_amd
    from rucene_amd import _lib as gpu
    doc_bytes, pos_bytes = ix.files()
    n = len(fx.postings)
    terms = np.zeros(n, dtype=gpu.TERM_STATE_DTYPE)
    tpos = np.zeros(n, dtype=gpu.TERM_POSITIONS_DTYPE)
    for t in range(n):
        st = ix.term_state(t)
        terms[t] = (st["doc_start_fp"], st["skip_offset"], st["total_term_freq"], st["doc_freq"], st["singleton_doc_id"])
        tpos[t]["pos_start_fp"], tpos[t]["last_pos_block_offset"] = st["pos_start_fp"], st["last_pos_block_offset"]
        if woven:
            tpos[t]["pay_start_fp"] = st["pay_start_fp"]
    leaf = rucene_amd.LeafReader(np.frombuffer(doc_bytes, np.uint8), fx.norms, fx.max_doc, terms, doc_base=doc_base, live_docs=live_docs,
                                 doc_count=fx.doc_count, sum_total_term_freq=fx.sum_ttf, index_options=4 if woven else 3, has_payloads=woven)
    leaf.pos_bytes, leaf.term_positions = np.frombuffer(pos_bytes, np.uint8), tpos
    if woven:
        leaf.pay_bytes = np.frombuffer(ix.pay_file(), np.uint8)
    return leaf
