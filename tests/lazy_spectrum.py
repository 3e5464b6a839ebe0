"""Fixtures for the bitmap disjunction kernel k_or_lazy (plain Python, no GPU): one posting on each side of every threshold
rucene_amd/csrc/kernels/search_or_lazy.hpp and search_or_lazy_group (rucene_amd/csrc/rgpu_api.hip) branch on.

The MAIN leaf has max_doc 147 493 = 9 * 16384 + 37: ten 16384-doc windows, the last of 37 docs; max_doc % 32 = 5, so the last
word of every bitmap is partial. A term gets a doc bitmap (its clause is LAZY) from doc_freq max(1024, ceil(max_doc / 64)) = 2305
on, from 1024 on under or_bitmaps = 256; the four-bits-per-doc array from doc_freq 1153 on (df * 128 >= max_doc). The small leaves
(2048, 16384 and 16385 docs: one step, one whole window, a window and one doc) hold the lists that fit them, built by the same
rules, so a term id means the same shape everywhere:

  BELOW_BM, ABOVE_BM    seeded lists of 2304 | 2305 docs: walked | lazy under the default knobs
  NIB_OFF, NIB_ON       1152 | 1153 background docs: both lazy under or_bitmaps = 256, the first without the nibble array
  D0 .. D7              eight seeded lists above the default bound, doc_freq strictly descending (idf ascending); D6 and D7 just
                        above it. The six densest of a query are lazy (LZ_MAX_LAZY), the others walked
  FREQS                 a lazy list over background docs (below) with planted freqs 14, 15, 16, 254, 255, 256 and 5000, each once on
                        a doc FREQ_TOUCH (walked) holds as well and once on a doc no walked clause holds. The planted docs have the
                        LONG norm: the nibble's 15, the clamped byte and the overflow list all move their scores
  LADDER                planted into D0 .. D5, by no walked clause: for every m in 1..6 a doc held by the m lists of highest idf with
                        freq 10 on a SHORT doc (HI_m: it scores the sum of the m largest clause maxima, and sits in the `hi` half of
                        every sketch), one with freq 1 on a SHORT doc (MID_m: still `hi`) and one with freq 1 on a LONG doc (LO_m:
                        outside every sketch)
  ANCH_A .. ANCH_C      three walked lists over the same 18 ANCHOR docs: three per m, scored between max(sum of the m - 1 largest
                        maxima, MID_m) and the sum of the m largest. LADDER_K[m] is the rank of the middle one: at that k the
                        threshold lies inside bracket m, HI_m is in and MID_m, LO_m are out
  STRETCH_n             n consecutive docs and nothing else inside one 2048-doc step, n in 63, 64, 65, 128, 129, 512, 513; walked.
                        Those of 63 .. 129 stand at run lanes 7 | 8 | 13 | 15 (Leaf.run_lanes: the position among the walked clauses)
                        STRETCH_64 ends on its step's last doc, STRETCH_129 on its window's. STRETCH_512B, STRETCH_513B: 512 | 513
                        more docs in STRETCH_512's step (1024 | 1025 touched docs: either side of or_lazy_cells = 1024)
  SPLIT                 513 consecutive docs laid 256 | 257 across a step edge: each step fits 512 cells, the two together do not
  SPLIT2_A, SPLIT2_B    400 docs each in two adjacent steps: the second step's group starts at cell rank r0 = 400
  EDGE_W, EDGE_LZ       docs 0, w - 1, w, w + 1 and max_doc - 1 for every multiple w of 2048 (so of 16384 too): alone (walked) and
                        added, with high freqs, to a dense list of background docs (lazy)
  LAST_DOC,             singletons: doc max_doc - 1, doc 16384
  FIRST_OF_WINDOW
  CONST, TIE_LZ         300 docs across the window edge 16384, one norm byte, freq 3 (walked); the same docs and freq inside a lazy
                        list of background docs: every CONST doc scores the same under either query
  ABSENT                df 0
  FILL_0 .. FILL_8      100 background docs each: they fill clause positions, score next to nothing and avoid every stretch's step
  EVERY, RARE_A ..      the fixed-point floor: a list that holds every doc (idf ~ 3e-6) next to four rare lists of 3 docs each.
  RARE_D                FLOOR_HI | FLOOR_LO are ONE query, FLOOR_Q, at k = 12 | 13: the twelfth row is a rare doc far above
                        n * 2^17 fixed-point steps, the thirteenth a doc that holds EVERY alone, far below them - the brackets and
                        the or_wide_redo_queries deltas of 0 | 1 are those of two queries

Background docs are a seeded 9000 outside every planted doc and every stretch's step; they have the LONG norm, so whatever list
holds them scores them below every planted posting. Every other freq is geometric, capped at 10. Norms are rank mode: 26 seeded
bytes (97 .. 106 for the seeded docs of D0 .. D7, 101 .. 122 elsewhere), the SHORT and the LONG one, TIE_BYTE and EDGE_BYTE.

The reference next to the oracle's rows is LazyRef: hit sets by numpy set algebra over the lists, a doc's score the float64 sum of
the oracle's per-term f32 scores. tests/test_lazy_spectrum_cpu.py proves every property named here before a GPU sees any of it.

LongLeaf (4 128 805 docs = 252 * 16384 + 37: 253 windows) has a vocabulary of its own - two seeded lists just above its bitmap
bound of 64 513 and eight sparse lists that share twelve TOP docs - for the plans a small batch takes there: alone, every window
is an item of its own (256 items: the pilot launch and k_premerge_items both run); among 300 rows two windows share an item.
UNIFORM_TEN and the ten-clause LONG_QUERIES are what the fused call (one op and clause count per batch) takes."""
import numpy as np

import segment_spectrum as ss
from segment_spectrum import Query

MAX_DOC = 9 * 16384 + 37
SMALL = (2048, 16384, 16385)
WINDOW, STEP = 16384, 2048
LZ_MAX_LAZY, LZ_PREFETCH, DEFAULT_CELLS = 6, 8, 512
KS = (1, 10, 64, 65, 100, 128)
VERSIONS = (1, 0)
STTF_PER_DOC = 60
K1, B = 1.2, 0.75
SHORT, LONG, TIE_BYTE, EDGE_BYTE = 124, 96, 120, 112
D_BYTES = (97, 107)
RAW_BYTES = np.arange(30, 100, dtype=np.uint8)
PLANTED_FREQS = (14, 15, 16, 254, 255, 256, 5000)
SHARP = 1e-4     # ten times the band of oracle/parity.py's rule at rtol 1e-5

NAMES = (["BELOW_BM", "ABOVE_BM", "NIB_OFF", "NIB_ON"] + ["D%d" % i for i in range(8)] + ["FREQS", "FREQ_TOUCH", "ANCH_A", "ANCH_B", "ANCH_C"] +
         ["STRETCH_%d" % n for n in (63, 64, 65, 128, 129, 512, 513)] + ["STRETCH_512B", "STRETCH_513B", "SPLIT", "SPLIT2_A", "SPLIT2_B", "EDGE_W",
         "EDGE_LZ", "LAST_DOC", "FIRST_OF_WINDOW", "CONST", "TIE_LZ", "ABSENT"] + ["FILL_%d" % i for i in range(9)] + ["EVERY", "RARE_A", "RARE_B", "RARE_C", "RARE_D"])
(BELOW_BM, ABOVE_BM, NIB_OFF, NIB_ON, D0, D1, D2, D3, D4, D5, D6, D7, FREQS, FREQ_TOUCH, ANCH_A, ANCH_B, ANCH_C, STRETCH_63, STRETCH_64, STRETCH_65,
 STRETCH_128, STRETCH_129, STRETCH_512, STRETCH_513, STRETCH_512B, STRETCH_513B, SPLIT, SPLIT2_A, SPLIT2_B, EDGE_W, EDGE_LZ, LAST_DOC, FIRST_OF_WINDOW,
 CONST, TIE_LZ, ABSENT, FILL_0, FILL_1, FILL_2, FILL_3, FILL_4, FILL_5, FILL_6, FILL_7, FILL_8, EVERY, RARE_A, RARE_B, RARE_C, RARE_D) = range(len(NAMES))
N_TERMS = len(NAMES)
DS = (D0, D1, D2, D3, D4, D5, D6, D7)
D_DFS = (30000, 21000, 15000, 11000, 8000, 6000, 2600, 2400)    # before the ladder's postings are added to D0 .. D5
FILLS = (FILL_0, FILL_1, FILL_2, FILL_3, FILL_4, FILL_5, FILL_6, FILL_7, FILL_8)
ANCHS = (ANCH_A, ANCH_B, ANCH_C)
LONG_RUNS = (STRETCH_63, STRETCH_64, STRETCH_65, STRETCH_128, STRETCH_129)
RARES = (RARE_A, RARE_B, RARE_C, RARE_D)
# (first doc, length) on MAIN, each inside one 2048-doc step: 5 * 2048 + 1984 + 64 = 6 * 2048, 32639 + 129 = 2 * 16384
STRETCHES = {STRETCH_63: (3 * STEP + 100, 63), STRETCH_64: (5 * STEP + 1984, 64), STRETCH_65: (11 * STEP, 65), STRETCH_128: (9 * STEP + 500, 128),
             STRETCH_129: (2 * WINDOW - 129, 129), STRETCH_512: (20 * STEP, 512), STRETCH_513: (22 * STEP, 513),
             STRETCH_512B: (20 * STEP + 512, 512), STRETCH_513B: (20 * STEP + 1024, 513)}
SPLIT_AT = 30 * STEP                                             # SPLIT: [SPLIT_AT - 256, SPLIT_AT + 257)
SPLIT2 = {SPLIT2_A: (40 * STEP + 1000, 400), SPLIT2_B: (41 * STEP + 100, 400)}
CONST_LO, CONST_HI, CONST_FREQ = WINDOW - 150, WINDOW + 150, 3
RESERVED_STEPS = (3, 5, 9, 11, 15, 20, 22, 29, 30, 40, 41)
N_BACKGROUND = 9000

_EMPTY = (np.zeros(0, np.int32), np.zeros(0, np.int32))


def bitmap_bound(max_doc, or_bitmaps=0):
    """The smallest doc_freq that gets a doc bitmap (bitmap_min_df of rgpu_api.hip, written out again)."""
    den = 64 if or_bitmaps == 0 else or_bitmaps
    return max(1024, -(-max_doc // den))


def nibble_bound(max_doc):
    """... and the four-bits-per-doc array: df * 128 >= max_doc."""
    return -(-max_doc // 128)


def idf(df, max_doc):
    """BM25's idf as the definition has it (bm25_similarity.rs: ln(1 + (N - n + 0.5) / (n + 0.5))), not read from any library."""
    return float(np.log(1.0 + (max_doc - df + 0.5) / (df + 0.5)))


def norm_cache(byte):
    """k1 * (1 - b + b * len / avgdl) for the doc length the norm byte stands for (SmallFloat byte315, length = 1 / f^2)."""
    f = np.array([((int(byte) & 0xff) << 21) + ((63 - 15) << 24)], np.uint32).view(np.float32)[0]
    return K1 * ((1.0 - B) + B * (1.0 / (float(f) * float(f))) / STTF_PER_DOC)


def bm25(df, max_doc, freq, byte):
    return idf(df, max_doc) * (K1 + 1.0) * freq / (freq + norm_cache(byte))


def _freqs(rng, n, cap=10):
    return np.minimum(cap, rng.geometric(0.5, size=n)).astype(np.int32)


def edge_docs(max_doc):
    d = {0, max_doc - 1}
    for w in range(STEP, max_doc, STEP):
        d.update((w - 1, w, w + 1))
    return np.array(sorted(x for x in d if 0 <= x < max_doc), np.int32)


def _merge(parts):
    """[(docs, freqs)] with disjoint docs -> one list in doc order."""
    d = np.concatenate([np.asarray(p[0], np.int32) for p in parts])
    f = np.concatenate([np.asarray(p[1], np.int32) for p in parts])
    assert np.unique(d).size == d.size
    o = np.argsort(d, kind="stable")
    return d[o], f[o]


class _Built:
    """Lists, norms, planted docs and .doc bytes of one (max_doc, version)."""

    def __init__(self, max_doc, version, raw=False):
        from rucene_amd import indexgen
        main = max_doc == MAX_DOC
        rng = np.random.default_rng([max_doc, 11])
        every = np.arange(max_doc, dtype=np.int32)
        lists = [_EMPTY] * N_TERMS
        edges = edge_docs(max_doc)
        reserved = np.zeros(max_doc, bool)       # no seeded list draws from these
        in_steps = np.zeros(max_doc, bool)       # the stretches' steps: background docs and fillers stay out
        reserved[edges] = True
        if main:
            reserved[CONST_LO:CONST_HI] = True
            for s in RESERVED_STEPS:
                in_steps[s * STEP:(s + 1) * STEP] = True
        free = np.flatnonzero(~reserved & ~in_steps)
        n_points = 18 + 18 + 14 + 12
        points = np.sort(rng.choice(free, size=n_points if main else 0, replace=False)).astype(np.int32)
        rng.shuffle(points)
        reserved[points] = True
        self.ladder = {(kind, m): int(points[3 * (m - 1) + j]) for m in range(1, 7) for j, kind in enumerate(("hi", "mid", "lo"))} if main else {}
        self.anchors = {(m, j): int(points[18 + 3 * (m - 1) + j]) for m in range(1, 7) for j in range(3)} if main else {}
        self.freq_docs = {(f, where): int(points[36 + 2 * i + j]) for i, f in enumerate(PLANTED_FREQS) for j, where in enumerate(("touched", "lazy"))} if main else {}
        rare = points[50:62] if main else np.zeros(0, np.int32)
        free = np.flatnonzero(~reserved & ~in_steps)
        background = np.sort(rng.choice(free, size=N_BACKGROUND if main else 0, replace=False)).astype(np.int32)
        seeded_from = np.flatnonzero(~reserved)   # the seeded lists may enter the stretches' steps: a stretch doc inside a lazy list

        def plain(docs):
            docs = np.asarray(docs, np.int32)
            return docs, _freqs(rng, docs.size)

        def drawn(df, pool=seeded_from):
            return plain(np.sort(rng.choice(pool, size=df, replace=False))) if df <= pool.size else _EMPTY

        bound = bitmap_bound(MAX_DOC)
        lists[BELOW_BM], lists[ABOVE_BM] = drawn(bound - 1), drawn(bound)
        nib_pool = background if main else seeded_from
        lists[NIB_OFF], lists[NIB_ON] = drawn(nibble_bound(MAX_DOC) - 1, nib_pool), drawn(nibble_bound(MAX_DOC), nib_pool)
        for t, df in zip(DS, D_DFS):
            lists[t] = drawn(df)
        lists[LAST_DOC] = plain([max_doc - 1])
        lists[FIRST_OF_WINDOW] = plain([WINDOW]) if max_doc > WINDOW else _EMPTY
        lists[EDGE_W] = plain(edges)
        lists[EVERY] = plain(every)
        norms = rng.integers(101, 123, size=max_doc).astype(np.uint8)
        # the seeded docs of D0 .. D7 are long (256 tokens and more): of the thousands that several of these lists hold, none scores
        # its way in between the ladder's docs and the anchors
        in_d = np.unique(np.concatenate([lists[t][0] for t in DS]))
        norms[in_d] = rng.integers(D_BYTES[0], D_BYTES[1], size=in_d.size).astype(np.uint8)
        norms[edges] = EDGE_BYTE
        if main:
            # the ladder: HI_m, MID_m and LO_m in the m lists of highest idf among D0 .. D5 (D5, D4, ...)
            for m in range(1, 7):
                for kind, freq, byte in (("hi", 10, SHORT), ("mid", 1, SHORT), ("lo", 1, LONG)):
                    doc = self.ladder[(kind, m)]
                    norms[doc] = byte
                    for t in DS[6 - m:6]:
                        lists[t] = _merge([lists[t], ([doc], [freq])])
            norms[background] = LONG
            # FREQS: 3000 background docs and the planted postings; FREQ_TOUCH: the "touched" half of those docs, freq 1
            planted = sorted((doc, f) for (f, _), doc in self.freq_docs.items())
            lists[FREQS] = _merge([plain(rng.choice(background, size=3000, replace=False)), ([d for d, _ in planted], [f for _, f in planted])])
            touched = sorted(doc for (_, where), doc in self.freq_docs.items() if where == "touched")
            lists[FREQ_TOUCH] = (np.array(touched, np.int32), np.ones(len(touched), np.int32))
            norms[[d for d, _ in planted]] = LONG
            for t, (first, n) in list(STRETCHES.items()) + list(SPLIT2.items()):
                lists[t] = plain(first + every[:n])
            lists[SPLIT] = plain(SPLIT_AT - 256 + every[:513])
            # the window edges' docs stand out of EDGE_LZ's step edges, and both out of its background
            at_window = np.isin(edges, [0, max_doc - 1]) | (np.minimum(edges % WINDOW, WINDOW - edges % WINDOW) <= 1)
            ef = np.where(at_window, 1000 - 30 * np.cumsum(at_window), 12 + np.arange(edges.size) % 90).astype(np.int32)
            lists[EDGE_LZ] = _merge([plain(rng.choice(background, size=3000, replace=False)), (edges, ef)])
            const = every[CONST_LO:CONST_HI]
            lists[CONST] = (const.copy(), np.full(const.size, CONST_FREQ, np.int32))
            lists[TIE_LZ] = _merge([plain(rng.choice(background, size=2400, replace=False)), (const, np.full(const.size, CONST_FREQ, np.int32))])
            norms[const] = TIE_BYTE
            for t in FILLS:
                lists[t] = drawn(100, background)
            for i, t in enumerate(RARES):
                lists[t] = (np.sort(rare[3 * i:3 * i + 3]), np.array([3, 2, 1], np.int32))
            # the anchors: three per bracket, spread inside it; each is held by ANCH_A, ANCH_B and ANCH_C with one freq, and its
            # norm byte and that freq are the pair whose BM25 score (by the formula) comes closest to the level wanted
            df_a = 18
            maxima = sorted((bm25(lists[t][0].size, max_doc, 10, SHORT) for t in DS[:6]), reverse=True)
            mid_ratio = (1.0 / (1.0 + norm_cache(SHORT))) / (10.0 / (10.0 + norm_cache(SHORT)))
            choices = [(3.0 * bm25(df_a, max_doc, f, byte), f, byte) for f in range(1, 200) for byte in range(101, 123)]
            rows = []
            for m in range(1, 7):
                hi = sum(maxima[:m])
                lo = max(sum(maxima[:m - 1]), hi * mid_ratio)
                for j, frac in enumerate((0.7, 0.5, 0.3)):
                    want = lo + (hi - lo) * frac
                    _, f, byte = min(choices, key=lambda c: abs(c[0] - want))
                    doc = self.anchors[(m, j)]
                    norms[doc] = byte
                    rows.append((doc, f))
            rows.sort()
            for t in ANCHS:
                lists[t] = (np.array([d for d, _ in rows], np.int32), np.array([f for _, f in rows], np.int32))
        if raw:   # 70 distinct bytes on docs no property depends on: raw mode, which keeps the fixed-point kernels away
            plain_docs = np.flatnonzero(~reserved & ~in_steps & ~np.isin(every, background))
            norms[plain_docs[:7000]] = np.tile(RAW_BYTES, 100)
        self.max_doc, self.lists, self.norms, self.edges, self.background = max_doc, lists, norms, edges, background
        self.seg = indexgen.build_explicit(max_doc, lists, norms=norms, version=version)
        self.has = np.zeros((N_TERMS, max_doc), bool)
        for t, (d, _) in enumerate(lists):
            self.has[t, d] = True
        assert [int(x) for x in self.seg.terms["doc_freq"]] == [d.size for d, _ in lists]


_built = {}


class Leaf:
    """One fixture leaf; the attributes tests/segment_spectrum.py's Leaf has, so that its set algebra takes it. live: "none", or
    "one" - a single doc deleted (enough to keep the fixed-point kernels away); raw: 70 more norm bytes (raw mode: the same)."""

    def __init__(self, max_doc=MAX_DOC, version=1, live="none", raw=False):
        key = (max_doc, version, raw)
        if key not in _built:
            _built[key] = _Built(max_doc, version, raw)
        self.built = b = _built[key]
        self.key = key + (live,)
        self.max_doc, self.lists, self.norms, self.seg, self.has = max_doc, b.lists, b.norms, b.seg, b.has
        self.version, self.doc_base, self.sttf = version, 0, STTF_PER_DOC * max_doc
        self.alive = np.ones(max_doc, bool)
        if live == "one":
            self.alive[max_doc // 2] = False
        self.live_docs = None if live == "none" else ss.live_words(self.alive)

    def oracle_segment(self, oracle):
        return oracle.Segment(self.seg.doc_bytes, self.norms, self.max_doc, self.seg.terms, doc_base=0, live_docs=self.live_docs,
                              sum_total_term_freq=self.sttf)

    def df(self, t):
        return int(self.lists[t][0].size)

    def run_lanes(self, q, or_bitmaps=0):
        """{clause position: run lane} of q's walked clauses, as search_or_lazy_group fills run_of: the clauses with a scorer in
        clause order, without the (up to six) densest clause instances at or above the bound - ties to the earlier clause."""
        bound = bitmap_bound(self.max_doc, or_bitmaps)
        live = [i for i, t in enumerate(q.should) if self.df(t) > 0]
        lazy = sorted((i for i in live if self.df(q.should[i]) >= bound), key=lambda i: -self.df(q.should[i]))[:LZ_MAX_LAZY]
        return {i: lane for lane, i in enumerate(i for i in live if i not in lazy)}

    def lazy_terms(self, q, or_bitmaps=0):
        """The distinct terms search_or_lazy_group meets through a bitmap: the (up to six) densest clauses at or above the bound."""
        bound = bitmap_bound(self.max_doc, or_bitmaps)
        dense = sorted((t for t in q.should if self.df(t) >= bound), key=lambda t: -self.df(t))[:LZ_MAX_LAZY]
        return sorted(set(dense))

    def bitmap_terms(self, queries, or_bitmaps=0):
        """The distinct terms that get a bitmap once these queries ran: every clause at or above the bound."""
        bound = bitmap_bound(self.max_doc, or_bitmaps)
        return sorted({t for q in queries for t in q.should if self.df(t) >= bound})


# ---- queries (MAIN) -----------------------------------------------------------------------------------------------------------------
def _fill(n, special, pool=FILLS):
    """n SHOULD clauses: `special` {index: term}, the fillers in turn everywhere else."""
    free = [t for t in pool if t not in special.values()]
    out, j = [], 0
    for i in range(n):
        if i in special:
            out.append(special[i])
        else:
            out.append(free[j % len(free)])
            j += 1
    return tuple(out)


def Q(*terms, n=10):
    """The terms first, fillers up to n clauses."""
    return Query(should=_fill(max(n, len(terms)), dict(enumerate(terms))))


LADDER_Q = Query(should=(D0, D1, D2, D3, D4, D5, ANCH_A, ANCH_B, ANCH_C, FILL_0))
FREQS_Q = {"nibble": Q(FREQS, FREQ_TOUCH),                         # one lazy clause with the nibble array: the fast path, left on a 15
           "general": Q(FREQS, FREQ_TOUCH, NIB_OFF, NIB_ON)}       # under or_bitmaps = 256 NIB_OFF is lazy without one: all_nib false
EDGE_Q = {"lazy": Q(EDGE_LZ), "both": Q(EDGE_LZ, EDGE_W), "walked": Q(D0, EDGE_W, LAST_DOC, FIRST_OF_WINDOW)}
TIE_Q = {"walked": Q(CONST), "both": Q(CONST, TIE_LZ)}
TIE_KS = (1, 10, 64, 65, 128)
BAIL_Q = {512: (Q(D0, STRETCH_512), Q(D0, STRETCH_513)),           # (fits, bails) by the cells of a context
          1024: (Q(D0, STRETCH_512, STRETCH_512B), Q(D0, STRETCH_512, STRETCH_513B))}
FLOOR_Q = Query(should=RARES + (EVERY,) * 6)                       # six copies of EVERY are lazy: nothing is walked but the rare lists
FLOOR_K = {"hi": 12, "lo": 13}                                     # the twelve rare docs, far above the floor | a doc that holds EVERY alone


def _families():
    fam = {}
    fam["bounds"] = [Q(BELOW_BM, ABOVE_BM), Q(NIB_OFF, NIB_ON), Q(NIB_ON, ABOVE_BM), Q(BELOW_BM, NIB_OFF)]
    # 0, 1, 4, 5, 6, 7 and 8 of D0 .. D7: none (the empty bitmap), NC = 4 | 6, LZ_MAX_LAZY, the 7th and 8th densest walked
    fam["dense"] = [Q(BELOW_BM, EDGE_W, LAST_DOC), Q(D3), Q(D0, D2, D5, D7), Q(D0, D1, D3, D5, D6), Q(*DS[:6]), Q(*DS[:7]), Q(*DS), Q(*DS, n=16),
                    Query(should=(D4,) * 6 + FILLS[:4]), Query(should=(D4,) * 10), Q(D7, D6, D5, D4, D3, D2, D1, D0, ABOVE_BM, NIB_ON, n=16)]
    fam["freqs"] = list(FREQS_Q.values())
    fam["ladder"] = [LADDER_Q, Query(should=LADDER_Q.should[::-1]), Query(should=LADDER_Q.should + (D6, D7))]
    st = {}
    # a clause's RUN LANE is its position among the walked clauses (the kernel's lane t; lazy clauses take none), so the lazy lists
    # stand last: lanes 7 | 8 (the last prefetched head | the first clause without one), two stretches at 7 and 8, lane 15 of sixteen
    # walked clauses (nothing dense) and the last lane, 13, next to two lazy lists
    wide_pool = FILLS + (EDGE_W, LAST_DOC, FIRST_OF_WINDOW, FREQ_TOUCH, BELOW_BM, ANCH_A)
    for i, t in enumerate(LONG_RUNS):
        other = LONG_RUNS[(i + 1) % len(LONG_RUNS)]
        st[t] = [Query(should=_fill(10, {7: t, 9: D0})), Query(should=_fill(10, {8: t, 9: D0})), Query(should=_fill(16, {15: t}, wide_pool)),
                 Query(should=_fill(12, {7: t, 8: other, 11: D2})), Query(should=_fill(16, {13: t, 14: D3, 15: D1}))]
    fam["stretch"] = [q for qs in st.values() for q in qs]
    fam["split"] = [Q(D0, SPLIT), Q(D0, SPLIT2_A, SPLIT2_B), Q(D1, D4, SPLIT, SPLIT2_A, SPLIT2_B, STRETCH_129), Q(BELOW_BM, SPLIT, SPLIT2_B)]
    fam["edge"] = list(EDGE_Q.values()) + [Q(EDGE_LZ, D0, D5, EDGE_W, LAST_DOC), Q(D6, LAST_DOC, FIRST_OF_WINDOW)]
    fam["tie"] = list(TIE_Q.values())
    # ABSENT takes no clause position; the same walked term twice, three times (one run for the batch), next to a lazy one twice
    fam["absent"] = [Q(D0, ABSENT, EDGE_W, n=11), Q(ABSENT, ABSENT, D2, D6, n=12), Query(should=(D0, EDGE_W, EDGE_W) + FILLS[:7]),
                     Query(should=(D1, D1, BELOW_BM, BELOW_BM, BELOW_BM) + FILLS[:5]), Query(should=(D3, FILL_0, FILL_0, FILL_1, FILL_1) + FILLS[2:7])]
    return fam


FAMILIES = _families()
ALL_QUERIES = list(dict.fromkeys(q for fam in FAMILIES.values() for q in fam))
UNIFORM_TEN = [q for q in ALL_QUERIES if len(q.should) == 10 and ABSENT not in q.should] + [BAIL_Q[512][1], FLOOR_Q]
EIGHT = [FAMILIES["dense"][2], FAMILIES["dense"][4], FAMILIES["dense"][6], LADDER_Q, FREQS_Q["nibble"], EDGE_Q["both"], FAMILIES["stretch"][9], FAMILIES["split"][2]]


def small_queries(leaf):
    """What a small leaf can hold: the lists that fit it (a longer one is absent there), in ten-clause queries."""
    present = [t for t in range(N_TERMS) if leaf.df(t) > 0]
    dense = [t for t in present if leaf.df(t) >= bitmap_bound(leaf.max_doc)]
    sparse = [t for t in present if t not in dense]
    assert len(sparse) >= 2
    return [Query(should=tuple((dense[:n] + sparse * 10)[:10])) for n in (0, 1, 2, len(dense))]


def oracle_rows(oracle, osr, queries, k):
    return ss.oracle_rows(oracle, osr, queries, k)


# ---- the numpy reference ------------------------------------------------------------------------------------------------------------
def ref_docs(leaf, q):
    """Docs that match q, ascending: set algebra over the input lists and the live mask."""
    return ss.ref_leaf_docs(leaf, q)


class LazyRef:
    """Hit sets by set algebra; a doc's score the float64 sum of the oracle's f32 TermScorer scores (Searcher.score_docs with OP_TERM)
    of the SHOULD clauses that hold it - a clause given twice counts twice."""

    def __init__(self, oracle, leaf, osr=None):
        self.oracle, self.leaf = oracle, leaf
        self.osr = osr or oracle.Searcher([leaf.oracle_segment(oracle)])
        self._clauses, self._scores = {}, {}

    def clause(self, t):
        """-> (live docs of the list, the oracle's f32 score of each)."""
        if t not in self._clauses:
            docs = self.leaf.lists[t][0]
            docs = docs[self.leaf.alive[docs]].astype(np.int32)
            scores, matched = self.osr.score_docs(self.oracle.OP_TERM, [t], docs)
            assert matched.all(), ("the oracle's TermScorer does not hold a live doc of the fixture's list", t)
            scores.setflags(write=False)
            self._clauses[t] = (docs, scores)
        return self._clauses[t]

    def clause_max(self, t):
        return float(self.clause(t)[1].max())

    def scores(self, q):
        """-> (matching docs ascending, their float64 sums)."""
        if q not in self._scores:
            total = np.zeros(self.leaf.max_doc, np.float64)
            for t in q.should:
                d, s = self.clause(t)
                total[d] += s.astype(np.float64)
            docs = ref_docs(self.leaf, q)
            out = (docs.astype(np.int32), total[docs])
            for a in out:
                a.setflags(write=False)
            self._scores[q] = out
        return self._scores[q]

    def ranking(self, q):
        """Every matching doc, score descending, doc ascending -> (docs, float64 scores)."""
        docs, sc = self.scores(q)
        order = np.lexsort((docs, -sc))
        return docs[order], sc[order]

    def row(self, q, k):
        docs, sc = self.ranking(q)
        return docs[:k], sc[:k], int(docs.size)

    def score_with(self, q, doc, t, freq):
        """The doc's sum with term t's posting scored at another freq (by BM25 scaled from the oracle's own score of the posting)."""
        docs, sc = self.scores(q)
        d, s = self.clause(t)
        at = int(np.searchsorted(d, doc))
        assert d[at] == doc
        real = int(self.leaf.lists[t][1][np.searchsorted(self.leaf.lists[t][0], doc)])
        c = norm_cache(self.leaf.norms[doc])
        ratio = (freq / (freq + c)) / (real / (real + c))
        return float(sc[np.searchsorted(docs, doc)]) + q.should.count(t) * float(s[at]) * (ratio - 1.0)

    def gap(self, q, k):
        """Relative distance of the k-th and the (k + 1)-th score (inf when fewer than k + 1 docs match)."""
        _, sc = self.ranking(q)
        return float("inf") if sc.size <= k else float((sc[k - 1] - sc[k]) / sc[k - 1])

    def is_sharp(self, q, k):
        return self.gap(q, k) > SHARP

    def separated(self, q, k):
        """Positions of the k-row whose neighbours on both sides (the (k + 1)-th doc included) are further than SHARP away."""
        _, sc = self.ranking(q)
        n = min(k, sc.size)
        rel = (sc[:-1] - sc[1:]) / sc[:-1] if sc.size > 1 else np.zeros(0)
        ok = np.ones(n, bool)
        ok[1:] &= rel[:n - 1] > SHARP
        ok[:min(n, rel.size)] &= rel[:n] > SHARP
        return np.flatnonzero(ok)


def ladder_ks(ref):
    """{m: k}: the rank of bracket m's middle anchor in LADDER_Q's ranking."""
    docs, _ = ref.ranking(LADDER_Q)
    return {m: int(np.flatnonzero(docs == ref.leaf.built.anchors[(m, 1)])[0]) + 1 for m in range(1, 7)}


# ---- the long leaf ------------------------------------------------------------------------------------------------------------------
LONG_MAX_DOC = 252 * WINDOW + 37
LONG_L0, LONG_L1 = 0, 1
LONG_SPARSE = tuple(range(2, 10))
LONG_QUERIES = [Query(should=(LONG_L0, LONG_L1) + LONG_SPARSE), Query(should=(LONG_L1,) + LONG_SPARSE + (LONG_SPARSE[0],)),
                Query(should=LONG_SPARSE + LONG_SPARSE[:2]), Query(should=(LONG_L0,) * 3 + LONG_SPARSE)]
LONG_BATCH = 300


def long_plan(n_queries, max_doc=LONG_MAX_DOC, target=65536):
    """(items per query, windows per item) as search_or_lazy_group cuts a batch (written out again)."""
    wpq = -(-max_doc // WINDOW)
    ipq = min(wpq, max(1, -(-target // n_queries)))
    wpi = -(-wpq // ipq)
    return -(-(-(-wpq // wpi)) // 4) * 4, wpi


class LongLeaf:
    N_TERMS = 10

    def __init__(self):
        from rucene_amd import indexgen
        if "long" not in _built:
            max_doc = LONG_MAX_DOC
            rng = np.random.default_rng([max_doc, 12])
            bound = bitmap_bound(max_doc)
            top = np.sort(rng.choice(max_doc - 1, size=12, replace=False)).astype(np.int32)
            rest = np.setdiff1d(np.arange(max_doc, dtype=np.int32), top)
            lists = []
            for extra in (200, 50):        # the two lazy lists: the first four TOP docs and the last doc with freq 10
                d = np.sort(rng.choice(rest[:-1], size=bound + extra, replace=False))
                lists.append(_merge([(d, _freqs(rng, d.size)), (np.append(top[:4], max_doc - 1), np.full(5, 10, np.int32))]))
            for i in range(8):             # the sparse lists: 50 docs of their own and every TOP doc
                d = np.sort(rng.choice(rest[:-1], size=50, replace=False))
                lists.append(_merge([(d, _freqs(rng, d.size)), (top, 1 + (np.arange(12) + i) % 10)]))
            norms = rng.integers(101, 123, size=max_doc).astype(np.uint8)
            norms[top] = np.arange(101, 113, dtype=np.uint8)
            seg = indexgen.build_explicit(max_doc, lists, norms=norms)
            has = np.zeros((len(lists), max_doc), bool)
            for t, (d, _) in enumerate(lists):
                has[t, d] = True
            _built["long"] = (lists, norms, seg, has, top)
        self.lists, self.norms, self.seg, self.has, self.top = _built["long"]
        self.key = ("long",)
        self.max_doc, self.version, self.doc_base, self.sttf = LONG_MAX_DOC, 1, 0, STTF_PER_DOC * LONG_MAX_DOC
        self.alive, self.live_docs = np.ones(LONG_MAX_DOC, bool), None

    oracle_segment = Leaf.oracle_segment
    df = Leaf.df
    lazy_terms = Leaf.lazy_terms
