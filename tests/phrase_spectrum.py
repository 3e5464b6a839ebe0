"""Fixtures for the phrase kernels' ladder (tests/test_phrase_spectrum_cpu.py proves them, tests/test_gpu_phrase_spectrum.py runs
them): plain Python / numpy postings with positions, built through oracle.PositionsIndex, and a table of named cases with one doc
on every rung of the ladder in rucene_amd/csrc/kernels/search_phrase.hpp -

  positions of one term in one doc    1, 10 | 11 (the 64-candidate kernels' lists), 128 | 129 (the small lists), 1024 | 1025 (refused);
  a sloppy phrase's pool              256 | 257, 2048 | 2049 (refused), two distinct terms and one term named twice;
  terms per phrase                    6 | 7 distinct (sloppy), 1 .. 3 repetition groups, 16 | 17 (refused);
  where the positions lie             skip + freq at 127 | 128 | 129 of a packed block, with a packed, an all-equal, the trailing VInt
                                      block or nothing behind it; whole blocks of earlier docs' positions in front; singleton terms;
  16-bit lists (sloppy)               position - phrase offset at 32767 | 32768 and -32768 | -32769;
  the collector's chunks              8191 .. 16385 candidates, the first match at index 0, 8191, 8192, 8193 and n - 1.

Every rung case has terms of its own. A term's docs are: one "ordinary" doc that holds all the case's terms side by side (the
query's other candidate), filler docs that hold this term alone (they put the designed doc's positions at a chosen value of a chosen
position block and leave blocks behind it), the designed doc. place() recomputes a doc's place in a term's position stream from the
postings alone; the case table only names it.

What a query is expected to launch is restated from the documented ladder (level()): "lanes" = the 64-candidate kernel answers
every candidate, "left" = some candidate is handed on to the one-candidate kernel with the small lists / pool, "wide" = and on to the
wide lists / pool, None = the call is refused."""
from collections import namedtuple

import numpy as np

BLOCK = 128
LANE_CAP, SMALL_CAP, LIST_CAP = 10, 128, 1024       # PHRASE_LANE_CAP, PHRASE_SMALL_CAP, PHRASE_LIST_CAP
SMALL_POOL, POOL = 256, 2048                        # SLOPPY_SMALL_POOL, SLOPPY_POOL
LANE_TERMS, RPT_GROUPS, MAX_TERMS = 6, 3, 16        # SLOPPY_LANE_TERMS, SLOPPY_RPT_GROUPS, RGPU_MAX_PHRASE_TERMS
CHUNK = 8192                                        # PHRASE_COLLECT_CHUNK
PASS_K = 128                                        # above: k_phrase_collect in passes, no chunks
DEFAULT_NEXT_LIMIT = 500_000
ILLEGAL_ARGUMENT, UNSUPPORTED = -2, -5

LANES = "k_phrase_match_lanes"
LEFT = "k_phrase_match(left by the 64-candidate kernel)"
WIDE = "k_phrase_match(wide lists)"
ONE = "k_phrase_match"
S_LANES = "k_sloppy_match_lanes"
S_RPT = "k_sloppy_rpt_lanes"
S_GROUPS = "k_sloppy_groups"
S_LEFT = "k_sloppy_match(left by the 64-candidate kernel)"
S_WIDE = "k_sloppy_match(wide pool)"
S_ONE = "k_sloppy_match"
COLLECT = "k_phrase_collect"
MERGE = "k_merge_items"    # folds the chunked collector's partial lists: launched iff the chunked collector ran
EXACT_NAMES = (LANES, LEFT, WIDE, ONE)
SLOPPY_NAMES = (S_LANES, S_RPT, S_GROUPS, S_LEFT, S_WIDE, S_ONE)

# One query of a case. level: see the module docstring; rpt: the phrase names a term twice; error: the status the call is refused with.
PQ = namedtuple("PQ", "terms positions slop level rpt error")
Case = namedtuple("Case", "name rung queries designed ordinary shape")


def level(freqs, slop):
    """The documented ladder for a doc that holds the phrase's terms freqs[i] times (one entry per phrase term, a repeated term
    counted once per mention) in packed blocks: which kind of kernel answers it, None = refused."""
    if slop == 0:
        top = max(freqs)
        return "lanes" if top <= LANE_CAP else "left" if top <= SMALL_CAP else "wide" if top <= LIST_CAP else None
    if len(freqs) <= LANE_TERMS and max(freqs) <= LANE_CAP:
        return "lanes"
    return "left" if sum(freqs) <= SMALL_POOL else "wide" if sum(freqs) <= POOL else None


def launches(q, legacy=False):
    """{launch name: must it appear} for a batch that holds this query alone."""
    out = {n: False for n in EXACT_NAMES + SLOPPY_NAMES}
    out[COLLECT] = True
    if q.slop == 0:
        if legacy:
            out.update({ONE: True, WIDE: q.level == "wide"})
        else:
            out.update({LANES: True, LEFT: q.level != "lanes", WIDE: q.level == "wide"})
    elif legacy:
        out.update({S_GROUPS: True, S_ONE: True, S_WIDE: q.level == "wide"})
    else:
        out.update({S_LANES: True, S_RPT: q.rpt, S_GROUPS: q.rpt, S_LEFT: q.level != "lanes", S_WIDE: q.level == "wide"})
    return out


def alt(f, first=2, last=None):
    """f ascending positions whose deltas alternate 2, 3 (never an all-equal block), the first one `first`, the last delta `last`."""
    d = [2 + (i & 1) for i in range(f)]
    d[0] = first
    if last is not None and f > 1:
        d[-1] = last
    return np.cumsum(d).tolist()


def packed(n, salt=0):
    return [1 + (7 * i + salt) % 5 for i in range(n)]


def place(plist, doc):
    """Where `doc`'s positions lie in the term's position stream, from the postings [(doc, [positions])] alone: the stream is every
    doc's position deltas (the first one from 0) in doc order, cut into blocks of 128 values - all-equal ones are stored as one
    value, the others bit-packed - and fewer than 128 values at the end are the trailing VInt block. kernel_skip: values between the
    place the skip entry of the doc's block of 128 docs names and the doc's first one (what the kernels step over)."""
    docs = [d for d, _ in plist]
    at = docs.index(doc)
    freqs = [len(ps) for _, ps in plist]
    deltas = np.concatenate([np.diff(np.asarray(ps, dtype=np.int64), prepend=0) for _, ps in plist])
    ttf = int(deltas.size)
    kinds = ["equal" if np.unique(deltas[b * BLOCK:(b + 1) * BLOCK]).size == 1 else "packed" for b in range(ttf // BLOCK)]
    if ttf % BLOCK:
        kinds.append("trailing")
    start = sum(freqs[:at])
    block, skip = divmod(start, BLOCK)
    last_block = (start + freqs[at] - 1) // BLOCK
    block0 = at // BLOCK * BLOCK
    return dict(freq=freqs[at], ttf=ttf, df=len(plist), block=block, skip=skip, kind=kinds[block], last_block=last_block,
                behind=kinds[block + 1] if block + 1 < len(kinds) else "nothing", between=kinds[block:last_block + 1],
                kernel_skip=sum(freqs[:block0]) % BLOCK + sum(freqs[block0:at]),
                skipped=kinds[(sum(freqs[:block0]) // BLOCK):block])


class Segment:
    """Postings under construction: docs are numbered as they are made, so every term's list is in doc order."""
    PER_DOC = (4, 10, 2, 50)   # positions per filler doc, by term: lists of a few docs (a VInt tail of docs) up to hundreds (packed doc blocks)

    def __init__(self, name):
        self.name, self.postings, self.n_docs, self.cases, self.per_doc = name, [], 0, [], {}

    def terms(self, n):
        self.postings += [[] for _ in range(n)]
        return list(range(len(self.postings) - n, len(self.postings)))

    def doc(self, holdings):
        d = self.n_docs
        self.n_docs += 1
        for t, ps in holdings.items():
            assert list(ps) == sorted(set(ps)) and ps[0] >= 0
            self.postings[t].append((d, [int(p) for p in ps]))
        return d

    def fill(self, term, deltas):
        """Docs that hold `term` alone and carry these position deltas, in order."""
        per = self.per_doc.get(term, self.PER_DOC[term % 4])
        for i in range(0, len(deltas), per):
            self.doc({term: np.cumsum(deltas[i:i + per]).tolist()})

    def lay(self, name, rung, queries, designed, at=None, after=None, ordinary="first", singletons=(), shape=None):
        """One case: the ordinary doc (the first query's terms side by side from position 5 on), per term the fillers that put the
        designed doc's first position at value at[term][1] of position block at[term][0], the designed doc, the fillers behind it
        (after[term]: [(kind, values)], default two packed blocks' worth). ordinary = "after": behind the designed doc."""
        q0 = queries[0]
        offs = list(range(len(q0.terms))) if q0.positions is None else q0.positions
        held = {}
        for t, o in zip(q0.terms, offs):
            if t not in singletons:
                held.setdefault(t, []).append(5 + o - offs[0])
        terms = [t for t in designed if t not in singletons]
        od = self.doc(held) if ordinary == "first" else None
        for i, t in enumerate(terms):
            b, s = (at or {}).get(t, (1, 5 + 3 * i))
            need = BLOCK * b + s - (len(held[t]) if ordinary == "first" else 0)
            assert need >= 0
            self.fill(t, packed(need, salt=t))
        dd = self.doc(designed)
        if ordinary == "after":
            od = self.doc(held)
        for t in terms:
            for kind, n in (after or {}).get(t, [("packed", 200)]):
                self.fill(t, packed(n, salt=t + 1) if kind == "packed" else [1] * n)
        sh = dict(shape or {})
        sh.setdefault("freqs", {t: len(ps) for t, ps in designed.items()})
        case = Case(name, rung, list(queries), dd, od, sh)
        self.cases.append(case)
        return case

    def finish(self, seed):
        rng = np.random.default_rng(seed)
        self.max_doc = self.n_docs
        self.norms = rng.integers(95, 125, size=self.max_doc).astype(np.uint8)
        self.doc_count = self.max_doc                       # every doc holds some term
        self.sum_ttf = sum(len(ps) for pl in self.postings for _, ps in pl)
        assert len({c.name for c in self.cases}) == len(self.cases)
        return self

    def index(self, oracle, version=1):
        return oracle.PositionsIndex(self.max_doc, self.postings, version=version)

    def search(self, ix, q, k, live_docs=None, next_limit=None):
        """The oracle's row for one query: (docs, scores, total hits)."""
        return ix.phrase_search(q.terms, k, self.norms, self.max_doc, self.doc_count, self.sum_ttf, offsets=q.positions, slop=q.slop,
                                live_docs=live_docs, next_limit=next_limit)

    def every_position(self):
        return np.array([p for pl in self.postings for _, ps in pl for p in ps], dtype=np.int32)


def pair(terms, freqs, positions=None, rpt=False, force=None, error=None):
    """The exact and the slop-1 query of one rung. force: "left" = where the positions lie hands the designed doc on whatever its
    freqs, "left-if-sloppy" = the 16-bit lists do (the sloppy 64-candidate kernels only)."""
    out = []
    for slop in (0, 1):
        lv = level(freqs, slop)
        if lv == "lanes" and (force == "left" or (force == "left-if-sloppy" and slop > 0)):
            lv = "left"
        err = error if error is not None else (UNSUPPORTED if lv is None else None)
        out.append(PQ(list(terms), positions, slop, None if err is not None else lv, rpt and slop > 0, err))
    return out


# ---- rungs: positions per term and doc, the sloppy pool, terms per phrase ------------------------------------------------------------
FREQS = (1, 10, 11, 128, 129, 1024, 1025)
POOLS = {"pool-256": (128, 128), "pool-257": (128, 129), "pool-2048": (1024, 1024), "pool-2049": (1024, 1025)}
RPT_POOLS = {"rpt-pool-256": (128, 0), "rpt-pool-257": (128, 1), "rpt-pool-2048": (1024, 0), "rpt-pool-2049": (1024, 1)}


def pairs_of(n):
    """n positions in pairs (p, p + 1) three apart: an exact [x, x] matches every pair; deltas 1, 2, 1, 2 ..."""
    return [3 * (i // 2) + (i & 1) + 2 for i in range(n)]


def build_freq():
    s = Segment("freq")
    for f in FREQS:   # one term f times, the other once, behind the LAST of the f positions: a position too few and the phrase is gone
        a, b = s.terms(2)
        pa = alt(f)
        s.lay("freq-%d" % f, "freq", pair([a, b], [f, 1]), {a: pa, b: [pa[-1] + 1]})
    for name, (fa, fb) in POOLS.items():   # two distinct terms: b one behind every a (and one more)
        a, b = s.terms(2)
        pa = alt(fa)
        pb = [p + 1 for p in pa] + ([pa[-1] + 3] if fb > fa else [])
        s.lay(name, "pool", pair([a, b], [fa, fb]), {a: pa, b: pb}, shape=dict(pool=fa + fb))
    for name, (fx, fy) in RPT_POOLS.items():   # one term named twice: its freq counts twice
        px = pairs_of(fx)
        if fy:
            x, y = s.terms(2)
            s.lay(name, "pool", pair([x, x, y], [fx, fx, fy], rpt=True), {x: px, y: [px[-1] + 1]}, shape=dict(pool=2 * fx + fy))
        else:   # the designed doc is the phrase's FIRST candidate: k_sloppy_groups reads its 1024 positions
            x, = s.terms(1)
            s.per_doc[x] = 4   # (every doc of x is a candidate of [x, x]: no filler in front, small ones behind)
            s.lay(name, "pool", pair([x, x], [fx, fx], rpt=True), {x: px}, at={x: (0, 0)}, ordinary="after", shape=dict(pool=2 * fx, first_candidate=x))
    return s.finish(101)


def build_terms():
    s = Segment("terms")
    for n in (LANE_TERMS, LANE_TERMS + 1, MAX_TERMS):
        ts = s.terms(n)
        s.lay("distinct-%d" % n, "terms", pair(ts, [1] * n), {t: [20 + i] for i, t in enumerate(ts)}, shape=dict(n_terms=n))
    for g in (1, 2, 3):   # [x, x], [x, x, y, y], [x, x, y, y, z, z]: g repetition groups
        ts = s.terms(g)
        phrase = [t for t in ts for _ in range(2)]
        after = None
        if g == 1:   # every doc of x is a candidate of [x, x]: small fillers, and no trailing block (its docs would be handed on)
            s.per_doc[ts[0]] = 4
            after = {ts[0]: [("packed", 3 * BLOCK - (BLOCK + 5 + 2))]}
        s.lay("groups-%d" % g, "terms", pair(phrase, [2] * (2 * g), rpt=True), {t: [20 + 2 * i, 21 + 2 * i] for i, t in enumerate(ts)}, after=after,
              shape=dict(n_terms=2 * g, groups=g))
    ts = s.terms(MAX_TERMS)   # 17 terms: the first one again behind the sixteenth. The oracle answers; the library refuses the call
    held = {t: [20 + i] for i, t in enumerate(ts)}
    held[ts[0]] = [20, 20 + MAX_TERMS]
    s.lay("terms-17", "terms", pair(ts + [ts[0]], [2] + [1] * (MAX_TERMS - 1) + [2], rpt=True, error=ILLEGAL_ARGUMENT), held,
          shape=dict(n_terms=MAX_TERMS + 1))
    return s.finish(102)


# ---- rungs: where the positions lie (designed docs of freq <= 10), 16-bit lists -------------------------------------------------------
BEHIND = {"packed": [("packed", 200)], "equal": [("equal", BLOCK), ("packed", 150)], "trailing": [("packed", 50)], "nothing": []}


def build_place():
    s = Segment("place")

    def one(name, rung, f, at, after, force, last=None, per=None, **shape):
        a, b = s.terms(2)
        if per:
            s.per_doc[a] = per
        pa = alt(f, last=last)
        s.lay(name, rung, pair([a, b], [f, 1], force=force), {a: pa, b: [pa[-1] + 1]}, at={a: at}, after={a: after},
              shape=dict(shape, placed=a, block=at[0], skip=at[1]))
        return a

    f = 7
    for end in (BLOCK - 1, BLOCK, BLOCK + 1):   # skip + freq: inside the block, its last value used, one value in the block behind
        for behind in ("packed", "equal", "trailing", "nothing"):
            if behind == "nothing" and end != BLOCK:
                continue   # nothing behind: the doc's positions end the stream at a block edge
            after = list(BEHIND[behind])
            if end < BLOCK:   # the block is filled up first
                after = [("packed", BLOCK - end)] + after
            if end > BLOCK and behind == "equal":   # the doc's last delta belongs to the all-equal block
                after = [("equal", 2 * BLOCK - end)] + after[1:]
            handed_on = end > BLOCK and behind in ("equal", "trailing")
            one("end-%d-behind-%s" % (end, behind), "straddle", f, (2, end - f), after, "left" if handed_on else None,
                last=1 if behind == "equal" else None, kind="packed", behind=behind, end=end)
    one("first-value-0", "straddle", f, (2, 0), BEHIND["packed"], None, kind="packed", end=f)
    # whole blocks of earlier docs' positions between the skip entry's place and the doc: filler docs of 50 positions each share the
    # doc's block of docs (a tail of docs: the skip entry names the term's first position), of 2 each fill whole blocks of 128 docs
    for name, per, at, force, through in (("skip-packed-docs-tail", 50, (3, 40), None, ["packed"] * 3), ("skip-packed-doc-block", 2, (4, 9), None, None)):
        one(name, "skip", f, at, BEHIND["packed"], force, per=per, kind="packed", kernel_skip_min=BLOCK, through=through)
    a, b = s.terms(2)
    s.per_doc[a] = 64
    pa = alt(f)
    od = s.doc({a: [5], b: [6]})
    s.fill(a, packed(BLOCK - 1, salt=a))                  # block 0 (with the ordinary doc's value)
    s.fill(a, [1] * BLOCK)                                # block 1: all equal
    s.fill(a, packed(20, salt=a))
    dd = s.doc({a: pa, b: [pa[-1] + 1]})
    s.fill(a, packed(200, salt=a + 1))
    s.fill(b, packed(300, salt=b))
    s.cases.append(Case("skip-through-equal", "skip", pair([a, b], [f, 1], force="left"), dd, od,
                        dict(freqs={a: f, b: 1}, placed=a, block=2, skip=20, kind="packed", kernel_skip_min=BLOCK, through=["packed", "equal"])))
    for f1 in (1, LANE_CAP, LANE_CAP + 1):   # a singleton term (df = 1): it lives in the term dictionary entry, its positions in a VInt block
        for where in ("first", "last"):
            x, b = s.terms(2)
            px = alt(f1)
            phrase, held = ([x, b], {x: px, b: [px[-1] + 1]}) if where == "first" else ([b, x], {b: [px[0] - 1], x: px})
            s.lay("singleton-%s-%d" % (where, f1), "singleton", pair(phrase, [f1, 1] if where == "first" else [1, f1], force="left"), held,
                  singletons=(x,), shape=dict(singleton=x))
    # ---- 16-bit lists of the 64-candidate sloppy kernels: position - phrase offset. Exact phrases keep 32-bit lists.
    for name, pos, offs, fits in (("i16-pos-32767", 32767, None, True), ("i16-pos-32768", 32768, None, False),
                                  ("i16-gap-32767", 32767, [0, 5], True), ("i16-gap-32768", 32768, [0, 5], False)):
        a, b = s.terms(2)
        o = offs or [0, 1]
        s.lay(name, "int16", pair([a, b], [1, 1], positions=offs, force=None if fits else "left-if-sloppy"), {a: [pos], b: [pos + o[1]]},
              shape=dict(value=pos, fits=fits))
    # (PhraseWeight wants the first offset at 0, so where a phrase matches every position - offset is >= 0; a negative one is the
    # second term's position 0 under a large offset, in a doc that matches through a later position of that term)
    for name, off, fits in (("i16-offset-minus-32768", 32768, True), ("i16-offset-minus-32769", 32769, False)):
        a, b = s.terms(2)
        s.lay(name, "int16", pair([a, b], [1, 2], positions=[0, off], force=None if fits else "left-if-sloppy"), {a: [10], b: [0, 10 + off]},
              shape=dict(value=-off, fits=fits))
    for name, last, fits in (("i16-last-of-ten-32767", 32767, True), ("i16-last-of-ten-40000", 40000, False)):
        a, b = s.terms(2)   # the first nine positions (and the other term's) are in range, the match is at the ninth
        pa = [32000 + 10 * i for i in range(9)] + [last]
        s.lay(name, "int16", pair([a, b], [10, 1], force=None if fits else "left-if-sloppy"), {a: pa, b: [pa[8] + 1]},
              shape=dict(value=last, fits=fits, in_range=pa[8]))
    return s.finish(103)


BUILDERS = {"freq": build_freq, "terms": build_terms, "place": build_place}
_built = {}


def segment(name):
    if name not in _built:
        _built[name] = BUILDERS[name]()
    return _built[name]


def all_cases():
    return [(name, c) for name in BUILDERS for c in segment(name).cases]


# ---- the collector's chunks ---------------------------------------------------------------------------------------------------------
CHUNK_NS = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
KS = (1, 10, 64, 65, 128, 129, 300)
EVERY = 37   # behind the first match, every 37th candidate matches too


class Chunks:
    """n docs, all of them candidates of every pair of terms (p, q): doc = candidate index. Pair j's first phrase match is candidate
    FIRST[j]; behind it every 37th candidate matches; everywhere else p and q are ~50 positions apart (a conjunction match, no
    phrase match at slop 1). A matching doc reads "p q p"."""

    def __init__(self, n):
        self.n = self.max_doc = n
        self.first = [i for i in (0, CHUNK - 1, CHUNK, CHUNK + 1, n - 1) if i < n]
        self.first = sorted(set(self.first))
        self.postings = []
        self.matches = []
        for i in self.first:
            m = np.zeros(n, dtype=bool)
            m[i] = True
            m[np.arange(n) % EVERY == 0] = True
            m[:i] = False
            self.matches.append(m)
            self.postings.append([(d, [3, 5] if m[d] else [d % 7]) for d in range(n)])
            self.postings.append([(d, [4] if m[d] else [50 + d % 5]) for d in range(n)])
        rng = np.random.default_rng(200 + n)
        self.norms = rng.integers(95, 125, size=n).astype(np.uint8)
        self.doc_count = n
        self.sum_ttf = sum(len(ps) for pl in self.postings for _, ps in pl)

    def queries(self, j):
        """Pair j: the exact phrase, the plain sloppy one, the sloppy one that names p twice."""
        p, q = 2 * j, 2 * j + 1
        return [PQ([p, q], None, 0, None, False, None), PQ([p, q], None, 1, None, False, None), PQ([p, q, p], None, 1, None, True, None)]

    def limits(self, j):
        i = self.first[j]
        return sorted({x for x in (i - 1, i, i + 1, 0, self.n - 1, self.n) if x >= 0}) + [None]

    index = Segment.index
    search = Segment.search

    def live_words(self, alive):
        return np.packbits(np.concatenate([alive, np.zeros(-self.n % 64, dtype=bool)]), bitorder="little").view(np.uint64).copy()


_chunks = {}


def chunks(n):
    if n not in _chunks:
        _chunks[n] = Chunks(n)
    return _chunks[n]


# ---- a PositionsIndex as a LeafReader ------------------------------------------------------------------------------------------------
def leaf_of(ix, n_terms, norms, max_doc, doc_count, sum_ttf, live_docs=None):
    """The oracle writer's files as a rucene_amd.LeafReader with its positions attached."""
    import rucene_amd
    from rucene_amd import _lib as gpu
    doc_bytes, pos_bytes = ix.files()
    terms = np.zeros(n_terms, dtype=gpu.TERM_STATE_DTYPE)
    tpos = np.zeros(n_terms, dtype=gpu.TERM_POSITIONS_DTYPE)
    for t in range(n_terms):
        st = ix.term_state(t)
        terms[t] = (st["doc_start_fp"], st["skip_offset"], st["total_term_freq"], st["doc_freq"], st["singleton_doc_id"])
        tpos[t]["pos_start_fp"], tpos[t]["last_pos_block_offset"] = st["pos_start_fp"], st["last_pos_block_offset"]
    leaf = rucene_amd.LeafReader(np.frombuffer(doc_bytes, np.uint8), norms, max_doc, terms, live_docs=live_docs, doc_count=doc_count,
                                 sum_total_term_freq=sum_ttf, index_options=3)
    leaf.pos_bytes, leaf.term_positions = np.frombuffer(pos_bytes, np.uint8), tpos
    return leaf
