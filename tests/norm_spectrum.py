"""Norm-spectrum fixtures (plain Python, no GPU): segments whose norm bytes cover the range a real index can hold, built so that the
two ways the library stores norms are both entered the way an index enters them. A segment with at most 64 distinct norm bytes is
kept in RANK mode (HBM holds each byte's rank, the LDS score table, block-max frontier words of 6 rank bits per freq, chunk
frontiers, sketches, the pruned TERM kernels, k_or_wide / k_or_lazy); one with 65 or more is kept in RAW mode, where none of that
runs. Spectra:

  one       1 byte (200: above 127)                                   rank
  extremes  {0, 255}                                                  rank
  rank64    exactly 64 bytes: 0, 1, 70..125, 132 .. 164, 255          rank, ranks 0..63 all used
  raw65     the same and byte 128                                     raw, entered without the config switch
  all256    every byte                                                raw

Every spectrum has one max_doc and these lists (term ids: the names below):

  PLANTED   320 full blocks (five 64-block chunks) + a VInt tail; background postings of freq 1 and the spectrum's lowest byte;
            one winner in block 0, on both sides of two chunk edges, in the last full block and in the tail, whose norm byte has a
            high rank (63, 62, 33, 32 in rank64; bytes >= 128 in the raw spectra); one loser just above the background.
  CROSSED   200 full blocks + a tail on other docs: one block holds three winners of different (freq, rank) slots, one block's
            best posting has freq 11 (frontier word 15: never pruned).
  ZERO_FRONT / ZERO_DEEP  lists of lowest-byte docs (byte 0: table[0] = 1 / table[255], a length near 3.7e18, scores near 1e-17)
            with a few ordinary bytes spread over the list / only in its last blocks.
  RANDOM    lists over docs of random bytes of the whole spectrum: a singleton, an absent term, df 127 / 128 / 129, either side of
            the bitmap density (1 doc in 64), 20 000, 100 000 and every doc; freqs 1..10, a few above 10 and above 255.

A second, small segment over the same norms carries positions (two- and three-term phrases).

The builder asserts its own rules, so a bad fixture fails on the CPU: every plant is separated from its neighbours and from the
background by a relative gap of 1e-4 in float64 (far above the f32 rounding of one multiply and one divide; scores saturate at the
top of the byte range - bytes 164 and 255 are 7e-7 apart - so saturated winners differ by freq, never by byte alone); every
rank-mode winner of rank r >= 32 is a winner ONLY because of its norm: the same freq scored with the byte of rank r & 31 falls
below the lowest winner, so a frontier word that loses the top rank bit prunes the block at k = number of winners; rank64 and
raw65 hold exactly 64 and 65 distinct bytes in the norms array."""
import numpy as np

K1, B = 1.2, 0.75
GAP = 1e-4


def _byte315_to_float(b):
    b = np.asarray(b, dtype=np.uint32)
    bits = ((b & 0xFF) << 21) + ((63 - 15) << 24)
    return np.where(b == 0, 0.0, bits.astype(np.uint32).view(np.float32).astype(np.float64))


def bm25_f64(df, doc_count, avgdl, freq, norm_byte):
    """Plain BM25 in float64 (bm25_similarity.rs: idf, the 1 / f^2 length table, k1 (1 - b + b dl / avgdl)); norm_byte None: no norms."""
    idf = np.log(1.0 + (doc_count - df + 0.5) / (df + 0.5))
    freq = np.asarray(freq, dtype=np.float64)
    if norm_byte is None:
        norm = K1
    else:
        nb = np.asarray(norm_byte)
        f = _byte315_to_float(np.where(nb == 0, 255, nb))
        length = np.where(nb == 0, f * f, 1.0 / (f * f))  # table[0] = 1 / table[255]
        norm = K1 * ((1.0 - B) + B * length / avgdl)
    return idf * (K1 + 1.0) * freq / (freq + norm)


def scores_f32(doc_freq, max_doc, doc_count, sttf, freqs, norm_bytes):
    """f32 BM25 of one term's postings, left to right as bm25_similarity.rs:203-212 writes it (tests/fullsize_checks.py): numpy's
    elementwise f32 arithmetic is IEEE correctly rounded, so these are the reference's bits without the oracle."""
    import rucene_amd
    w, _idf, cache = rucene_amd.bm25_compute_weight(K1, B, max_doc, doc_count, sttf, [int(doc_freq)])
    wk = np.float32(np.float32(w) * np.float32(np.float32(K1) + np.float32(1.0)))
    f = np.asarray(freqs).astype(np.float32)
    return (wk * f) / (f + cache.astype(np.float32)[np.asarray(norm_bytes)])


MAX_DOC = 300_000
STTF = 3 * MAX_DOC
SPECTRA = ("one", "extremes", "rank64", "raw65", "all256")
RANK_SPECTRA = ("one", "extremes", "rank64")
RAW_SPECTRA = ("raw65", "all256")
_RANK64 = [0, 1] + list(range(70, 126)) + [132, 140, 148, 156, 164, 255]
BYTES = {"one": [200], "extremes": [0, 255], "rank64": _RANK64, "raw65": sorted(_RANK64 + [128]), "all256": list(range(256))}
# the bytes the plants take, by role: HI1 / HI2 saturated top bytes, MID1 / MID2 / MID3 bytes whose scores still separate
_rank_roles = dict(HI1=255, HI2=164, MID1=101, MID2=100, MID3=110, ORD=[120, 110, 124, 132])   # ranks 63, 62, 33, 32, 42
_raw_roles = dict(HI1=255, HI2=164, MID1=128, MID2=132, MID3=140, ORD=[120, 110, 124, 132])
ROLES = {"one": dict(HI1=200, HI2=200, MID1=200, MID2=200, MID3=200, ORD=[200]),
         "extremes": dict(HI1=255, HI2=255, MID1=255, MID2=255, MID3=255, ORD=[255]),
         "rank64": _rank_roles, "raw65": _raw_roles, "all256": _raw_roles}

PLANTED, CROSSED, ZERO_FRONT, ZERO_DEEP = 0, 1, 2, 3
RANDOM0 = 4
RANDOM_DFS = [1, 0, 127, 128, 129, 3000, 4600, 4800, 20_000, 100_000, MAX_DOC]
SINGLETON, ABSENT, EVERY_DOC = RANDOM0, RANDOM0 + 1, RANDOM0 + len(RANDOM_DFS) - 1
SPARSE, BELOW_DENSITY, ABOVE_DENSITY, BITMAP, HALF = RANDOM0 + 5, RANDOM0 + 6, RANDOM0 + 7, RANDOM0 + 8, RANDOM0 + 9
N_TERMS = RANDOM0 + len(RANDOM_DFS)
assert MAX_DOC // 64 > RANDOM_DFS[6] and (MAX_DOC + 63) // 64 < RANDOM_DFS[7]  # either side of the bitmap density

TAIL = 77
PLANTED_BLOCKS, CROSSED_BLOCKS, ZERO_BLOCKS = 320, 200, 150
# (block, posting inside the block, freq, role); block "tail": the VInt tail. Freqs distinct within a list: saturated bytes tie.
PLANTED_WINNERS = [(0, 77, 3, "HI1"), (63, 5, 10, "MID1"), (64, 120, 6, "HI2"), (127, 127, 9, "MID2"), (128, 0, 5, "HI1"),
                   (PLANTED_BLOCKS - 1, 64, 4, "HI2"), ("tail", 40, 8, "MID1")]
PLANTED_LOSER = (200, 33, 2, "BG")   # mid-chunk (chunk 3, lane 8)
CROSSED_WINNERS = [(0, 1, 7, "MID2"), (70, 3, 3, "HI1"), (70, 64, 6, "MID3"), (70, 126, 10, "MID1"), (63, 90, 4, "HI2"),
                   (64, 17, 8, "MID1"), (CROSSED_BLOCKS - 1, 100, 11, "HI2"), ("tail", 76, 5, "HI1")]
CROSSED_LOSER = (130, 60, 2, "BG")


class _Stats:
    """What tests/fullsize_checks.py's scorers read from a segment."""

    def __init__(self, seg, norms):
        self.max_doc = self.doc_count = MAX_DOC
        self.sum_total_term_freq, self.terms, self.norms = STTF, seg.terms, norms


class Spectrum:
    def __init__(self, name, version=1):
        from rucene_amd import indexgen
        assert name in SPECTRA
        self.name, self.version = name, version
        self.rank_mode = name in RANK_SPECTRA
        self.bytes = np.array(BYTES[name], dtype=np.uint8)
        self.roles = dict(ROLES[name], BG=int(self.bytes.min()))
        self.max_doc, self.sttf = MAX_DOC, STTF
        self.avgdl = float(np.float32(STTF / MAX_DOC))
        rng = np.random.default_rng(315)
        # disjoint doc sets for the four built lists, everything else carries random bytes of the spectrum
        sizes = [128 * PLANTED_BLOCKS + TAIL, 128 * CROSSED_BLOCKS + TAIL, 128 * ZERO_BLOCKS + TAIL, 128 * ZERO_BLOCKS + TAIL]
        perm = rng.permutation(MAX_DOC)
        cuts = np.cumsum([0] + sizes)
        owned = [np.sort(perm[cuts[i]:cuts[i + 1]]).astype(np.int32) for i in range(4)]
        norms = self.bytes[rng.integers(0, self.bytes.size, size=MAX_DOC)]
        norms[perm[cuts[4]:cuts[4] + self.bytes.size]] = self.bytes  # every byte present whatever the draw, on docs no built list owns
        lists = []
        self.plants = {}
        for term, (blocks, winners, loser) in enumerate([(PLANTED_BLOCKS, PLANTED_WINNERS, PLANTED_LOSER),
                                                         (CROSSED_BLOCKS, CROSSED_WINNERS, CROSSED_LOSER)]):
            docs = owned[term]
            freqs = np.ones(docs.size, np.int32)
            norms[docs] = self.roles["BG"]
            pos = np.array([128 * (blocks if b == "tail" else b) + i for b, i, _, _ in winners + [loser]])
            freqs[pos] = [p[2] for p in winners + [loser]]
            norms[docs[pos]] = [self.roles[p[3]] for p in winners + [loser]]
            lists.append((docs, freqs))
            self.plants[term] = (pos, docs[pos], len(winners))
        ordinary = self.roles["ORD"]
        for term, where in ((ZERO_FRONT, np.array([3, 128 * 20 + 9, 128 * 63 + 127, 128 * 64, 128 * 100 + 50, 128 * ZERO_BLOCKS + 5])),
                            (ZERO_DEEP, 128 * (ZERO_BLOCKS - 2) + np.array([0, 77, 127, 128, 200, 260]))):
            docs = owned[term]
            norms[docs] = self.roles["BG"]
            norms[docs[where]] = [ordinary[i % len(ordinary)] for i in range(where.size)]
            freqs = rng.integers(1, 4, size=docs.size).astype(np.int32)
            freqs[where] = 1 + np.arange(where.size)
            lists.append((docs, freqs))
        for df in RANDOM_DFS:
            docs = np.arange(MAX_DOC, dtype=np.int32) if df == MAX_DOC else np.sort(rng.choice(MAX_DOC, size=df, replace=False)).astype(np.int32)
            freqs = rng.integers(1, 11, size=df).astype(np.int32)
            if df >= 127:
                odd = rng.choice(df, size=max(3, df // 300), replace=False)
                freqs[odd] = rng.choice([11, 12, 57, 255, 256, 1000, 70_000], size=odd.size)
            lists.append((docs, freqs))
        self.norms, self.lists = norms, lists
        n_distinct = np.unique(norms).size
        assert n_distinct == self.bytes.size == {"one": 1, "extremes": 2, "rank64": 64, "raw65": 65, "all256": 256}[name], n_distinct
        assert (n_distinct <= 64) == self.rank_mode
        self.rank_of = {int(b): r for r, b in enumerate(np.unique(norms))}
        if name == "rank64":
            assert sorted(self.rank_of[self.roles[r]] for r in ("HI1", "HI2", "MID1", "MID2")) == [32, 33, 62, 63]
            assert {0, 1, 255} <= set(self.rank_of) and sum(b > 130 for b in self.rank_of) >= 5
        self.seg = indexgen.build_explicit(MAX_DOC, lists, norms=norms, version=version)
        self.stats = _Stats(self.seg, norms)
        for term in (PLANTED, CROSSED):
            self._check_plants(term)

    # ---- the planted lists ----------------------------------------------------------------------------------------------------
    def n_winners(self, term):
        return self.plants[term][2]

    def plant_scores(self, term, extra=None):
        pos, docs, _ = self.plants[term]
        s = bm25_f64(self.lists[term][0].size, MAX_DOC, self.avgdl, self.lists[term][1][pos], self.norms[docs])
        return s if extra is None else s + extra(docs)

    def _check_plants(self, term, extra=None):
        """The fixture rules: gaps of 1e-4 between plants and to the background; winners of rank >= 32 win by their norm alone."""
        pos, docs, nw = self.plants[term]
        df = self.lists[term][0].size
        s = self.plant_scores(term, extra)
        w = np.sort(s[:nw])
        assert (np.diff(w) > GAP * w[1:]).all(), (self.name, term, "winners too close", w)
        assert s[nw] < w[0] * (1 - GAP), (self.name, term, "loser not below the winners")
        bg = bm25_f64(df, MAX_DOC, self.avgdl, 1, self.roles["BG"])
        if extra is not None:  # the best a background doc of this list can total
            bgdocs = np.setdiff1d(self.lists[term][0], docs)
            bg = bg + extra(bgdocs).max()
        assert s[nw] > bg * (1 + GAP), (self.name, term, "loser not above the background")
        if self.rank_mode and extra is None:
            by_rank = np.unique(self.norms)
            freqs = self.lists[term][1][pos[:nw]]
            for i in range(nw):
                r = self.rank_of[int(self.norms[docs[i]])]
                if r >= 32 and freqs[i] <= 10:
                    under = scores_f32(df, MAX_DOC, MAX_DOC, STTF, [freqs[i]], [by_rank[r & 31]])[0]
                    lowest = scores_f32(df, MAX_DOC, MAX_DOC, STTF, freqs, self.norms[docs[:nw]]).min()
                    assert under < lowest and bm25_f64(df, MAX_DOC, self.avgdl, freqs[i], by_rank[r & 31]) < w[0] * (1 - GAP), \
                        (self.name, term, i, "a winner that would also win with the byte of rank r & 31")

    def ranking(self, term, extra=None, live=None):
        """Planted docs of `term` by float64 BM25 (winners, then the loser); `extra(docs) -> float64`: other clauses' scores (the gap
        rules are asserted again on the sums); `live`: boolean mask over the plants."""
        if extra is not None:
            self._check_plants(term, extra)
        s, docs = self.plant_scores(term, extra), self.plants[term][1]
        if live is not None:
            s, docs = s[live], docs[live]
        return docs[np.lexsort((docs, -s))]

    def term_score_f64(self, term, docs):
        """float64 BM25 that `term` gives to `docs` (all of which it must hold)."""
        d, f = self.lists[term]
        at = np.searchsorted(d, docs)
        assert (d[at] == docs).all()
        return bm25_f64(d.size, MAX_DOC, self.avgdl, f[at], self.norms[docs])

    def term_rows_f32(self, term, k):
        """The top k of one term from the f32 numpy scoring: (docs, scores), score descending, ties to the lower doc."""
        d, f = self.lists[term]
        s = scores_f32(d.size, MAX_DOC, MAX_DOC, STTF, f, self.norms[d])
        order = np.lexsort((d, -s.astype(np.float64)))[:k]
        return d[order], s[order]

    def oracle_segment(self, oracle, live_docs=None):
        return oracle.Segment(self.seg.doc_bytes, self.seg.norms, MAX_DOC, self.seg.terms, live_docs=live_docs, sum_total_term_freq=STTF)

    # ---- positions ------------------------------------------------------------------------------------------------------------
    def positions(self):
        """A positions field over the same norms: 24 000 docs (a stride through the segment, so every kind of doc set above is met)
        of 1..14 tokens from a vocabulary of five, plus a term in every 7th of them at position 2 and a singleton.
        Returns (segment, phrases as (terms, slop), doc_count, sum_total_term_freq)."""
        from rucene_amd import indexgen
        rng = np.random.default_rng(77)
        vocab = 5
        holders = np.arange(5, MAX_DOC, MAX_DOC // 24_000)[:24_000]
        postings = [[] for _ in range(vocab + 2)]
        sum_ttf = 0
        for n, d in enumerate(holders.tolist()):
            toks = rng.integers(0, vocab, size=int(rng.integers(1, 15))).tolist()
            if n % 7 == 0:
                toks[2:3] = [vocab]
            sum_ttf += len(toks)
            where = {}
            for p, t in enumerate(toks):
                where.setdefault(t, []).append(p)
            for t, ps in where.items():
                postings[t].append((d, ps))
        postings[vocab + 1] = [(int(holders[100]), [1, 3])]
        sum_ttf += 2
        seg = indexgen.build_explicit_positions(MAX_DOC, postings, norms=self.norms, version=self.version)
        phrases = [([0, 1], 0), ([1, 0], 0), ([2, 3, 4], 0), ([0, 0], 0), ([4, vocab], 0), ([vocab, 1, 2], 0), ([vocab + 1, 0], 0),
                   ([0, 1], 2), ([3, 2], 2), ([0, 1, 2], 2), ([4, 4], 2), ([vocab, 3], 2), ([1, vocab, 0], 2)]
        return seg, phrases, holders.size, sum_ttf


_built = {}


def spectrum(name, version=1):
    """One Spectrum per (name, .doc version) and process."""
    if (name, version) not in _built:
        _built[(name, version)] = Spectrum(name, version)
    return _built[(name, version)]
