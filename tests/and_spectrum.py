"""Fixtures for the conjunction kernel k_search_and (plain Python, no GPU): one list or query on each side of every threshold
rucene_amd/csrc/kernels/search_and.hpp and the host rules of rucene_amd/csrc/rgpu_api.hip (bitmap_min_df_and, ensure_bitmaps_locked,
ensure_memb_only_locked) branch on, an independent reference (AndRef) and Python models of the kernel's survivor queue, of its
register window over a walked clause's block directory, of find_block_wave and of the launch's block-decode counter.

The main leaf has max_doc 300 007 (no multiple of 32: the last bitmap word holds 7 docs), which gives four doc_freq ranges:
walked below MEMB_MIN_DF = 512, membership bits alone below BITMAP_MIN_DF = max(1024, ceil(max_doc / 256)) = 1172, a full bitmap
without the four-bits-per-doc array below NIB_MIN_DF = ceil(max_doc / 128) = 2344, with it from there on. Every list is derived from
these constants:

  CORE (not a term)     200 docs every clause list below holds: doc 0, doc max_doc - 1 and 198 docs at bit 0, bit 31, bit 8 (nibble 0
                        of a four-bit word) and bit 15 (nibble 7) of a bitmap word, in turn; NEIGH: the doc after every second bit-0
                        CORE doc, which no clause list holds (absent from the word that holds its neighbour)
  CORE_LEAD, EDGE_LEAD  CORE[:139] and max_doc - 1 (one block and a 12-doc tail); CORE and NEIGH (one block and a tail)
  LEAD_127, LEAD_128    the first 127 | 128 CORE docs: a VInt tail alone (never the batched probe) | one FullBlock and nothing
  TAIL_2, SING_*        docs 0 and max_doc - 1; singletons (they live in the term-dictionary entry) on an even and an odd posting of
                        CORE_LEAD and on doc 7, which only EVERY and REG4 hold besides
  C_511 .. C_2344       CORE and seeded docs up to the doc_freq they are named for: either side of 512, of 1172 and of 2344. C_2344
                        carries freq 14 | 15 on CORE[30] | CORE[31] (one lane's two slots of CORE_LEAD's block)
  EQ_A, EQ_B, EQ_C      three lists of doc_freq 300 over CORE: the stable clause order decides the f32 sum
  OVF_SMALL, OVF_CAP,   freq 255 on CORE[20], 256 on CORE[21] (one lane's two slots), 254 on CORE[40], 300 on CORE[60], 255 on
  OVF_OVER              CORE[100] - the first and the last posting of the overflow list hold 255. OVF_CAP has 4096 postings of freq >=
                        255 (BITMAP_OVF_CAP), OVF_OVER 4097: no bitmap, walked whatever its doc_freq, doc_bitmap_refused + 1
  SPREAD, SPREAD_NOTAIL docs 1000 i + 3 (blocks that span 127 000 docs: far more than the 2048 bits of the LDS filter) and max_doc - 1:
                        two blocks and a 45-doc tail; its first 256 docs alone
  FP_LEAD               pairs (e, e + 2048) with e in SPREAD, neighbours in the lead: a real hit and a filter false positive in
                        neighbouring lanes and, behind a single doc in the middle, in one lane's two slots; a block's last doc and
                        last doc + 1; a doc below the first block; candidates behind the last FullBlock that the tail holds, does
                        not hold, and a false positive there
  SAME_LEAD             two lead blocks inside SPREAD's first block: the cursor does not move
  REG4, WIN_LEAD        docs 4 i + 3 (doc_freq 75 001: block b spans docs 512 b ..) and candidates in its blocks 0, 62, 63, 125, 127,
                        190: the next pending candidate's block 62 | 63 | 64 slots past the register window's start
  EVERY, CONST          every doc (freq 2 on CONST's docs); docs 50 000 .. 51 099 with freq 3 and one norm byte: 1100 tied hits across
                        every item edge
  Q_LEAD, Q_C1          eight blocks and a tail; every doc of it but one of the first four blocks: the queue holds 127 + 512 = 639 of
                        640 cells
  S_LEAD, S_C1          twenty blocks and nothing; 0, 128, 129, 126 and 1 survivors in its five groups of four blocks
  G_1 .. G_9, G_C1      1, 2, 3, 4, 5, 7, 8 and 9 lead blocks (a 3-doc tail behind the odd ones); every other doc of them
  T_A, T_B, T_C, T_C1   twelve blocks and a tail with a freq of 2^20 - 1 | 2^20 in the first group | 2^20 in the third group; two docs
                        in five of each
  W_60 .. W_130         60, 61, 64, 65 and 130 lead blocks: the lead's own directory window reloads
  HALF_B, HALF_N        every second CORE doc from the first | from the second on, with seeded docs: a bitmap | a bitmap with the four-bit
                        array that holds half of the candidates (as MUST_NOT clauses they leave the other half alive)

The big leaf (550 475 docs) holds one list of every doc - 4300 FullBlocks and a 75-doc tail - and short leads whose second block lies
0 .. 64 + 4097 blocks behind find_block_wave's `from`: its first look, none, one and two rounds of the 64-ary loop, a loop entered
at hi - lo = 64 | 65 and "no slot qualifies". It is searched with every clause walked (and_bitmaps = -1).

Freqs are geometric, capped at 10, unless stated. Norms "rank" / "raw" / "none"; live docs "none" / "seeded" (85 % alive; deleted
for certain: CORE[4] - bit 0 -, CORE[5] - bit 31 -, and SPREAD's doc 4003, a real filter hit of FP_LEAD); `.doc` version 1 | 0.
tests/test_and_spectrum_cpu.py proves every property named here, and the oracle against AndRef, before a GPU sees any of it."""
import numpy as np

import segment_spectrum as ss
from segment_spectrum import Query

MAX_DOC = 300_007
BIG_MAX_DOC = 4300 * 128 + 75
BLOCK = 128
MEMB_MIN_DF = 512              # MEMB_ONLY_MIN_DF
MEMB_MIN_LEAD = 128            # ... and the lead needs a FullBlock
NIBBLE_DENSITY = 128           # BITMAP_NIBBLE_DENSITY
BITMAP_OVF_CAP = 4096
OVF_FREQ = 255
AND_G = 4
AND_Q_CAP = 128 + 128 * AND_G
AND_Q_FREQ_LIMIT = 1 << 20
FILTER_BITS = 2048
XCD_ROUND_ITEMS = 8 * 64 * 4   # chunks x workgroups x wavefronts
AUTO_ITEM_BLOCKS = 8           # and_item_blocks for a small launch
KS = (1, 10, 64, 65, 128, 129, 300)
NORMS = ("rank", "raw", "none")
LIVE = ("none", "seeded")
VERSIONS = (1, 0)
STTF_PER_DOC = 60
RAW_BYTES = np.arange(60, 130, dtype=np.uint8)
TIE_BYTE = 110
CONST_LO, CONST_HI, CONST_FREQ, EVERY_FREQ_ON_CONST = 50_000, 51_100, 3, 2


def bitmap_min_df(max_doc, and_bitmaps=0):
    """bitmap_min_df_and: the smallest doc_freq that gets a full bitmap (None: no bitmaps)."""
    if and_bitmaps < 0:
        return None
    den = 256 if and_bitmaps == 0 else and_bitmaps
    return max(1024, -(-max_doc // den))


def nib_min_df(max_doc):
    return -(-max_doc // NIBBLE_DENSITY)


BITMAP_MIN_DF = bitmap_min_df(MAX_DOC)
NIB_MIN_DF = nib_min_df(MAX_DOC)

NAMES = ["CORE_LEAD", "EDGE_LEAD", "LEAD_127", "LEAD_128", "TAIL_2", "SING_EVEN", "SING_ODD", "SING_MISS", "ABSENT", "C_511", "C_512", "C_1171", "C_1172",
         "C_2343", "C_2344", "EQ_A", "EQ_B", "EQ_C", "OVF_SMALL", "OVF_CAP", "OVF_OVER", "SPREAD", "SPREAD_NOTAIL", "FP_LEAD", "SAME_LEAD", "REG4",
         "WIN_LEAD", "EVERY", "CONST", "Q_LEAD", "Q_C1", "S_LEAD", "S_C1", "G_1", "G_2", "G_3", "G_4", "G_5", "G_7", "G_8", "G_9", "G_C1", "T_A", "T_B",
         "T_C", "T_C1", "W_60", "W_61", "W_64", "W_65", "W_130", "HALF_B", "HALF_N"]
(CORE_LEAD, EDGE_LEAD, LEAD_127, LEAD_128, TAIL_2, SING_EVEN, SING_ODD, SING_MISS, ABSENT, C_511, C_512, C_1171, C_1172, C_2343, C_2344, EQ_A, EQ_B, EQ_C,
 OVF_SMALL, OVF_CAP, OVF_OVER, SPREAD, SPREAD_NOTAIL, FP_LEAD, SAME_LEAD, REG4, WIN_LEAD, EVERY, CONST, Q_LEAD, Q_C1, S_LEAD, S_C1, G_1, G_2, G_3, G_4,
 G_5, G_7, G_8, G_9, G_C1, T_A, T_B, T_C, T_C1, W_60, W_61, W_64, W_65, W_130, HALF_B, HALF_N) = range(len(NAMES))
N_TERMS = len(NAMES)
KINDS = {C_511: 511, C_512: 512, C_1171: BITMAP_MIN_DF - 1, C_1172: BITMAP_MIN_DF, C_2343: NIB_MIN_DF - 1, C_2344: NIB_MIN_DF}
G_LEADS = {G_1: 1, G_2: 2, G_3: 3, G_4: 4, G_5: 5, G_7: 7, G_8: 8, G_9: 9}
W_LEADS = {W_60: 60, W_61: 61, W_64: 64, W_65: 65, W_130: 130}
T_LEADS = {T_A: (5, AND_Q_FREQ_LIMIT - 1), T_B: (5, AND_Q_FREQ_LIMIT), T_C: (2 * AND_G * BLOCK + 6, AND_Q_FREQ_LIMIT)}   # posting index, freq
S_SURVIVORS = (0, 128, 129, 126, 1)
Q_MISSING_AT = 100
# freqs planted on the posting of CORE[i]
OVF_PLANTS = {20: 255, 21: 256, 40: 254, 60: 300, 100: 255}
NIB_PLANTS = {30: 14, 31: 15}
SPREAD_STEP, SPREAD_OFF, SPREAD_N = 1000, 3, 300
FP_PAIRS_STEP = 4
WIN_BLOCKS = (0, 62, 63, 125, 127, 190)
REG4_STEP, REG4_OFF = 4, 3

_EMPTY = (np.zeros(0, np.int32), np.zeros(0, np.int32))


def core_docs(max_doc=MAX_DOC):
    at = (0, 31, 8, 15)
    mid = [1500 * i // 32 * 32 + at[i % 4] for i in range(1, 199)]
    return np.array([0] + mid + [max_doc - 1], np.int32)


def neigh_docs(max_doc=MAX_DOC):
    c = core_docs(max_doc)
    return np.array([int(d) + 1 for i, d in enumerate(c) if i % 8 == 0 and 0 < i < 199], np.int32)


def spread_docs(max_doc=MAX_DOC):
    return np.array([SPREAD_STEP * i + SPREAD_OFF for i in range(SPREAD_N)] + [max_doc - 1], np.int32)


def fp_lead_docs(max_doc=MAX_DOC):
    """Doc 1 (below SPREAD's first block); pairs (e, e + 2048) for every fourth e of SPREAD, a single doc in the middle that swaps the
    slots of the pairs behind it; SPREAD's first block's last doc and the doc after it; a doc in the tail's range
    that the tail does not hold."""
    sp = spread_docs(max_doc)
    docs = {1, int(sp[BLOCK - 1]), int(sp[BLOCK - 1]) + 1, int(sp[290]) + 500, int(sp[150]) - 10}
    for i in range(0, SPREAD_N, FP_PAIRS_STEP):
        docs.update((int(sp[i]), int(sp[i]) + FILTER_BITS))
    return np.array(sorted(docs), np.int32)


def _freqs(rng, n, cap=10):
    return np.minimum(cap, rng.geometric(0.5, size=n)).astype(np.int32)


def build_lists(max_doc=MAX_DOC):
    rng = np.random.default_rng([max_doc, 11])
    every = np.arange(max_doc, dtype=np.int32)
    core, neigh, sp = core_docs(max_doc), neigh_docs(max_doc), spread_docs(max_doc)
    taken = np.zeros(max_doc, bool)
    taken[core] = taken[neigh] = True
    taken[[1, 7]] = True
    pool = np.flatnonzero(~taken).astype(np.int32)
    lists = [None] * N_TERMS

    def plain(docs):
        docs = np.asarray(docs, np.int32)
        return docs, _freqs(rng, docs.size)

    def drawn(n):
        return np.sort(rng.choice(pool, size=n, replace=False)).astype(np.int32)

    def over_core(df, plants=None):
        d = np.union1d(core, drawn(df - core.size)).astype(np.int32)
        f = _freqs(rng, d.size)
        for i, v in (plants or {}).items():
            f[np.searchsorted(d, core[i])] = v
        return d, f

    lead = np.concatenate([core[:139], core[-1:]])
    lists[CORE_LEAD] = plain(lead)
    lists[EDGE_LEAD] = plain(np.union1d(core, neigh))
    lists[LEAD_127], lists[LEAD_128] = plain(core[:127]), plain(core[:128])
    lists[TAIL_2] = plain([0, max_doc - 1])
    lists[SING_EVEN], lists[SING_ODD], lists[SING_MISS] = plain(lead[10:11]), plain(lead[11:12]), plain([7])
    lists[ABSENT] = _EMPTY
    for t, df in KINDS.items():
        lists[t] = over_core(df, NIB_PLANTS if t == C_2344 else None)
    for t in (EQ_A, EQ_B, EQ_C):
        lists[t] = over_core(300)
    lists[OVF_SMALL] = over_core(1300, OVF_PLANTS)
    for t, n_ovf in ((OVF_CAP, BITMAP_OVF_CAP), (OVF_OVER, BITMAP_OVF_CAP + 1)):
        d, f = over_core(4200, OVF_PLANTS)
        planted = np.isin(d, core[list(OVF_PLANTS)])
        rest = np.flatnonzero(~planted)
        have = int((f >= OVF_FREQ).sum())
        f[rest[:n_ovf - have]] = OVF_FREQ
        lists[t] = (d, f)
    lists[SPREAD] = plain(sp)
    lists[SPREAD_NOTAIL] = plain(sp[:2 * BLOCK])
    lists[FP_LEAD] = plain(fp_lead_docs(max_doc))
    inside = sp[:100]
    filler = np.setdiff1d(pool[(pool > sp[0]) & (pool < sp[BLOCK - 1])], sp)
    lists[SAME_LEAD] = plain(np.union1d(inside, rng.choice(filler, size=2 * BLOCK - inside.size, replace=False)))
    lists[REG4] = plain(every[REG4_OFF::REG4_STEP])
    lists[WIN_LEAD] = plain(sorted(512 * b + o for b in WIN_BLOCKS for o in (3, 4)))
    f = _freqs(rng, max_doc)
    f[CONST_LO:CONST_HI] = EVERY_FREQ_ON_CONST
    lists[EVERY] = (every, f)
    lists[CONST] = (every[CONST_LO:CONST_HI].copy(), np.full(CONST_HI - CONST_LO, CONST_FREQ, np.int32))
    q = drawn(8 * BLOCK + 5)
    lists[Q_LEAD] = plain(q)
    lists[Q_C1] = plain(np.union1d(np.delete(q, Q_MISSING_AT), drawn(400)))
    s = drawn(20 * BLOCK)
    keep = np.concatenate([s[g * AND_G * BLOCK:(g + 1) * AND_G * BLOCK][::3][:n] for g, n in enumerate(S_SURVIVORS)])
    other = np.setdiff1d(drawn(3000), s)
    lists[S_LEAD] = plain(s)
    lists[S_C1] = plain(np.union1d(keep, other[:2600 - keep.size]))
    g = drawn(9 * BLOCK + 3)
    for t, n in G_LEADS.items():
        lists[t] = plain(g[:n * BLOCK + (3 if n % 2 else 0)])
    lists[G_C1] = plain(np.union1d(g[::2], np.setdiff1d(drawn(1200), g)[:900]))
    held = []
    for t, (at, freq) in T_LEADS.items():
        d = drawn(12 * BLOCK + 10)
        fr = _freqs(rng, d.size)
        fr[at] = freq
        lists[t] = (d, fr)
        held.append(d[np.arange(d.size) % 5 < 2])
    t_all = np.concatenate([lists[t][0] for t in T_LEADS])
    lists[T_C1] = plain(np.union1d(np.concatenate(held), np.setdiff1d(drawn(1500), t_all)[:800]))
    w = drawn(130 * BLOCK)
    for t, n in W_LEADS.items():
        lists[t] = plain(w[:n * BLOCK])
    lists[HALF_B] = plain(np.union1d(core[::2], drawn(1400)))
    lists[HALF_N] = plain(np.union1d(core[1::2], drawn(2900)))
    return lists



def build_norms(max_doc, kind):
    rng = np.random.default_rng([max_doc, 12])
    if kind == "none":
        return None
    if kind == "rank":
        nb = rng.integers(95, 125, size=max_doc).astype(np.uint8)
    else:
        assert kind == "raw"
        nb = RAW_BYTES[rng.integers(0, RAW_BYTES.size, size=max_doc)]
        nb[rng.permutation(CONST_LO)[:RAW_BYTES.size]] = RAW_BYTES
    if max_doc >= CONST_HI:
        nb[CONST_LO:CONST_HI] = TIE_BYTE
    return nb


def deleted_for_certain(max_doc=MAX_DOC):
    c = core_docs(max_doc)
    return [int(c[4]), int(c[5]), SPREAD_STEP * 4 + SPREAD_OFF]


def alive_for_certain(max_doc=MAX_DOC):
    c = core_docs(max_doc)
    return [0, max_doc - 1] + [int(c[i]) for i in list(OVF_PLANTS) + list(NIB_PLANTS)]


class _Built:
    def __init__(self, max_doc, lists, norms_kind, version):
        from rucene_amd import indexgen
        self.lists = lists
        self.norms = build_norms(max_doc, norms_kind)
        self.seg = indexgen.build_explicit(max_doc, lists, norms=self.norms, version=version)
        assert [int(x) for x in self.seg.terms["doc_freq"]] == [d.size for d, _ in lists]


_lists, _built, _has = {}, {}, {}


class Leaf:
    """One fixture leaf with the attributes tests/segment_spectrum.py's Leaf has, so that its set algebra takes it."""

    def __init__(self, norms="rank", live="none", version=1, big=False):
        assert norms in NORMS and live in LIVE and version in VERSIONS
        max_doc = BIG_MAX_DOC if big else MAX_DOC
        if big not in _lists:
            _lists[big] = build_big_lists() if big else build_lists()
            has = np.zeros((len(_lists[big]), max_doc), bool)
            for t, (d, _) in enumerate(_lists[big]):
                has[t, d] = True
            _has[big] = has
        key = (big, norms, version)
        if key not in _built:
            _built[key] = _Built(max_doc, _lists[big], norms, version)
        b = _built[key]
        self.key = key + (live,)
        self.big, self.max_doc, self.lists, self.norms, self.seg, self.has = big, max_doc, b.lists, b.norms, b.seg, _has[big]
        self.norms_kind, self.live, self.version, self.doc_base, self.sttf = norms, live, version, 0, STTF_PER_DOC * max_doc
        self.alive = np.ones(max_doc, bool)
        if live == "seeded":
            self.alive = np.random.default_rng([max_doc, 13]).random(max_doc) < 0.85
            self.alive[alive_for_certain(max_doc)] = True
            self.alive[deleted_for_certain(max_doc)] = False
        self.live_docs = None if live == "none" else ss.live_words(self.alive)

    def oracle_segment(self, oracle):
        return oracle.Segment(self.seg.doc_bytes, self.norms, self.max_doc, self.seg.terms, doc_base=0, live_docs=self.live_docs,
                              sum_total_term_freq=self.sttf)

    def df(self, t):
        return int(self.lists[t][0].size)

    def full_blocks(self, t):
        return 0 if self.df(t) == 1 else self.df(t) // BLOCK    # (a singleton lives in its dictionary entry)

    def tail_n(self, t):
        return 0 if self.df(t) == 1 else self.df(t) % BLOCK

    def dir_last(self, t):
        """The last doc of every FullBlock: the clause's block directory."""
        return self.lists[t][0][BLOCK - 1::BLOCK][:self.full_blocks(t)].astype(np.int64)

    def n_overflow(self, t):
        return int((self.lists[t][1] >= OVF_FREQ).sum())

    def kind(self, t, and_bitmaps=0):
        """How a clause behind the lead is answered: "walked", "memb" (membership bits alone: only right behind the lead), "bitmap"
        or "nib" (a bitmap with the four-bits-per-doc array)."""
        df, min_df = self.df(t), bitmap_min_df(self.max_doc, and_bitmaps)
        if min_df is None or df < 2:
            return "walked"
        if df >= min_df:
            if self.n_overflow(t) > BITMAP_OVF_CAP:
                return "walked"
            return "nib" if df * NIBBLE_DENSITY >= self.max_doc else "bitmap"
        return "memb" if df >= MEMB_MIN_DF else "walked"


# ---- the big leaf -------------------------------------------------------------------------------------------------------------------
BIG_BLOCKS = BIG_MAX_DOC // BLOCK
EVERY_BIG = 0
# (clause block of the lead's first block, clause block of its second block): find_block_wave starts at first + 63
BIG_DELTAS = (0, 63, 64, 65, 127, 128, 129, 64 + 4096, 64 + 4097)
BIG_PAIRS = ([(0, 63 + d) for d in BIG_DELTAS] + [(20, 83 + d) for d in (64, 65, 129, 64 + 4096)]
             + [(BIG_BLOCKS - 128 - 63, BIG_BLOCKS - 64), (BIG_BLOCKS - 128 - 63, BIG_BLOCKS - 1), (BIG_BLOCKS - 129 - 63, BIG_BLOCKS - 65),
                (BIG_BLOCKS - 129 - 63, BIG_BLOCKS - 2)])
BIG_TAIL_LEADS = 2       # block 0 / block 20 and 40 docs of the every-doc list's VInt tail: no slot qualifies
BIG_LEADS = list(range(1, 1 + len(BIG_PAIRS) + BIG_TAIL_LEADS))
BIG_NAMES = ["EVERY_BIG"] + ["B_%d_%d" % p for p in BIG_PAIRS] + ["B_TAIL_0", "B_TAIL_20"]


def build_big_lists():
    rng = np.random.default_rng([BIG_MAX_DOC, 14])
    every = np.arange(BIG_MAX_DOC, dtype=np.int32)
    lists = [(every, np.ones(BIG_MAX_DOC, np.int32))]
    for a, b in BIG_PAIRS:
        assert 0 <= a < b < BIG_BLOCKS
        d = np.concatenate([every[a * BLOCK:(a + 1) * BLOCK], every[b * BLOCK:(b + 1) * BLOCK]])
        lists.append((d, _freqs(rng, d.size)))
    for a in (0, 20):
        d = np.concatenate([every[a * BLOCK:(a + 1) * BLOCK], every[BIG_BLOCKS * BLOCK + 10:BIG_BLOCKS * BLOCK + 50]])
        lists.append((d, _freqs(rng, d.size)))
    return lists


BIG_QUERIES = [Query(must=(t, EVERY_BIG)) for t in BIG_LEADS]


# ---- queries ------------------------------------------------------------------------------------------------------------------------
def _plain():
    qs = []
    for c in KINDS:
        qs += [(CORE_LEAD, c), (EDGE_LEAD, c), (LEAD_127, c), (LEAD_128, c), (TAIL_2, c), (SING_EVEN, c), (CORE_LEAD, c, EVERY)]
    qs += [(CORE_LEAD, C_512, C_1172, C_2344, EVERY), (CORE_LEAD, C_511, C_1171, C_2343), (EDGE_LEAD, EVERY), (EDGE_LEAD, REG4), (EDGE_LEAD, C_2344, C_1172),
           (CORE_LEAD, OVF_SMALL), (CORE_LEAD, OVF_CAP), (CORE_LEAD, OVF_OVER), (CORE_LEAD, C_1172, OVF_SMALL), (EDGE_LEAD, OVF_CAP, OVF_SMALL),
           (LEAD_127, OVF_SMALL, OVF_OVER), (Q_LEAD, Q_C1), (Q_LEAD, Q_C1, EVERY), (S_LEAD, S_C1), (S_LEAD, S_C1, REG4), (S_LEAD, S_C1, SPREAD)]
    for t in G_LEADS:
        qs += [(t, G_C1), (G_C1, t, EVERY)]
    for t in T_LEADS:
        qs += [(t, T_C1), (t, T_C1, EVERY)]
    for t in W_LEADS:
        qs += [(t, EVERY), (REG4, t)]
    qs += [(FP_LEAD, SPREAD), (FP_LEAD, SPREAD_NOTAIL), (FP_LEAD, SPREAD, EVERY), (FP_LEAD, EVERY, SPREAD_NOTAIL, SPREAD), (SAME_LEAD, SPREAD),
           (SAME_LEAD, SPREAD, REG4), (WIN_LEAD, REG4), (WIN_LEAD, REG4, EVERY), (CONST, EVERY), (CONST, EVERY, EVERY), (TAIL_2, SPREAD), (TAIL_2, EVERY),
           (SING_EVEN, EVERY), (SING_EVEN, SPREAD), (SING_MISS, EVERY), (SING_EVEN, SING_ODD), (SING_EVEN, SING_EVEN), (CORE_LEAD, SING_MISS),
           (CORE_LEAD, SING_ODD), (CORE_LEAD, ABSENT), (ABSENT, EVERY), (ABSENT, ABSENT), (EQ_A, EQ_A), (C_1172, C_1172), (CORE_LEAD, CORE_LEAD),
           (CORE_LEAD, EQ_A, EQ_A), (LEAD_128, LEAD_127), (LEAD_127, TAIL_2)]
    qs += [(a, b, c) for a in (EQ_A, EQ_B, EQ_C) for b in (EQ_A, EQ_B, EQ_C) for c in (EQ_A, EQ_B, EQ_C) if len({a, b, c}) == 3]
    # 64 clauses: a walked clause at clause positions 1 and 2, and at 62 and 63 (OVF_OVER is walked whatever its doc_freq)
    qs += [(CORE_LEAD, EQ_A, EQ_A) + (C_1172,) * 61, (C_1172,) * 61 + (OVF_OVER, CORE_LEAD, OVF_OVER),
           (C_512,) * 30 + (CORE_LEAD,) + (C_2344,) * 31 + (EQ_B, OVF_OVER)]
    return [Query(must=m) for m in qs]


NOT_SETS = ((SPREAD,), (HALF_B, SING_ODD), (ABSENT, LEAD_127), (SING_EVEN, SING_MISS, Q_C1), (HALF_N,), (S_C1, LEAD_128))


def _with_not(plain):
    qs = [Query(must=q.must, must_not=NOT_SETS[i % len(NOT_SETS)]) for i, q in enumerate(plain) if len(q.must) + 3 <= 64]
    qs += [Query(must=(FP_LEAD, EVERY), must_not=(SPREAD,)), Query(must=(FP_LEAD,), must_not=(SPREAD,)),
           Query(must=(FP_LEAD,), must_not=(SPREAD_NOTAIL, SPREAD)),
           Query(must=(EDGE_LEAD, EVERY), must_not=(C_1172,)), Query(must=(EDGE_LEAD, C_512), must_not=(C_2344,)), Query(must=(EDGE_LEAD,), must_not=(C_1171,)),
           Query(must=(CORE_LEAD, C_1172), must_not=(SING_EVEN,)), Query(must=(CORE_LEAD, C_1172), must_not=(SING_ODD,)),
           Query(must=(CORE_LEAD, C_1172), must_not=(SING_MISS,)), Query(must=(CORE_LEAD, C_511), must_not=(SING_EVEN, SING_ODD)),
           Query(must=(EVERY,), must_not=(REG4,)), Query(must=(CONST,), must_not=(SING_MISS,)), Query(must=(CORE_LEAD, EVERY), must_not=(EVERY,)),
           Query(must=(CORE_LEAD,) + (C_1172,) * 61, must_not=(SING_EVEN, OVF_OVER)), Query(must=(Q_LEAD, Q_C1), must_not=(S_C1, G_C1)),
           Query(must=(S_LEAD,), must_not=(S_C1,)), Query(must=(CORE_LEAD, OVF_CAP), must_not=(OVF_SMALL,))]
    qs += [Query(must=(t,), must_not=(SPREAD,)) for t in W_LEADS]     # one MUST clause: block by block, whatever the bitmaps
    return qs


def _with_filter(plain):
    qs = []
    for i, q in enumerate(plain):
        if len(q.must) >= 2:
            qs.append(Query(must=q.must[:1], filt=q.must[1:]) if i % 2 == 0 else Query(must=q.must[1:], filt=q.must[:1]))
    qs += [Query(must=(EVERY,), filt=(CORE_LEAD,)), Query(must=(C_1172,), filt=(CORE_LEAD, SPREAD)), Query(must=(SPREAD,), filt=(FP_LEAD,)),
           Query(must=(EQ_A, EQ_B), filt=(EQ_C,)), Query(must=(EQ_C,), filt=(EQ_B, EQ_A))]
    return qs


PLAIN = _plain()
WITH_NOT = _with_not(PLAIN)
WITH_FILTER = _with_filter(PLAIN)
FAMILIES = {"plain": PLAIN, "not": WITH_NOT, "filter": WITH_FILTER}
ALL_QUERIES = PLAIN + WITH_NOT + WITH_FILTER


def mixed():
    """The three families dealt into one batch in turn -> (queries, {family: row indexes in family order})."""
    out, rows = [], {name: [] for name in FAMILIES}
    for i in range(max(len(f) for f in FAMILIES.values())):
        for name, fam in FAMILIES.items():
            if i < len(fam):
                rows[name].append(len(out))
                out.append(fam[i])
    return out, rows


def required(leaf, q):
    """The required clauses in ConjunctionScorer's order: MUST then FILTER clauses, stable by doc_freq -> [(term, scored)]."""
    cl = [(t, True) for t in q.must] + [(t, False) for t in q.filt]
    return sorted(cl, key=lambda c: leaf.df(c[0]))     # (sorted is stable)


def lead_of(leaf, q):
    return required(leaf, q)[0][0]


def matches_nothing(leaf, q):
    return any(leaf.df(t) == 0 for t in q.must + q.filt)


def items_of(leaf, q, bpi):
    """Work items of one query: chunks of the lead's FullBlocks, one for a lead without any."""
    if matches_nothing(leaf, q):
        return 0
    return max(1, -(-leaf.full_blocks(lead_of(leaf, q)) // bpi))


def batch_of_items(leaf, n_items, bpi=1):
    """Plain queries in turn until the batch has exactly n_items work items at `bpi` lead blocks per item."""
    pool = [q for q in PLAIN if 0 < items_of(leaf, q, bpi) <= 12 and len(q.must) <= 5]
    ones = [q for q in pool if items_of(leaf, q, bpi) == 1]
    out, have, i = [], 0, 0
    while have < n_items:
        q = pool[i % len(pool)]
        if have + items_of(leaf, q, bpi) > n_items:
            q = ones[i % len(ones)]
        out.append(q)
        have += items_of(leaf, q, bpi)
        i += 1
    return out


def oracle_rows(oracle, osr, queries, k):
    return ss.oracle_rows(oracle, osr, queries, k)


def ref_docs(leaf, q):
    return ss.ref_leaf_docs(leaf, q)


# ---- the numpy reference ------------------------------------------------------------------------------------------------------------
class AndRef:
    """Hit sets by set algebra over the explicit lists (MUST and FILTER lists intersected, MUST_NOT lists subtracted, deleted docs
    dropped); a doc's score the f32 sum of the oracle's per-term scores (Searcher.score_docs with OP_TERM) in ConjunctionScorer's
    order - the required clauses sorted by doc_freq, stable -, a FILTER clause adding 0."""

    def __init__(self, oracle, leaf, osr=None):
        self.oracle, self.leaf = oracle, leaf
        self.osr = osr or oracle.Searcher([leaf.oracle_segment(oracle)])
        self._scores = {}

    def term_scores(self, t):
        """The oracle's TermScorer score of every live doc of the list, as a dense f32 array over the leaf."""
        if t not in self._scores:
            docs = self.leaf.lists[t][0]
            docs = docs[self.leaf.alive[docs]].astype(np.int32)
            scores, matched = self.osr.score_docs(self.oracle.OP_TERM, [t], docs)
            assert matched.all(), ("the oracle's TermScorer does not hold a live doc of the fixture's list", t)
            dense = np.zeros(self.leaf.max_doc, np.float32)
            dense[docs] = scores
            dense.setflags(write=False)
            self._scores[t] = dense
        return self._scores[t]

    def scores(self, q):
        docs = ref_docs(self.leaf, q).astype(np.int64)
        total = None
        for t, scored in required(self.leaf, q):
            s = self.term_scores(t)[docs] if scored else np.zeros(docs.size, np.float32)
            total = s.astype(np.float32) if total is None else (total + s).astype(np.float32)
        return docs.astype(np.int32), total

    def row(self, q, k):
        """-> (docs, scores, total_hits): score descending, doc ascending, cut at k."""
        docs, sc = self.scores(q)
        order = np.lexsort((docs, -sc.astype(np.float64)))[:k]
        return docs[order], sc[order], int(docs.size)


# ---- models of the kernel's own bookkeeping -----------------------------------------------------------------------------------------
def queue_trace(leaf, lead, c1, bpi):
    """The survivor queue of the batched first probe, item by item: the lead's FullBlocks in groups of AND_G, the survivors (lead
    docs the first clause holds, deleted or not) appended, 128 popped while at least 128 wait -> per item a dict of the entries
    waiting when each group is appended (`before`), right after (`after`), each group's survivors and blocks."""
    docs, has = leaf.lists[lead][0], leaf.has[c1]
    nb = leaf.full_blocks(lead)
    out = []
    for b0 in range(0, nb, bpi):
        b1 = min(nb, b0 + bpi)
        waiting, tr = 0, dict(before=[], after=[], survivors=[], blocks=[])
        for blk in range(b0, b1, AND_G):
            n = min(AND_G, b1 - blk)
            surv = int(has[docs[blk * BLOCK:(blk + n) * BLOCK]].sum())
            tr["before"].append(waiting)
            tr["after"].append(waiting + surv)
            tr["survivors"].append(surv)
            tr["blocks"].append(n)
            assert waiting < 128 and waiting + surv <= AND_Q_CAP
            waiting = (waiting + surv) % 128 if blk + n < b1 else 0
        out.append(tr)
    return out


def find_block_wave(last, frm, target):
    """find_block_wave of search_and.hpp -> (the first slot in [frm, nblocks] whose last doc >= target, what answered):
    ("first",) the look at the 64 entries behind frm; ("loop", width at entry, rounds, "final" | "none") the 64-ary search."""
    nb = last.size
    if frm >= nb:
        return nb, ("past",)
    at = max(frm, int(np.searchsorted(last, target, "left")))
    if at < frm + 64:
        return at, ("first",)          # (at == nb: a lane past the directory reads INT_MAX)
    lo, hi, rounds = frm + 64, nb, 0
    entry = hi - lo
    while hi - lo > 64:
        stride = (hi - lo + 63) >> 6
        probes = np.minimum(lo + (np.arange(64) + 1) * stride - 1, hi - 1)
        ok = np.flatnonzero(last[probes] >= target)
        if ok.size == 0:
            return hi, ("loop", entry, rounds, "none")
        j = int(ok[0])
        hi, lo = min(lo + (j + 1) * stride - 1, hi - 1), lo + j * stride
        rounds += 1
    assert lo <= at <= hi      # the loop's invariant: every slot below lo is below the target, the answer lies in [lo, hi]
    return at, ("loop", entry, rounds, "final")


def walk(last, pending, cursor):
    """One walked clause against one vector of candidates (search_and.hpp `locate` and the pipeline behind it) -> (the FullBlocks
    decoded, the clause's cursor afterwards, events). `last`: the clause's directory; `pending`: the candidates still alive,
    ascending. Events: ("find", what find_block_wave answered with) and ("next", d) - the next pending candidate's block lies d
    slots behind the register window's start: the pipeline stays in the window up to d = 62."""
    nb = last.size
    frm = min(cursor, nb)
    decoded, events, i, first = [], [], 0, True

    def block_of(d):
        return max(frm, int(np.searchsorted(last, d, "left")))

    while i < len(pending):
        while block_of(pending[i]) > frm + 62:
            frm, what = find_block_wave(last, frm + 63, pending[i])
            events.append(("find", what))
        blk = block_of(pending[i])
        if first:
            cursor, first = blk, False
        if blk >= nb:
            break                       # the VInt tail, or nothing, answers everything that is left
        while True:
            while i < len(pending) and pending[i] <= last[blk]:
                i += 1
            decoded.append(blk)
            if i == len(pending):
                break
            nxt = block_of(pending[i])
            events.append(("next", nxt - frm))
            if nxt > frm + 62 or nxt >= nb:
                break
            blk = nxt
    return decoded, cursor, events


def vectors_of(leaf, lead):
    """The lead's candidates as the kernel takes them block by block: every FullBlock, then the VInt tail or the singleton."""
    docs = leaf.lists[lead][0]
    nb = leaf.full_blocks(lead)
    out = [docs[b * BLOCK:(b + 1) * BLOCK] for b in range(nb)]
    if docs.size > nb * BLOCK:
        out.append(docs[nb * BLOCK:])
    return out


def walked_trace(leaf, q):
    """The launch's blocks_decoded for q when every clause is walked (and_bitmaps = -1) and the query is one work item, by the window
    model -> (count, the same count by the plain rule, events): the lead's FullBlocks plus, per lead vector and clause, the clause's
    FullBlocks that hold (by their doc range) a candidate still alive."""
    if matches_nothing(leaf, q):
        return 0, 0, []
    clauses = [(t, "must") for t, _ in required(leaf, q)] + [(t, "not") for t in q.must_not]
    lead = clauses[0][0]
    count = plain = leaf.full_blocks(lead)
    cursors, events = {}, []
    for vec in vectors_of(leaf, lead):
        alive = vec[leaf.alive[vec]].astype(np.int64)
        for ti, (t, kind) in enumerate(clauses[1:], 1):
            if alive.size == 0:
                break
            if leaf.df(t) >= 2:
                last = leaf.dir_last(t)
                decoded, cursors[ti], ev = walk(last, alive, cursors.get(ti, 0))
                events += [(ti, t) + e for e in ev]
                count += len(decoded)
                at = np.searchsorted(last, alive, "left")
                plain += np.unique(at[at < last.size]).size
                assert len(set(decoded)) == len(decoded) and decoded == sorted(decoded)
            held = leaf.has[t][alive]
            alive = alive[held] if kind == "must" else alive[~held]
    return count, plain, events


def bitmap_terms(leaf, queries, and_bitmaps=0):
    """(doc_bitmap_terms, doc_bitmap_refused) of a fresh segment after `queries`: every clause (the lead included) of a conjunction
    of two or more clauses whose doc_freq reaches bitmap_min_df_and gets a bitmap, unless more than BITMAP_OVF_CAP of its freqs are >= 255."""
    min_df = bitmap_min_df(leaf.max_doc, and_bitmaps)
    seen = set()
    for q in queries:
        cl = q.must + q.filt + q.must_not
        if min_df is not None and len(cl) >= 2:
            seen.update(t for t in cl if leaf.df(t) >= min_df)
    refused = {t for t in seen if leaf.n_overflow(t) > BITMAP_OVF_CAP}
    return len(seen - refused), len(refused)


def wants_memb_only(leaf, q, and_bitmaps=0):
    """ensure_memb_only_locked is asked for the clause right behind the lead: two or more required clauses, the second smallest
    doc_freq in [512, bitmap_min_df_and), a lead of 128 docs or more."""
    min_df = bitmap_min_df(leaf.max_doc, and_bitmaps)
    req = required(leaf, q)
    if min_df is None or len(req) < 2 or matches_nothing(leaf, q):
        return False
    return leaf.df(req[0][0]) >= MEMB_MIN_LEAD and MEMB_MIN_DF <= leaf.df(req[1][0]) < min_df


def all_bitmaps_behind_the_lead(leaf, q, and_bitmaps=0):
    cl = [t for t, _ in required(leaf, q)][1:] + list(q.must_not)
    return len(cl) >= 1 and len(q.must + q.filt) >= 2 and all(leaf.kind(t, and_bitmaps) in ("bitmap", "nib") or leaf.df(t) <= 1 for t in cl)


def probe_outcomes(leaf, lead, clause):
    """Every doc of `lead` against the walked list `clause` -> (block, hit, false_positive) arrays: the FullBlock (or, at
    full_blocks, the VInt tail) whose range holds the candidate; whether that block holds it; whether it does not but holds a doc
    congruent to it modulo the filter's 2048 bits, so that the filter reports it and the compare against the docs rejects it."""
    cand, docs = leaf.lists[lead][0].astype(np.int64), leaf.lists[clause][0].astype(np.int64)
    nb, last = leaf.full_blocks(clause), leaf.dir_last(clause)
    blk = np.searchsorted(last, cand, "left")
    hit, fp = np.zeros(cand.size, bool), np.zeros(cand.size, bool)
    for i, (d, b) in enumerate(zip(cand, blk)):
        members = docs[b * BLOCK:(b + 1) * BLOCK] if b < nb else docs[nb * BLOCK:]
        hit[i] = d in members
        fp[i] = not hit[i] and bool(((members - d) % FILTER_BITS == 0).any())
    return blk, hit, fp


def lead_window_reloads(n_blocks, step):
    """Reloads of the lead's own 64-entry directory window inside one item of n_blocks lead blocks taken `step` at a time (AND_G on
    the batched probe's path, 1 block by block): `blk - lw0 > 63 - AND_G`."""
    lw0, reloads = 0, 0
    for blk in range(0, n_blocks, step):
        if blk - lw0 > 63 - AND_G:
            lw0, reloads = blk, reloads + 1
        assert blk + min(step, n_blocks - blk) - 1 - lw0 + 1 <= 63      # every block of the step has a window slot
    return reloads
