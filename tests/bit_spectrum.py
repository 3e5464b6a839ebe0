"""Bit-spectrum fixtures (plain Python, no GPU): explicit postings lists whose 128-posting FullBlocks land on chosen cells of the
space every kernel's unpackers depend on - the packed width of the doc-delta stream (0 = all-equal with a VInt of 1..3 bytes,
1..27), the packed width of the freq stream (0 = all-equal with a VInt of 1..5 bytes, 1..31; width 1 needs freqs of 0 and 1, which
no writer produces and every reader decodes), and the block's byte misalignment `(start_fp + off) & 15` in the .doc file.

Layout of the doc-id space (MAX_DOC = 2^26 + 2^22, so one 27-bit delta fits): a STEERED term starts low (at doc 0 when its first block
is to have doc width 1: deltas 0, 1, 1, ...), walks up through up to five spectrum blocks - width set by one value with the top bit
and random lower ones in every lane -, jumps into the ZONE at the top of the space for one background block (freqs 1..3, one norm byte)
that also carries three plants, and ends in a VInt tail. The builder keeps the byte position of every block it emits (block sizes,
tail bytes and the one-level skip data of a term of at most seven blocks are plain arithmetic), picks for the position at hand the
(doc option, freq option) that fills the most missing cells, and after every batch parses the bytes it really got (parse_cells) and
goes on from there until no cell is missing.

Scores are kept apart by norm byte: a posting that is not meant to win sits on a doc of byte 0 (a length near 3.7e18: even a freq of
2^31 scores below any ordinary posting of freq 1), the posting of the largest freq in every spectrum block (a PLANT) and the
background docs carry one of 63 ordinary bytes (68..130; with byte 0 that is 64 distinct bytes: rank mode), chosen so that the
plants of a term are a relative GAP apart in float64 whatever their freq. An ordinary doc belongs to one term (and to the lists
built from that term on purpose: its twin, its half, the dense list); byte-0 docs may be shared. check_separation() proves for
a query that its top k rows are GAP apart or full ties (the same freq in every clause and the same byte), which doc ids resolve."""
import numpy as np

from norm_spectrum import GAP, bm25_f64

MAX_DOC = 2 ** 26 + 2 ** 22
ZONE0 = MAX_DOC - 2 ** 21          # the zone: bump-allocated, one stretch per term
STTF = 3 * MAX_DOC
AVGDL = float(np.float32(STTF / MAX_DOC))
PAIR_WIDTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 24)
DOC_WIDTHS = tuple(range(28))
FREQ_WIDTHS = tuple(range(32))
DOC_VINT_LENGTHS = (1, 2, 3)
FREQ_VINT_LENGTHS = (1, 2, 3, 4, 5)
NOISE, BG = 0, 68
PALETTE = tuple(range(69, 131))    # the plants' bytes
HEADER_BYTES, FOOTER_BYTES = 94, 16   # indexgen.cpp begin() / finish(): index header + ForUtil table; codec footer (asserted in __init__)
MAX_STEERED_BLOCKS = 7             # one skip level only: the term's length in the file is plain arithmetic
CELL_DTYPE = np.dtype([("term", "<i4"), ("block", "<i4"), ("bd", "<i4"), ("dvl", "<i4"), ("bf", "<i4"), ("fvl", "<i4"), ("mis", "<i4")])

_DOC_VINT_RANGE = {1: (1, 128), 2: (128, 2000), 3: (16384, 20000)}
_FREQ_VINT_RANGE = {1: (1, 128), 2: (128, 2 ** 14), 3: (2 ** 14, 2 ** 21), 4: (2 ** 21, 2 ** 28), 5: (2 ** 28, 2 ** 31)}
DOC_OPTIONS = [(0, v) for v in DOC_VINT_LENGTHS] + [(b, 0) for b in range(1, 28)]
FREQ_OPTIONS = [(0, v) for v in FREQ_VINT_LENGTHS] + [(b, 0) for b in range(1, 32)]
_PAIR_FREQ_OPTIONS = [j for j, (b, _) in enumerate(FREQ_OPTIONS) if b in PAIR_WIDTHS]
_FIFTH = FREQ_OPTIONS.index((0, 5))


def vint_len(x):
    x = np.asarray(x, dtype=np.int64)
    return 1 + (x >= 2 ** 7).astype(np.int64) + (x >= 2 ** 14) + (x >= 2 ** 21) + (x >= 2 ** 28)


def doc_kind(bd, dvl):
    """What precedes a freq VInt in its block (the 5-byte VInt's fifth byte is the last byte a prepare stages when the bytes in
    front of it end 12 past a 16-byte row)."""
    return "vint%d" % dvl if bd == 0 else ("packed<=8" if bd <= 8 else "packed>=9")


DOC_KINDS = ("vint1", "vint2", "vint3", "packed<=8", "packed>=9")


def stream_bytes(b, vl):
    return 16 * b if b else vl


def cell_sets(cells):
    """The cell sets the CPU test asserts complete, from parse_cells' rows."""
    c = cells
    fifth = c[(c["bf"] == 0) & (c["fvl"] == 5)]
    last_staged = fifth[(fifth["mis"] + 6 + np.where(fifth["bd"] > 0, 16 * fifth["bd"], fifth["dvl"])) % 16 == 0]
    return {
        "doc_width_x_mis": set(zip(c["bd"].tolist(), c["mis"].tolist())),
        "freq_width_x_mis": set(zip(c["bf"].tolist(), c["mis"].tolist())),
        "pairs": set(zip(c["bd"].tolist(), c["bf"].tolist())),
        "doc_vint_lengths": set(c["dvl"][c["bd"] == 0].tolist()),
        "freq_vint_lengths": set(c["fvl"][c["bf"] == 0].tolist()),
        "fifth_byte_x_mis": set(fifth["mis"].tolist()),
        "fifth_byte_last_staged": set(doc_kind(int(r["bd"]), int(r["dvl"])) for r in last_staged),
    }


def wanted_sets():
    return {
        "doc_width_x_mis": {(b, m) for b in DOC_WIDTHS for m in range(16)},
        "freq_width_x_mis": {(b, m) for b in FREQ_WIDTHS for m in range(16)},
        "pairs": {(a, b) for a in PAIR_WIDTHS for b in PAIR_WIDTHS},
        "doc_vint_lengths": set(DOC_VINT_LENGTHS),
        "freq_vint_lengths": set(FREQ_VINT_LENGTHS),
        "fifth_byte_x_mis": set(range(16)),
        "fifth_byte_last_staged": set(DOC_KINDS),
    }


def missing_cells(cells):
    have, want = cell_sets(cells), wanted_sets()
    return {k: want[k] - have[k] for k in want if want[k] - have[k]}


def parse_cells(seg):
    """Walks the .doc bytes from the term states: one row per FullBlock - (term, block, doc width, doc VInt length, freq width, freq
    VInt length, misalignment); a VInt length is 0 for a packed stream."""
    doc = seg.doc_bytes
    rows = []
    for t, st in enumerate(seg.terms):
        df = int(st["doc_freq"])
        if df < 128:
            continue
        p = int(st["doc_start_fp"])
        for blk in range(df // 128):
            mis = p & 15
            out = [t, blk]
            p0 = p
            for _ in range(2):
                h = int(doc[p])
                assert h <= 32, (t, blk, h)
                p += 1
                vl = 0
                if h == 0:
                    vl = 1
                    while doc[p + vl - 1] & 0x80:
                        vl += 1
                    p += vl
                else:
                    p += 16 * h
                out += [h, vl]
            rows.append(tuple(out + [mis]))
            assert p > p0
    return np.array(rows, dtype=CELL_DTYPE)


# ---- blocks --------------------------------------------------------------------------------------------------------------------
def _doc_deltas(rng, bd, dvl):
    if bd == 0:
        lo, hi = _DOC_VINT_RANGE[dvl]
        return np.full(128, int(rng.integers(lo, hi)), np.int64)
    if bd == 1:
        d = np.ones(128, np.int64)
        d[0] = 0
        return d
    d = rng.integers(1, 2 ** min(bd, 8), size=128).astype(np.int64)
    lanes = rng.choice(128, size=3 if bd <= 16 else 1, replace=False)
    d[lanes] = 2 ** (bd - 1) + rng.integers(0, 2 ** min(bd - 1, 20), size=lanes.size)
    return d


def doc_span_bound(bd, dvl):
    if bd == 0:
        return 128 * _DOC_VINT_RANGE[dvl][1]
    if bd == 1:
        return 128
    return 128 * 2 ** min(bd, 8) + (3 if bd <= 16 else 1) * (2 ** (bd - 1) + 2 ** min(bd - 1, 20))


def _freqs(rng, bf, fvl):
    if bf == 0:
        lo, hi = _FREQ_VINT_RANGE[fvl]
        return np.full(128, int(rng.integers(lo, hi)), np.int64)
    if bf == 1:
        f = rng.integers(0, 2, size=128).astype(np.int64)
        f[rng.choice(128, size=2, replace=False)] = [0, 1]
        return f
    f = rng.integers(1, 2 ** bf, size=128).astype(np.int64)
    lanes = rng.choice(128, size=2, replace=False)
    f[lanes[0]] |= 2 ** (bf - 1)
    f[lanes[1]] = 1 if f[lanes[0]] != 1 else 2
    return f


def _tail_bytes(deltas, freqs):
    code = (deltas << 1) | (freqs == 1)
    return int(vint_len(code).sum() + vint_len(freqs)[freqs != 1].sum())


def unit_score(freq, byte):
    return float(bm25_f64(1000, MAX_DOC, AVGDL, freq, byte))


class BitSpectrum:
    """The SEARCH fixture: self.lists (docs, freqs per term), self.norms, self.seg[version], self.cells[version], and the roles of
    its terms: steered (dict per term: plants, background docs), LONG terms, twins / halves of some steered terms, DENSE."""

    def __init__(self, seed=2718):
        from rucene_amd import indexgen
        self.rng = rng = np.random.default_rng(seed)
        self.lists, self.info = [], []
        self.norms = np.zeros(MAX_DOC, np.uint8)            # NOISE everywhere until a term claims a doc
        self.used = np.zeros(MAX_DOC, bool)                 # docs some list holds
        self.zone_cursor = ZONE0
        self._long_terms()
        self.n_long = len(self.lists)
        # ---- steered terms, batch by batch, until parse_cells finds every cell
        pos = HEADER_BYTES + self._long_bytes
        cells = np.zeros(0, CELL_DTYPE)
        self.rounds = 0
        while True:
            seg = indexgen.build_explicit(MAX_DOC, self.lists, norms=None, version=1)
            assert len(seg.doc_bytes) - FOOTER_BYTES == pos, ("the builder's byte arithmetic", len(seg.doc_bytes) - FOOTER_BYTES, pos)
            cells = parse_cells(seg)
            miss = missing_cells(cells)
            if not miss:
                break
            self.rounds += 1
            assert self.rounds <= 40 and len(self.lists) < 700, ("cells that would not fill", {k: sorted(v)[:8] for k, v in miss.items()})
            self._have = {k: set(v) for k, v in cell_sets(cells).items()}
            for _ in range(40):
                pos += self._steered_term(pos)
        self.n_steered_end = len(self.lists)
        self.steered = list(range(self.n_long, self.n_steered_end))
        self._companions()
        self.seg, self.cells = {}, {}
        for version in (1, 0):
            self.seg[version] = indexgen.build_explicit(MAX_DOC, self.lists, norms=self.norms, version=version)
            self.cells[version] = parse_cells(self.seg[version])
        assert np.count_nonzero(np.bincount(self.norms, minlength=256)) <= 64

    # ---- bytes a term takes in the file (at most MAX_STEERED_BLOCKS FullBlocks + tail: level-0 skip entries only) -------------------
    def _term_bytes(self, docs, freqs, sizes=None):
        df = docs.size
        if df == 1:
            return 0
        nfull = df // 128
        d = np.diff(np.concatenate([[0], docs.astype(np.int64)]))
        if sizes is None:
            sizes = []
            for b in range(nfull):
                dd, ff = d[128 * b:128 * b + 128], freqs[128 * b:128 * b + 128].astype(np.int64)
                bd = 0 if (dd == dd[0]).all() else int(dd.max()).bit_length()
                bf = 0 if (ff == ff[0]).all() else int(ff.max()).bit_length()
                sizes.append(2 + (16 * bd if bd else int(vint_len(dd[0]))) + (16 * bf if bf else int(vint_len(ff[0]))))
        total = sum(sizes) + _tail_bytes(d[128 * nfull:], freqs[128 * nfull:].astype(np.int64))
        if df > 128:
            assert nfull <= MAX_STEERED_BLOCKS
            n_entries = nfull - 1 + (1 if df % 128 and nfull else 0)
            last_doc, fp = 0, 0
            ends = np.cumsum(sizes)
            skip = 0
            for e in range(n_entries):
                bdoc = int(docs[128 * e + 127])
                skip += int(vint_len(bdoc - last_doc)) + int(vint_len(int(ends[e]) - fp))
                last_doc, fp = bdoc, int(ends[e])
            total += skip
        return total

    def _claim(self, docs, byte):
        self.norms[docs] = byte

    def _plant(self, scores, freq):
        """A byte for a plant of this freq: above the background (freq 3 on byte BG) and GAP-separated (four times over) from the
        scores its term already has."""
        floor = unit_score(3, BG)
        for byte in self.rng.permutation(PALETTE):
            s = unit_score(freq, int(byte))
            if s > floor and all(abs(s - o) > 4 * GAP * max(s, o) for o in scores):
                scores.append(s)
                return int(byte)
        raise AssertionError("no byte keeps a plant of freq %d apart" % freq)

    def _background(self, scores, n=128):
        """One block's worth of background docs in the zone (freqs 1..3 on byte BG) carrying three plants of freq 4..10."""
        rng = self.rng
        docs = self.zone_cursor + np.cumsum(rng.integers(1, 4, size=n))
        freqs = rng.integers(1, 4, size=n).astype(np.int64)
        freqs[:3] = [1, 2, 3]
        lanes = rng.choice(np.arange(3, n), size=3, replace=False)
        freqs[lanes] = rng.choice(np.arange(4, 11), size=3, replace=False)
        return docs, freqs, lanes

    # ---- the long lists: 130+ blocks, spectrum blocks on both sides of the 64-block chunk edge ----------------------------------------
    def _long_terms(self):
        from rucene_amd import indexgen
        rng = self.rng
        plans = [{63: ((17, 0), (31, 0)), 64: ((24, 0), (1, 0)), 100: ((0, 2), (0, 5)), 128: ((9, 0), (0, 3)), 131: ((16, 0), (16, 0))},
                 {0: ((1, 0), (24, 0)), 63: ((4, 0), (2, 0)), 64: ((2, 0), (4, 0)), 127: ((0, 3), (1, 0)), 128: ((15, 0), (17, 0)), 139: ((25, 0), (9, 0))}]
        start = 2 ** 20
        for plan in plans:
            nblocks = 140
            scores = [unit_score(f, BG) for f in (1, 2, 3)]
            deltas, freqs, plant_at = [], [], []
            for b in range(nblocks):
                if b in plan:
                    (bd, dvl), (bf, fvl) = plan[b]
                    d, f = _doc_deltas(rng, bd, dvl), _freqs(rng, bf, fvl)
                    if bd != 1:
                        plant_at.append(128 * b + int(np.argmax(f)))
                else:
                    d, f = rng.integers(1, 4, size=128).astype(np.int64), rng.integers(1, 4, size=128).astype(np.int64)
                if b == (1 if 0 in plan else 0):
                    d[0] += start
                deltas.append(d)
                freqs.append(f)
            tail_d, tail_f = rng.integers(1, 4, size=61).astype(np.int64), rng.integers(1, 4, size=61).astype(np.int64)
            tail_f[40] = 7
            plant_at.append(128 * nblocks + 40)
            docs = np.cumsum(np.concatenate(deltas + [tail_d]))
            freqs = np.concatenate(freqs + [tail_f])
            assert docs[-1] < ZONE0 and not self.used[docs].any()
            start = int(docs[-1]) + 1000
            noise = np.zeros(docs.size, bool)
            for b in plan:
                noise[128 * b:128 * b + 128] = True
            noise[plant_at] = False
            self._claim(docs[~noise], BG)
            for at in plant_at:
                self._claim(docs[at], self._plant(scores, int(freqs[at])))
            self.used[docs] = True
            self.lists.append((docs.astype(np.int32), freqs.astype(np.int32)))
            self.info.append({"kind": "long", "plants": docs[plant_at].astype(np.int32), "blocks": sorted(plan)})
        # (their length in the file, higher skip levels included, is measured: the steered terms' is arithmetic)
        seg = indexgen.build_explicit(MAX_DOC, self.lists, norms=None, version=1)
        self._long_bytes = len(seg.doc_bytes) - FOOTER_BYTES - HEADER_BYTES

    # ---- one steered term ---------------------------------------------------------------------------------------------------------------
    def _gain(self, mis, first, room):
        """The (doc option, freq option) that fills the most missing cells for a block at this misalignment."""
        have = self._have
        nd, nf = len(DOC_OPTIONS), len(FREQ_OPTIONS)
        g = self.rng.random((nd, nf)) * 0.5
        for i, (bd, dvl) in enumerate(DOC_OPTIONS):
            if (bd == 1 and not first) or (first and 2 <= bd < 14) or doc_span_bound(bd, dvl) > room:
                g[i, :] = -1e9
                continue
            g[i, :] += ((bd, mis) not in have["doc_width_x_mis"]) + (bd == 0 and dvl not in have["doc_vint_lengths"]) - 0.002 * bd
            if bd in PAIR_WIDTHS:
                for j in _PAIR_FREQ_OPTIONS:
                    g[i, j] += (bd, FREQ_OPTIONS[j][0]) not in have["pairs"]
            g[i, _FIFTH] += mis not in have["fifth_byte_x_mis"]
            if (mis + 6 + stream_bytes(bd, dvl)) % 16 == 0 and doc_kind(bd, dvl) not in have["fifth_byte_last_staged"]:
                g[i, _FIFTH] += 3
        for j, (bf, fvl) in enumerate(FREQ_OPTIONS):
            g[:, j] += ((bf, mis) not in have["freq_width_x_mis"]) + (bf == 0 and fvl not in have["freq_vint_lengths"])
        i, j = np.unravel_index(int(np.argmax(g)), g.shape)
        return DOC_OPTIONS[i], FREQ_OPTIONS[j]

    def _steered_term(self, pos):
        """Appends one term whose first byte is at `pos`; returns its length in the file."""
        rng = self.rng
        for _ in range(50):
            have_before = {k: set(v) for k, v in self._have.items()}
            p = pos
            prev = 0
            deltas, freqs, sizes, plant_at = [], [], [], []
            nspec = int(rng.integers(3, MAX_STEERED_BLOCKS - 1))
            for b in range(nspec):
                first = b == 0
                (bd, dvl), (bf, fvl) = self._gain(p & 15, first, ZONE0 - 1 - prev)
                d, f = _doc_deltas(rng, bd, dvl), _freqs(rng, bf, fvl)
                mis = p & 15
                h = self._have
                h["doc_width_x_mis"].add((bd, mis)); h["freq_width_x_mis"].add((bf, mis)); h["pairs"].add((bd, bf))
                if bd == 0:
                    h["doc_vint_lengths"].add(dvl)
                if bf == 0:
                    h["freq_vint_lengths"].add(fvl)
                    if fvl == 5:
                        h["fifth_byte_x_mis"].add(mis)
                        if (mis + 6 + stream_bytes(bd, dvl)) % 16 == 0:
                            h["fifth_byte_last_staged"].add(doc_kind(bd, dvl))
                deltas.append(d); freqs.append(f)
                sizes.append(2 + stream_bytes(bd, dvl) + stream_bytes(bf, fvl))
                if bd != 1:   # (docs 0..127 are every width-1 block's: nobody's plant)
                    plant_at.append(128 * b + int(np.argmax(f)))
                p += sizes[-1]
                prev += int(d.sum())
            assert prev < ZONE0
            scores = [unit_score(f, BG) for f in (1, 2, 3)]
            bg_docs, bg_freqs, bg_lanes = self._background(scores)
            ntail = int(rng.integers(0, 100))
            tail_d, tail_f = rng.integers(1, 9, size=ntail).astype(np.int64), rng.integers(1, 4, size=ntail).astype(np.int64)
            spec_docs = np.cumsum(np.concatenate(deltas))
            tail_docs = bg_docs[-1] + np.cumsum(tail_d)
            docs = np.concatenate([spec_docs, bg_docs, tail_docs])
            fr = np.concatenate(freqs + [bg_freqs, tail_f])
            plants = np.array(plant_at + [128 * nspec + int(x) for x in bg_lanes] + ([128 * (nspec + 1) + ntail // 2] if ntail else []))
            is_plant = np.zeros(docs.size, bool)
            is_plant[plants] = True
            spec = np.arange(docs.size) < 128 * nspec
            # ordinary docs are this term's alone; its byte-0 docs may be shared with other byte-0 docs only
            if self.used[docs[is_plant | ~spec]].any() or (self.norms[docs[spec & ~is_plant]] != NOISE).any() or docs[-1] >= MAX_DOC:
                self._have = have_before
                continue
            sizes.append(2 + 16 * int(np.diff(docs[128 * nspec - 1:128 * nspec + 128]).max()).bit_length() + 16 * int(bg_freqs.max()).bit_length())
            self._claim(docs[~spec], BG)
            if ntail:
                tail_noise = 128 * (nspec + 1) + np.arange(ntail)
                self._claim(docs[tail_noise], NOISE)
            for at in plants:
                self._claim(docs[at], self._plant(scores, int(fr[at])))
            self.used[docs] = True
            self.zone_cursor = int(docs[-1]) + 1
            assert self.zone_cursor < MAX_DOC - 4096, "the zone is full"
            self.lists.append((docs.astype(np.int32), fr.astype(np.int32)))
            self.info.append({"kind": "steered", "plants": docs[plants].astype(np.int32), "bg": bg_docs.astype(np.int32), "nspec": nspec})
            return self._term_bytes(self.lists[-1][0], self.lists[-1][1], sizes)
        raise AssertionError("fifty draws of a term met other terms' ordinary docs")

    # ---- twins, halves, the dense list ----------------------------------------------------------------------------------------------------
    def _companions(self):
        rng = self.rng
        self.twins, self.halves = {}, {}
        picks = [self.steered[i] for i in (0, len(self.steered) // 3, len(self.steered) // 2, len(self.steered) - 1)] + [0]
        for t in picks:
            docs, freqs = self.lists[t]
            f2 = np.empty(docs.size, np.int64)
            for b in range(docs.size // 128):
                bf = int(rng.integers(0, 13))
                f2[128 * b:128 * b + 128] = _freqs(rng, bf, int(rng.integers(1, 4)) if bf == 0 else 0)
            f2[128 * (docs.size // 128):] = rng.integers(1, 4, size=docs.size % 128)
            ordinary = self.norms[docs] != NOISE
            f2[ordinary] = freqs[ordinary]   # (a twin has its term's df, so its idf: freqs 2 + 3 and 3 + 2 would tie without being full ties)
            at = np.searchsorted(docs, self.info[t]["plants"])
            f2[at] = 4 + (np.arange(at.size) * 3 + 1) % 7
            self.twins[t] = len(self.lists)
            self.lists.append((docs.copy(), f2.astype(np.int32)))
            self.info.append({"kind": "twin", "of": t})
            if self.info[t]["kind"] == "steered":   # the "half": every eighth background doc and the first plant, a tail-only term
                hd = np.unique(np.concatenate([self.info[t]["bg"][::8], self.info[t]["plants"][:1]]))
                self.halves[t] = len(self.lists)
                self.lists.append((hd.astype(np.int32), np.ones(hd.size, np.int32)))
                self.info.append({"kind": "half", "of": t})
        # DENSE: seven zone docs in eight and every ordinary one, freq 2 (above the bitmap density of 1 doc in 64)
        zone = np.arange(ZONE0, MAX_DOC, dtype=np.int64)
        keep = (rng.random(zone.size) < 0.875) | (self.norms[zone] != NOISE)
        keep &= self.used[zone] | (zone % 5 != 0)
        docs = zone[keep]
        unowned = ~self.used[docs]
        self._claim(docs[unowned], BG)
        freqs = np.full(docs.size, 2, np.int64)
        freqs[:128 * (docs.size // 128 // 2)] = 1 + (docs[:128 * (docs.size // 128 // 2)] % 2)
        self.dense = len(self.lists)
        assert docs.size > MAX_DOC // 64 + 128
        self.lists.append((docs.astype(np.int32), freqs.astype(np.int32)))
        self.info.append({"kind": "dense"})
        self.used[docs] = True

    # ---- what the tests ask -------------------------------------------------------------------------------------------------------------------
    def queries(self, oracle):
        """(op, positive terms, MUST_NOT terms) of every search the GPU module runs, at k = 10 and 100."""
        if getattr(self, "_queries", None) is not None:
            return self._queries
        T, A, O = oracle.OP_TERM, oracle.OP_AND, oracle.OP_OR
        q = [(T, [t], []) for t in range(len(self.lists))]
        st = self.steered
        some = st[::max(1, len(st) // 12)]
        for t, tw in self.twins.items():
            q += [(A, [t, tw], []), (O, [t, tw], []), (A, [tw, t, self.dense], []), (O, [t, tw, self.dense], [])]
            if t in self.halves:
                q += [(T, [t], [self.halves[t]]), (O, [t, tw], [self.halves[t]]), (A, [t, tw], [self.halves[t]])]
        q += [(A, [t, self.dense], []) for t in some] + [(A, [self.dense, t], []) for t in some[:3]]
        # disjunctions of unrelated steered terms: their plants were kept apart term by term, not across terms, so the terms of
        # a group are picked (in float64, here) such that the union's top rows are apart too
        def group(start, n):
            for shift in range(len(st) - n):
                g = [st[(start + shift + 7 * i) % len(st)] for i in range(n)]
                if len(set(g)) == n and self._apart(False, g, []):
                    return g
            raise AssertionError("no group of %d steered terms whose union is apart" % n)
        q += [(O, group(11 * i, 3), []) for i in range(4)]
        q += [(O, group(5, 8), []), (O, [0, 1], []), (O, [0, self.twins[0], st[0]], []), (T, [self.dense], [some[0]]), (O, [some[1], self.dense], [some[2]])]
        self._queries = q
        return q

    def rows_f64(self, op_is_and, pos, neg):
        """Every matching doc of a query with its float64 BM25 and its tie key (the freq in each clause, the byte)."""
        parts = [self.lists[t] for t in pos]
        alld = np.concatenate([d for d, _ in parts])
        docs, inv = np.unique(alld, return_inverse=True)
        score = np.zeros(docs.size)
        key = np.zeros((docs.size, len(pos) + 1), np.int64)
        count = np.zeros(docs.size, np.int64)
        o = 0
        for c, (d, f) in enumerate(parts):
            ix = inv[o:o + d.size]
            o += d.size
            if d.size:
                score[ix] += bm25_f64(d.size, MAX_DOC, AVGDL, f, self.norms[d])
                key[ix, c] = f.astype(np.int64) + 1
                count[ix] += 1
        key[:, -1] = self.norms[docs]
        ok = count == len(pos) if op_is_and else count > 0
        for t in neg:
            ok &= ~np.isin(docs, self.lists[t][0])
        return docs[ok], score[ok], key[ok]

    def _apart(self, op_is_and, pos, neg):
        try:
            for k in (10, 100):
                self.check_separation(op_is_and, pos, neg, k)
        except AssertionError:
            return False
        return True

    def check_separation(self, op_is_and, pos, neg, k):
        docs, score, key = self.rows_f64(op_is_and, pos, neg)
        n = min(k + 1, docs.size)
        top = np.lexsort((docs, -score))[:n] if docs.size <= 4096 else None
        if top is None:
            cut = np.partition(score, docs.size - n)[docs.size - n]
            cand = np.flatnonzero(score >= cut * (1 - 10 * GAP))
            top = cand[np.lexsort((docs[cand], -score[cand]))][:n]
        s, ky = score[top], key[top]
        for i in range(n - 1):
            tie = (ky[i] == ky[i + 1]).all()
            assert tie or s[i] - s[i + 1] > GAP * s[i], ("rows", i, i + 1, "neither apart nor a full tie", pos, neg, k, s[i], s[i + 1], ky[i], ky[i + 1])
        return docs[top], s


_built = {}


def search_fixture():
    if "search" not in _built:
        _built["search"] = BitSpectrum()
    return _built["search"]


# ---- the WIDE segment: decode only, no norms, max_doc 2^31 - 1 ------------------------------------------------------------------------
WIDE_MAX_DOC = 2 ** 31 - 1
WIDE_DOC_WIDTHS = (28, 29, 30, 31)


def wide_wanted():
    """(doc width, "packed" | "equal" freq stream) for 28..31, and the all-equal doc block of a 4-byte VInt under both."""
    return {(w, kind) for w in WIDE_DOC_WIDTHS for kind in ("packed", "equal")} | {("vint4", "packed"), ("vint4", "equal")}


def wide_cell_set(cells):
    out = set()
    for c in cells:
        kind = "equal" if c["bf"] == 0 else "packed"
        if c["bd"] in WIDE_DOC_WIDTHS:
            out.add((int(c["bd"]), kind))
        if c["bd"] == 0 and c["dvl"] == 4:
            out.add(("vint4", kind))
    return out


class WideSpectrum:
    """Terms of one ordinary block, then one block of doc width 28..31 (a term holds one: the deltas of a list sum below 2^31) or an
    all-equal doc block whose delta needs a 4-byte VInt (128 deltas of 2^21..2^22), as a term's first block and behind another one,
    under packed freqs of widths 2..31 and all-equal ones of every VInt length; tails of 0..90 postings move the misalignment."""

    def __init__(self, seed=31):
        from rucene_amd import indexgen
        rng = np.random.default_rng(seed)
        self.lists = []
        fvl = 0
        for rep in range(3):
            for shape in list(WIDE_DOC_WIDTHS) + ["vint4"]:
                for kind in ("packed", "equal"):
                    for lead in (True, False):
                        if shape == "vint4":
                            d = np.full(128, int(rng.integers(2 ** 21, 2 ** 22)), np.int64)
                        else:
                            d = rng.integers(1, 256, size=128).astype(np.int64)
                            d[int(rng.integers(0, 128))] = 2 ** (shape - 1) + int(rng.integers(0, 2 ** 20))
                        fvl = fvl % 5 + 1
                        f = _freqs(rng, 0, fvl) if kind == "equal" else _freqs(rng, int(rng.integers(2, 32)), 0)
                        deltas, freqs = [d], [f]
                        if lead:
                            deltas.insert(0, rng.integers(1, 8, size=128).astype(np.int64))
                            freqs.insert(0, rng.integers(1, 4, size=128).astype(np.int64))
                        ntail = int(rng.integers(0, 91))
                        deltas.append(rng.integers(1, 50, size=ntail).astype(np.int64))
                        freqs.append(rng.integers(1, 9, size=ntail).astype(np.int64))
                        docs = np.cumsum(np.concatenate(deltas))
                        assert docs[-1] < WIDE_MAX_DOC
                        self.lists.append((docs.astype(np.int32), np.concatenate(freqs).astype(np.int32)))
        self.seg, self.cells = {}, {}
        for version in (1, 0):
            self.seg[version] = indexgen.build_explicit(WIDE_MAX_DOC, self.lists, norms=None, version=version)
            self.cells[version] = parse_cells(self.seg[version])


def wide_fixture():
    if "wide" not in _built:
        _built["wide"] = WideSpectrum()
    return _built["wide"]


# ---- a bulk first touch: the search fixture's long and steered lists in front of 33 000 two- and three-posting terms ------------------
BULK_FILLERS = 33_000   # rgpu_decode_terms plans a first touch of >= 32768 new terms in file order with several host threads


def bulk_segment(fx, version):
    """(segment, number of leading terms that are fx.lists' - at the same bytes, so fx.cells names their blocks)."""
    from rucene_amd import indexgen
    rng = np.random.default_rng(99)
    n = fx.n_steered_end
    fill = []
    for i in range(BULK_FILLERS):
        df = 2 + i % 2
        fill.append((np.sort(rng.choice(100_000, size=df, replace=False)).astype(np.int32) + 7 * i, np.full(df, 1 + i % 3, np.int32)))
    seg = indexgen.build_explicit(MAX_DOC, fx.lists[:n] + fill, norms=None, version=version)
    assert (seg.terms["doc_start_fp"][:n] == fx.seg[version].terms["doc_start_fp"][:n]).all()
    return seg, n, fill


# ---- positions --------------------------------------------------------------------------------------------------------------------------
POS_MAX_DOC = 6000
POS_MAX_WIDTH = 31        # N: positions are i32, so the 128 deltas of a block sum below 2^31: one delta of 2^30 and small ones
POS_SHAPES = [(0, 1), (0, 2)] + [(b, 0) for b in range(1, POS_MAX_WIDTH + 1)]
POS_CELL_DTYPE = np.dtype([("term", "<i4"), ("block", "<i4"), ("b", "<i4"), ("vl", "<i4"), ("mis", "<i4")])


def _position_deltas(rng, b, vl):
    if b == 0:
        return np.full(128, int(rng.integers(1, 128) if vl == 1 else rng.integers(128, 2 ** 14)), np.int64)
    if b == 1:
        d = np.ones(128, np.int64)   # positions 0, 1, 2, ...: the first delta of a doc is its first position
        d[0] = 0
        return d
    d = rng.integers(1, 2 ** min(b, 6), size=128).astype(np.int64)
    d[int(rng.integers(1, 128))] = 2 ** (b - 1) + int(rng.integers(0, 2 ** min(b - 1, 20)))
    return d


def parse_pos_cells(seg):
    """One row per packed block of the .pos file: (term, block, width, VInt length of an all-equal block, misalignment)."""
    pos = seg.pos_bytes
    rows = []
    for t, st in enumerate(seg.terms):
        if st["doc_freq"] == 0:
            continue
        p = int(seg.pos_start_fp[t])
        for blk in range(int(st["total_term_freq"]) // 128):
            mis, h = p & 15, int(pos[p])
            assert h <= 32
            p += 1
            vl = 0
            if h == 0:
                vl = 1
                while pos[p + vl - 1] & 0x80:
                    vl += 1
            p += 16 * h if h else vl
            rows.append((t, blk, h, vl, mis))
    return np.array(rows, dtype=POS_CELL_DTYPE)


class PositionSpectrum:
    """Term 0 (FIRST): docs of 128 positions each, so that a doc is one block of the .pos file, its deltas of one shape of
    POS_SHAPES (every shape three times, in a shuffled order), and a last doc of five positions (the VInt block). Term 1 (NEXT)
    holds the same docs with every position + 1, term 2 (THIRD) every other one of them with position + 3, term 3 (ALONE) a
    doc of its own: "FIRST NEXT" matches exactly at every position, "FIRST THIRD" within slop 2."""
    FIRST, NEXT, THIRD, ALONE = 0, 1, 2, 3

    def __init__(self, seed=17):
        from rucene_amd import indexgen
        rng = np.random.default_rng(seed)
        shapes = [POS_SHAPES[i] for i in rng.permutation(np.repeat(np.arange(len(POS_SHAPES)), 3))]
        docs = np.sort(rng.choice(POS_MAX_DOC - 10, size=len(shapes) + 1, replace=False)) + 1
        first = [(int(d), np.cumsum(_position_deltas(rng, b, vl)).tolist()) for d, (b, vl) in zip(docs[:-1], shapes)]
        first.append((int(docs[-1]), [3, 4, 90, 1000, 70_000]))
        self.shapes = shapes
        self.postings = [first, [(d, [p + 1 for p in ps]) for d, ps in first], [(d, [p + 3 for p in ps]) for d, ps in first[::2]],
                         [(POS_MAX_DOC - 1, [0, 5])]]
        self.norms = rng.integers(90, 131, size=POS_MAX_DOC).astype(np.uint8)
        self.doc_count = len(docs) + 1
        self.sum_ttf = sum(len(ps) for pl in self.postings for _, ps in pl)
        self.phrases = [([0, 1], 0), ([1, 0], 0), ([0, 2], 0), ([0, 1], 2), ([0, 2], 2), ([2, 0], 2), ([1, 2], 2), ([0, 3], 0), ([0, 1, 2], 2)]
        self.seg, self.cells = {}, {}
        for version in (1, 0):
            self.seg[version] = indexgen.build_explicit_positions(POS_MAX_DOC, self.postings, norms=self.norms, version=version)
            self.cells[version] = parse_pos_cells(self.seg[version])

    def flat_positions(self):
        return np.array([p for pl in self.postings for _, ps in pl for p in ps], dtype=np.int32)


def positions_fixture():
    if "pos" not in _built:
        _built["pos"] = PositionSpectrum()
    return _built["pos"]
