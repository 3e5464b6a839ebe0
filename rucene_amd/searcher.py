"""Host-side mirror of the slice of Rucene's search API that the GPU path serves, with the reference's names,
argument meaning and error behaviour so tests read like the reference's own (paths relative to
/root/reference/src/core):

    search/searcher.rs:205-249, 306-363, 487-525, 732-767   IndexSearcher::search, statistics quirk
    search/query/term_query.rs:45-95                         TermQuery::new(term, boost) / create_weight
    search/query/boolean_query.rs:40-86                      BooleanQuery::build(musts, shoulds, ...)
    search/query/disjunction_max_query.rs:43-114             DisjunctionMaxQuery { disjuncts, tie_breaker_multiplier }
    search/query/boosting_query.rs:29-118                    BoostingQuery::build(positive, negative, negative_boost)
    search/similarity/bm25_similarity.rs:45-177              BM25Similarity::new(k1, b) / compute_weight
    search/collector/top_docs.rs:97-183                      TopDocsCollector::new(k) / top_docs()
    search/statistics.rs                                     CollectionStatistics / TermStatistics

    index/reader/directory_reader.rs, segment_reader.rs      open_directory: commit point -> segments -> per-format readers

Terms are named by bytes and resolved through each leaf's block-tree dictionary (rgpu_terms_*), or — synthetic indexes —
by an id into a flat table of BlockTermState records. All scoring work happens in librucene_gpu.so; this module only
resolves terms, computes BM25 weights (via the C ABI's host helper) and packs query structs.
"""
import numpy as np

from . import _lib
from ._lib import OP_AND, OP_DISMAX, OP_NESTED_MUST, OP_OR, OP_SHOULD_REQUIRED, OP_TERM, QUERY_DTYPE, QUERY_TERM_DTYPE, TERM_STATE_DTYPE, RgpuError


class CollectionStatistics:
    """search/statistics.rs CollectionStatistics (field-level)."""

    def __init__(self, field, doc_base, max_doc, doc_count, sum_total_term_freq, sum_doc_freq=-1):
        self.field, self.doc_base, self.max_doc = field, doc_base, max_doc
        self.doc_count, self.sum_total_term_freq, self.sum_doc_freq = doc_count, sum_total_term_freq, sum_doc_freq


class BM25Similarity:
    """bm25_similarity.rs:45-63. compute_weight returns (weight, cache[256]) == BM25SimWeight{weight, cache}."""
    DEFAULT_BM25_K1 = 1.2
    DEFAULT_BM25_B = 0.75

    def __init__(self, k1=DEFAULT_BM25_K1, b=DEFAULT_BM25_B):
        self.k1, self.b = float(np.float32(k1)), float(np.float32(b))

    def compute_weight(self, collection_stats, doc_freqs, boost=1.0):
        w, _idf, cache = _lib.bm25_compute_weight(self.k1, self.b, collection_stats.max_doc, collection_stats.doc_count,
                                                  collection_stats.sum_total_term_freq, doc_freqs, boost)
        return w, cache

    @staticmethod
    def encode_norm_value(boost, field_length):
        return _lib.bm25_encode_norm(boost, field_length)

    def __str__(self):
        return "BM25Similarity(k1: %s, b: %s)" % (self.k1, self.b)


class ExtraField:
    """A further indexed field of a leaf's segment (LeafReader.extra_fields): its number, norms, FieldReader statistics, index
    options and term lookup - a flat table of term states indexed by term id, or the leaf's block-tree dictionary under the
    field's number. `slot`: the field slot of the uploaded segment (rgpu_segment_attach_field), set by the searcher."""

    def __init__(self, name, field_number, norms, doc_count, sum_total_term_freq, index_options=_lib.INDEX_OPTIONS_DOCS_AND_FREQS,
                 has_payloads=False, terms=None, term_dictionary=None, sum_doc_freq=-1):
        self.name, self.field_number, self.norms = str(name), int(field_number), norms
        self.doc_count, self.sum_total_term_freq, self.sum_doc_freq = int(doc_count), int(sum_total_term_freq), int(sum_doc_freq)
        self.index_options, self.has_payloads = int(index_options), bool(has_payloads)
        self.terms = None if terms is None else np.ascontiguousarray(terms, dtype=TERM_STATE_DTYPE)
        self.term_dictionary = term_dictionary
        self._resolved = {}
        self.slot = None

    def term_state(self, term):
        """None when the term is absent from this field of the leaf"""
        if isinstance(term, bytes):
            if term not in self._resolved:
                if self.term_dictionary is None:
                    raise RgpuError(-2, "field %r of this leaf has no term dictionary: query it by term id" % self.name)
                states, found = self.term_dictionary.lookup(self.field_number, [term])
                if len(self._resolved) >= LeafReader.RESOLVED_CACHE_TERMS:
                    self._resolved.clear()
                self._resolved[term] = states[0].copy() if found[0] else None
            return self._resolved[term]
        if self.terms is None or term < 0 or term >= self.terms.size or self.terms[term]["doc_freq"] <= 0:
            return None
        return self.terms[term]


class LeafReader:
    """One segment as the searcher sees it (index/reader/leaf_reader.rs:62-182, reduced to what BM25 term and
    boolean queries read): postings file, norms, live docs, FieldReader statistics, and the term dictionary — either a
    flat table of term states indexed by term id (synthetic indexes) or a block-tree dictionary (`.tim`/`.tip`) keyed
    by term bytes."""

    RESOLVED_CACHE_TERMS = 1 << 20   # bound of the per-leaf memo of resolved byte terms

    def __init__(self, doc_bytes, norms, max_doc, terms, doc_base=0, live_docs=None, doc_count=None,
                 sum_total_term_freq=0, sum_doc_freq=-1, field="body", term_dictionary=None, field_number=0,
                 index_options=_lib.INDEX_OPTIONS_DOCS_AND_FREQS, has_payloads=False):
        self.doc_bytes, self.norms, self.max_doc, self.doc_base = doc_bytes, norms, int(max_doc), int(doc_base)
        self.terms = np.ascontiguousarray(terms if terms is not None else [], dtype=TERM_STATE_DTYPE)
        self.live_docs = live_docs
        self.doc_count = int(max_doc if doc_count is None else doc_count)
        self.sum_total_term_freq, self.sum_doc_freq, self.field = int(sum_total_term_freq), int(sum_doc_freq), field
        self.term_dictionary, self.field_number = term_dictionary, int(field_number)
        self.index_options = int(index_options)  # doc::IndexOptions ordinal: 1 Docs, 2 DocsAndFreqs, 3 DocsAndFreqsAndPositions, 4 ...AndOffsets
        self.has_payloads = bool(has_payloads)   # FieldInfo::has_store_payloads
        self.pos_bytes = None      # the ".pos" file of a positions field
        self.pay_bytes = None      # the ".pay" file of a field that stores payloads or offsets
        self.term_positions = None  # per flat term id: TERM_POSITIONS_DTYPE records (synthetic segments)
        self._resolved = {}  # term bytes -> state or None
        self.segment = None  # rgpu_segment, created by the searcher
        self.extra_fields = {}  # name -> ExtraField: the segment's further indexed fields a query may name (TermQuery(field=...))

    def add_field(self, name, norms, terms, doc_count=None, sum_total_term_freq=0, index_options=_lib.INDEX_OPTIONS_DOCS_AND_FREQS,
                  field_number=None):
        """Declare a further field of a synthetic leaf: `terms` are the term states of ITS terms in the leaf's one .doc file."""
        number = len(self.extra_fields) + 1 + self.field_number if field_number is None else field_number
        self.extra_fields[name] = ExtraField(name, number, norms, self.max_doc if doc_count is None else doc_count, sum_total_term_freq,
                                             index_options, terms=terms)
        return self.extra_fields[name]

    @classmethod
    def from_synthetic(cls, seg, doc_base=None):
        return cls(seg.doc_bytes, seg.norms, seg.max_doc, seg.terms, seg.doc_base if doc_base is None else doc_base,
                   seg.live_docs, seg.doc_count, seg.sum_total_term_freq, seg.sum_doc_freq)

    @classmethod
    def from_synthetic_positions(cls, seg, doc_base=None, offsets=False, payloads=False):
        """A synthetic DocsAndFreqsAndPositions field (indexgen.build_explicit_positions): .doc + .pos + per-term pointers;
        offsets / payloads: as the segment was built (+ .pay)."""
        leaf = cls(seg.doc_bytes, seg.norms, seg.max_doc, seg.terms, seg.doc_base if doc_base is None else doc_base,
                   seg.live_docs, seg.doc_count, seg.sum_total_term_freq, seg.sum_doc_freq,
                   index_options=_lib.INDEX_OPTIONS_OFFSETS if offsets else _lib.INDEX_OPTIONS_POSITIONS, has_payloads=payloads)
        leaf.pos_bytes = seg.pos_bytes
        leaf.pay_bytes = seg.pay_bytes
        tp = np.zeros(seg.terms.size, dtype=_lib.TERM_POSITIONS_DTYPE)
        tp["pos_start_fp"], tp["last_pos_block_offset"] = seg.pos_start_fp, seg.last_pos_block_offset
        if seg.pay_start_fp is not None:
            tp["pay_start_fp"] = seg.pay_start_fp
        leaf.term_positions = tp
        return leaf

    def positions_state(self, term):
        """The position-stream pointers of BlockTermState for `term` (None when the term is absent)."""
        if isinstance(term, bytes):
            if self.term_dictionary is None:
                raise RgpuError(-2, "this leaf has no term dictionary: query it by term id")
            states, pos, found = self.term_dictionary.lookup_positions(self.field_number, [term])
            return (states[0], pos[0]) if found[0] else None
        st = self.term_state(term)
        if st is None or self.term_positions is None:
            return None
        return st, self.term_positions[term]

    @classmethod
    def from_index_files(cls, doc, tim, tip, nvm, nvd, max_doc, field_number=0, index_options=2, liv=None, del_count=-1,
                         doc_base=0, field="body", other_fields=(), fnm=None, has_payloads=False, extra_fields=()):
        """A segment as Rucene wrote it (SegmentReader::open -> the per-format producers): `.doc` postings, `.tim`/`.tip`
        block-tree term dictionary, `.nvm`/`.nvd` norms, optional `.liv` live docs. With `fnm` (the segment's field infos
        file) the searched field is found by its name `field` and every other indexed field is declared from the file;
        otherwise pass `field_number`/`index_options` and `other_fields`: (number, index_options[, has_payloads]) of the
        segment's other indexed fields (the `.tim` summary lists them all).
        Any indexed field can be searched; for phrases set `pos_bytes` (and, for a field with payloads / offsets, `pay_bytes`).
        extra_fields: names of further indexed fields (needs `fnm`) that queries may name beside `field`: each gets its norms from
        `.nvm` / `.nvd` (none when the field omits them), its statistics from `.tim` and its term lookup from the same dictionary."""
        if extra_fields and fnm is None:
            raise RgpuError(-2, "extra_fields are found by name: pass the segment's .fnm")
        if fnm is not None:
            infos = _lib.field_infos_from_lucene60(fnm)
            mine = [fi for fi in infos if fi["name"] == field]
            if not mine:
                raise RgpuError(-2, "no field named %r in this segment" % field)
            field_number, index_options, has_payloads = mine[0]["number"], mine[0]["index_options"], bool(mine[0]["has_payloads"])
            other_fields = [(fi["number"], fi["index_options"], int(fi["has_payloads"])) for fi in infos
                            if fi["index_options"] != 0 and fi["name"] != field]
        if index_options not in (_lib.INDEX_OPTIONS_DOCS, _lib.INDEX_OPTIONS_DOCS_AND_FREQS, _lib.INDEX_OPTIONS_POSITIONS, _lib.INDEX_OPTIONS_OFFSETS):
            raise RgpuError(-5, "the searched field must be indexed (IndexOptions::Docs ... ::DocsAndFreqsAndPositionsAndOffsets)")
        td = _lib.TermDictionary(tim, tip, [(field_number, index_options, int(has_payloads))] + list(other_fields), max_doc)
        stats = td.field_stats(field_number)
        if stats is None:
            raise RgpuError(-2, "field %d has no postings in this segment" % field_number)
        norms = _lib.norms_from_lucene53(nvm, nvd, field_number, max_doc)
        live = _lib.live_docs_from_lucene50(liv, max_doc, del_count) if liv is not None else None
        leaf = cls(doc, norms, max_doc, None, doc_base, live, stats["doc_count"], stats["sum_total_term_freq"],
                   stats["sum_doc_freq"], field, td, field_number, index_options, has_payloads)
        for name in extra_fields:
            fi = [x for x in infos if x["name"] == name and x["index_options"] != 0]
            if not fi or name == field:
                raise RgpuError(-2, "no further indexed field named %r in this segment" % name)
            fi = fi[0]
            fstats = td.field_stats(fi["number"])
            if fstats is None:   # the field has no postings in this segment: every term of it is absent here
                fstats = dict(doc_count=0, sum_total_term_freq=0, sum_doc_freq=0)
            fnorms = None if fi.get("omit_norms") else _lib.norms_from_lucene53(nvm, nvd, fi["number"], max_doc)
            leaf.extra_fields[name] = ExtraField(name, fi["number"], fnorms, fstats["doc_count"], fstats["sum_total_term_freq"], fi["index_options"],
                                                 bool(fi["has_payloads"]), term_dictionary=td, sum_doc_freq=fstats["sum_doc_freq"])
        return leaf

    def resolve(self, terms):
        """One batched dictionary lookup for the byte terms not seen before (seek_exact + term_state each)."""
        new = [t for t in dict.fromkeys(terms) if isinstance(t, bytes) and t not in self._resolved]
        if not new:
            return
        if self.term_dictionary is None:
            raise RgpuError(-2, "this leaf has no term dictionary: query it by term id")
        states, found = self.term_dictionary.lookup(self.field_number, new)
        if len(self._resolved) + len(new) > self.RESOLVED_CACHE_TERMS:   # a memo, not an index: start over rather than grow forever
            self._resolved.clear()
        for t, st, ok in zip(new, states, found):
            self._resolved[t] = st if ok else None

    def term_state(self, term):
        """TermIterator::seek_exact + term_state(); None when the term is absent from this leaf."""
        if isinstance(term, bytes):
            if term not in self._resolved:
                self.resolve([term])
            return self._resolved[term]
        if term < 0 or term >= self.terms.size or self.terms[term]["doc_freq"] <= 0:
            return None
        return self.terms[term]


def _base36(v):
    digits, out = "0123456789abcdefghijklmnopqrstuvwxyz", ""
    while True:
        out = digits[v % 36] + out
        v //= 36
        if v == 0:
            return out


def open_directory(path, field="body", extra_fields=()):
    """StandardDirectoryReader::open for the slice this path needs: the newest commit point `segments_N` names the
    segments; per segment `.si` gives max_doc, `.fnm` the field's number and index options, `_Lucene50_0.{doc,tim,tip}` the
    postings and term dictionary, `.nvm/.nvd` the norms, `_<delgen>.liv` the live docs (index/reader/directory_reader.rs:
    90-140; segment_reader.rs open; file names per codec/segment_infos/mod.rs:60-114). Returns the LeafReaders with
    cumulative doc bases, ready for GpuIndexSearcher; extra_fields: further indexed fields by name (LeafReader.extra_fields). A compound segment's files are taken out of its `.cfs` through the
    `.cfe` entry table (codec/compound.rs); its `.si` and `.liv` stay outside, as Rucene writes them."""
    import os
    gens = [int(f[len("segments_"):], 36) for f in os.listdir(path) if f.startswith("segments_")]
    if not gens:
        raise RgpuError(-6, "no segments_N file found in %s" % path)   # IndexNotFound
    gen = max(gens)

    def read(name):
        with open(os.path.join(path, name), "rb") as fh:
            return fh.read()
    leaves, doc_base = [], 0
    for seg in _lib.commit_from_segments_file(read("segments_" + _base36(gen)), gen):
        name = seg["name"]
        info = _lib.segment_info_from_lucene62(read(name + ".si"), expected_id=seg["id"])
        inner = None
        if info["is_compound_file"]:
            inner = _lib.compound_files_from_lucene50(read(name + ".cfe"), read(name + ".cfs"), expected_id=seg["id"])

        def part(suffix, _inner=inner, _name=name):   # a file of this segment, from the directory or from inside its .cfs
            if _inner is None:
                return read(_name + suffix)
            if suffix not in _inner:
                raise RgpuError(-6, "%s%s is not in the compound file" % (_name, suffix))
            return _inner[suffix]
        # field infos rewritten by a doc-values update live outside the compound file under a generation suffix
        # (SegmentCommitInfo::field_infos_gen; file_name_from_generation, codec/segment_infos/mod.rs:100-114)
        fnm = read("%s_%s.fnm" % (name, _base36(seg["field_infos_gen"]))) if seg["field_infos_gen"] > 0 else part(".fnm")
        if seg["del_count"] > info["max_doc"]:
            raise RgpuError(-4, "invalid deletion count: %d vs maxDoc=%d" % (seg["del_count"], info["max_doc"]))
        # postings files carry PerFieldPostingsFormat's suffix: format "Lucene50", suffix "0" (field_infos/mod.rs:441-447)
        liv = read("%s_%s.liv" % (name, _base36(seg["del_gen"]))) if seg["del_gen"] >= 0 and seg["del_count"] > 0 else None
        leaf = LeafReader.from_index_files(np.frombuffer(part("_Lucene50_0.doc"), dtype=np.uint8), part("_Lucene50_0.tim"),
                                           part("_Lucene50_0.tip"), part(".nvm"), part(".nvd"), info["max_doc"],
                                           liv=liv, del_count=seg["del_count"] if liv is not None else -1, doc_base=doc_base,
                                           field=field, fnm=fnm, extra_fields=extra_fields)
        leaves.append(leaf)
        doc_base += info["max_doc"]
    return leaves


def _i32(op):
    """rgpu_query.op is an int32: RGPU_OP_NESTED_AT(i >= 32) sets its sign bit"""
    return ((int(op) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


class TermQuery:
    """term: bytes (resolved through each leaf's term dictionary) or an int term id (synthetic flat term table)."""

    def __init__(self, term, boost=1.0, field=None):
        """field: the name of the indexed field the term lives in; None = the leaf's primary field (LeafReader.field). Another
        field must be one of the leaves' extra_fields: such clauses are served by rgpu_search_fields_batch."""
        self.term = bytes(term) if isinstance(term, (bytes, bytearray, memoryview)) else int(term)
        self.boost = float(boost)
        self.field = None if field is None else str(field)

    def extract_terms(self):
        return [self]

    def __str__(self):
        return "TermQuery(field: %s, term: %r, boost: %s)" % (self.field or "body", self.term, self.boost)


class PhraseQuery:
    """PhraseQuery::build / ::new (query/phrase_query.rs:60-130): terms at positions 0, 1, 2, ... (or `positions`); slop 0 = an
    exact phrase, slop > 0 = the reference's SloppyPhraseScorer."""

    def __init__(self, terms, positions=None, boost=1.0, slop=0):
        self.terms = [bytes(t) if isinstance(t, (bytes, bytearray, memoryview)) else int(t) for t in terms]
        self.positions = list(range(len(self.terms))) if positions is None else [int(p) for p in positions]
        self.boost = float(boost)
        self.slop = int(slop)
        if self.slop < 0:
            raise RgpuError(-2, "Slop must be >= 0, got %d" % self.slop)
        if len(self.terms) < 2:
            raise RgpuError(-2, "PhraseWeight does not support less than 2 terms, call rewrite first")
        if len(self.positions) != len(self.terms):
            raise RgpuError(-2, "Must have as many terms as positions")


class SpanTermQuery:
    """query/spans/span_term.rs: the spans [position, position + 1) of one term. Served as a clause of a SpanNearQuery
    (whose weight takes the near query's boost alone: a clause's `boost` only travels with extract_terms)."""

    def __init__(self, term, boost=1.0):
        self.term = bytes(term) if isinstance(term, (bytes, bytearray, memoryview)) else int(term)
        self.boost = float(boost)

    def extract_terms(self):
        return [TermQuery(self.term, self.boost)]

    def __str__(self):
        return "SpanTermQuery(field: body, term: %r)" % (self.term,)


class SpanNearQuery:
    """SpanNearQuery::new (query/spans/span_near.rs:101-124): `clauses` within `slop` positions of each other, in the clauses' order
    when in_order. The GPU path serves a top-level query with in_order=True whose clauses are all SpanTermQuery
    (rgpu_search_span_near_batch), and the same shape with in_order=False (NearSpansUnordered, rgpu_search_span_unordered_batch) on a
    searcher made with unordered_spans=True. Unordered near on any other searcher and nested span clauses are UnsupportedOperation
    when the query is searched, i.e. the caller's CPU path, and so is a span query inside BooleanQuery, FilterQuery,
    DisjunctionMaxQuery, BoostingQuery or a rescoring.
    The weight sums the idf of every clause's term, a term named twice counted twice (build_sim_weight, span.rs:574-602)."""

    def __init__(self, clauses, slop=0, in_order=True, boost=1.0):
        self.clauses = list(clauses)
        self.slop, self.in_order, self.boost = int(slop), bool(in_order), float(boost)
        if len(self.clauses) < 2:
            raise RgpuError(-2, "clauses length must not be smaller than 2!")
        if not all(isinstance(c, (SpanTermQuery, SpanNearQuery)) for c in self.clauses):
            raise RgpuError(-2, "SpanNearQuery takes span queries as clauses")

    def served_by_gpu(self, unordered_spans=False):
        """None, or why the GPU path leaves this query to the CPU searcher. unordered_spans: the searcher's opt-in - without it
        unordered near is refused, as it is for every caller that has not opted in."""
        if not self.in_order and not unordered_spans:
            return "an unordered SpanNearQuery is not served by the GPU path"
        if not all(isinstance(c, SpanTermQuery) for c in self.clauses):
            return "a SpanNearQuery with nested span clauses is not served by the GPU path"
        if len(self.clauses) > _lib.MAX_PHRASE_TERMS:
            return "a SpanNearQuery of more than %d clauses is not served by the GPU path" % _lib.MAX_PHRASE_TERMS
        if self.slop < 0:   # (NearSpansOrdered would match nothing: match_width >= 0; NearSpansUnordered could, the call refuses it)
            return "a SpanNearQuery with a negative slop is not served by the GPU path"
        return None

    # the phrase packer's view of the query (GpuIndexSearcher.pack_phrases): clause i's term at "position" i
    @property
    def terms(self):
        return [c.term for c in self.clauses]

    @property
    def positions(self):
        return list(range(len(self.clauses)))

    def extract_terms(self):
        return [t for c in self.clauses for t in c.extract_terms()]

    def __str__(self):
        return "SpanNearQuery(clauses: [%s], slop: %d, in_order: %s)" % (", ".join(str(c) for c in self.clauses), self.slop, str(self.in_order).lower())


def _holds_span(query):
    """a span query anywhere inside `query`"""
    if isinstance(query, (SpanTermQuery, SpanNearQuery)):
        return True
    if isinstance(query, BooleanQuery):
        return any(_holds_span(q) for q in list(query.must_queries) + list(query.should_queries) + list(query.must_not_queries) + list(query.filter_queries))
    if isinstance(query, FilterQuery):
        return _holds_span(query.query)
    if isinstance(query, DisjunctionMaxQuery):
        return any(_holds_span(q) for q in query.disjuncts)
    if isinstance(query, BoostingQuery):
        return _holds_span(query.positive) or _holds_span(query.negative)
    return False


def _refuse_unserved_spans(query, unordered_spans=False):
    """UnsupportedOperation for every span query but a top-level SpanNearQuery over SpanTermQuery clauses - ordered, or, on a
    searcher that opted in (unordered_spans), unordered"""
    if isinstance(query, SpanNearQuery):
        why = query.served_by_gpu(unordered_spans)
        if why:
            raise RgpuError(-5, why)
    elif _holds_span(query):
        raise RgpuError(-5, "a span query is served by the GPU path as a top-level SpanNearQuery only")


class PointRangeQuery:
    """search/query/point_range_query.rs: the docs that hold a point of `field` with lower <= value <= upper, both ends inclusive,
    in unsigned byte order of the sortable bytes. ONE dimension: `lower_bytes` / `upper_bytes` are one encoded value each (4 or 8
    bytes; IntPoint / LongPoint / FloatPoint / DoublePoint below build them); a query built with num_dims > 1 is
    UnsupportedOperation (what it matches depends on the BKD cell layout: include/rucene_gpu.h). It does not score: ConstantScoreScorer(0.0) under
    MUST and FILTER alike (PointRangeWeight::new :482 — nothing normalises the weight), so GpuIndexSearcher turns the clause into
    a doc set (range_filter) and searches masked; under SHOULD, alone, or beside a phrase (unless the searcher was made with
    filtered_phrases=True and the phrase is exact) it is UnsupportedOperation."""

    def __init__(self, field, lower_bytes, upper_bytes, num_dims=1):
        self.field, self.lower, self.upper, self.num_dims = str(field), bytes(lower_bytes), bytes(upper_bytes), int(num_dims)
        if self.num_dims < 1 or len(self.lower) % self.num_dims:   # PointRangeQuery::new :384-390
            raise RgpuError(-2, "lowerPoint is not a fixed multiple of numDims")
        if len(self.lower) != len(self.upper):   # :391-397
            raise RgpuError(-2, "lowerPoint has length=%d but upperPoint has different length=%d" % (len(self.lower), len(self.upper)))
        if len(self.lower) == 0:
            raise RgpuError(-2, "a point range needs bounds")

    def extract_terms(self):
        return []

    def __str__(self):
        return "PointRangeQuery(field: %s, lower: %s, upper: %s)" % (self.field, self.lower.hex(), self.upper.hex())


class MatchAllDocsQuery:
    """search/query/match_all_query.rs: every doc, ConstantScoreScorer with the weight's default of 0.0 (nothing normalises it).
    BooleanQuery::build gives a query of MUST_NOT clauses alone one as its MUST clause (boolean_query.rs:76-79). Served by a
    searcher made with required_sets=True, alone and under `musts=`: as a required clause it is the every-doc set."""

    def extract_terms(self):
        return []

    def __str__(self):
        return "MatchAllDocsQuery()"


class _RequiredSet:
    """What _peel leaves of a query whose only required clauses are doc sets: its SHOULD side, TermQuery clauses of boost > 0
    (none: every doc of the sets at score 0). Searched through rgpu_search_batch_required_set."""

    def __init__(self, shoulds):
        self.shoulds = list(shoulds)


class _Point:
    """One-dimensional point types: encode = encode_dimension (the sortable bytes), new_range_query / new_exact_query as in the
    reference (point_range_query.rs:83-310)."""
    BYTES = 0

    @classmethod
    def new_range_query(cls, field, lower, upper):
        return PointRangeQuery(field, cls.encode(lower), cls.encode(upper))

    @classmethod
    def new_exact_query(cls, field, value):
        return cls.new_range_query(field, value, value)


class IntPoint(_Point):
    BYTES = 4

    @staticmethod
    def encode(value):   # core/util/numeric.rs:190-197 int2sortable_bytes: the sign bit flipped, big-endian
        return (((int(value) & 0xFFFFFFFF) ^ 0x80000000)).to_bytes(4, "big")


class LongPoint(_Point):
    BYTES = 8

    @staticmethod
    def encode(value):   # numeric.rs:208-218 long2sortable_bytes
        return ((int(value) & 0xFFFFFFFFFFFFFFFF) ^ 0x8000000000000000).to_bytes(8, "big")


class FloatPoint(_Point):
    BYTES = 4

    @staticmethod
    def encode(value):   # numeric.rs:171-186 float2sortable_int (bits ^ ((bits >> 31) & 0x7fffffff), arithmetic shift), then int2sortable_bytes
        bits = int(np.array([value], dtype=np.float32).view(np.int32)[0])
        return IntPoint.encode(bits ^ ((bits >> 31) & 0x7FFFFFFF))


class DoublePoint(_Point):
    BYTES = 8

    @staticmethod
    def encode(value):   # numeric.rs:163-182 double2sortable_long, then long2sortable_bytes
        bits = int(np.array([value], dtype=np.float64).view(np.int64)[0])
        return LongPoint.encode(bits ^ ((bits >> 63) & 0x7FFFFFFFFFFFFFFF))


class CachedFilter:
    """A filter that is not a term, as the query cache holds it: one doc set per leaf of a searcher, in HBM (rgpu_docset). What
    LRUQueryCache::do_cache leaves behind for a cached weight (search/cache/query_cache.rs:301-372) — made by
    GpuIndexSearcher.cache_filter (the GPU collects a term / boolean query's matches, live docs not applied), range_filter (a
    PointRangeQuery over attached points, built on the GPU), filter_from_docs (global doc ids, e.g. an ACL) or filter_from_bits
    (FixedBitSet words per leaf). Goes under
    `filters=` / `must_nots=` of BooleanQuery.build and into FilterQuery."""

    def __init__(self, searcher, sets):
        self.searcher, self.sets = searcher, list(sets)

    def cardinality(self):
        return sum(s.cardinality for s in self.sets)

    def close(self):
        for s in self.sets:
            s.close()


class FilterQuery:
    """query/filter_query.rs:155-233: `query`'s docs and scores, restricted to the docs every one of `filters` (CachedFilter)
    holds. Served by the GPU path when `query` is a term / boolean / dismax / boosting query (rgpu_search_batch_masked); a phrase
    underneath is UnsupportedOperation, i.e. the caller's CPU path, unless the searcher was made with filtered_phrases=True (exact
    phrases and the boolean queries over them then go through the masked phrase calls)."""

    def __init__(self, query, filters):
        self.query, self.filters = query, list(filters)
        if not self.filters or not all(isinstance(f, CachedFilter) for f in self.filters):
            raise RgpuError(-2, "FilterQuery takes a query and at least one CachedFilter")

    def extract_terms(self):
        return self.query.extract_terms()


class BooleanQuery:
    """Only the trees the GPU path serves: all-SHOULD with any min_should_match (OR), or MUST clauses (AND) with optional
    SHOULD clauses beside them (ReqOptScorer, boolean_query.rs:253-262 — its sequential skipping rule included unless the
    context was opened with req_opt_rule=-1, see RGPU_OP_WITH_SHOULD in include/rucene_gpu.h); each optionally with MUST_NOT TermQuery clauses
    (ReqNotScorer, boolean_query.rs:235-273). FILTER clauses are required clauses that score 0 (create_weight with
    needs_scores = false -> NonScoringSimilarity, boolean_query.rs:106-108, searcher.rs:158-202): they ride as MUST clauses
    of weight 0, which leaves every f32 sum unchanged."""

    def __init__(self, must_queries, should_queries, min_should_match, must_not_queries=(), filter_queries=()):
        self.must_queries, self.should_queries, self.min_should_match = must_queries, should_queries, min_should_match
        self.must_not_queries = list(must_not_queries)
        self.filter_queries = list(filter_queries)

    @staticmethod
    def build(musts, shoulds, filters=(), must_nots=(), min_should_match=0):
        # boolean_query.rs:40-86
        msm = min_should_match if min_should_match > 0 else (1 if len(musts) == 0 else 0)
        if len(musts) + len(shoulds) + len(filters) + len(must_nots) == 0:
            raise RgpuError(-2, "boolean query should at least contain one inner query!")
        if any(isinstance(q, CachedFilter) for q in list(musts) + list(shoulds)):
            raise RgpuError(-2, "a CachedFilter does not score: it goes under filters= or must_nots=")
        if any(isinstance(q, PointRangeQuery) for q in shoulds):
            raise RgpuError(-5, "a point range under SHOULD is not served by the GPU path")
        if len(must_nots) == 0 and len(musts) + len(shoulds) + len(filters) == 1 and not (filters and isinstance(filters[0], (CachedFilter, PointRangeQuery))):
            if filters:   # ConstantScoreQuery::with_boost(filter, 0.0) (boolean_query.rs:70-73): every match scores 0
                if isinstance(filters[0], PhraseQuery):
                    return PhraseQuery(filters[0].terms, filters[0].positions, 0.0, filters[0].slop)
                return TermQuery(filters[0].term, 0.0)
            return (list(musts) + list(shoulds))[0]
        if msm > 255:
            raise RgpuError(-5, "min_should_match above 255")
        if (musts or filters) and not shoulds:
            msm = 0   # nothing for it to count (beside MUST clauses it has no effect anyway: ReqOptScorer only advances the optional scorer)
        # (a clause that is itself a BooleanQuery builds, as it does in the reference: whether the GPU path serves the tree is
        # decided when it is searched — GpuIndexSearcher.flatten_nested / cpu_fallback)
        # (so does a PhraseQuery clause: GpuIndexSearcher.phrase_bool_parts says which trees over phrases the GPU path serves)
        # (a CachedFilter under FILTER / MUST_NOT is a doc-set clause: GpuIndexSearcher.search_batch peels it off and masks the search)
        # (a PointRangeQuery under MUST / FILTER / MUST_NOT likewise: GpuIndexSearcher.range_filter makes its doc set)
        # (a MatchAllDocsQuery under MUST is the every-doc set: GpuIndexSearcher(required_sets=True). A query of MUST_NOT clauses alone
        # gets one from the reference's build(); here the searcher supplies it when it peels such a query, the tree stays as given)
        # (a span clause builds too; no tree with one is served: GpuIndexSearcher.search_batch refuses it as UnsupportedOperation)
        spans = (SpanTermQuery, SpanNearQuery)
        # (a DisjunctionMaxQuery clause builds: the multi-field query "(title:a | body:a) (title:b | body:b)"; it is served when its
        # terms name a further field of the leaves - GpuIndexSearcher routes such trees to rgpu_search_fields_batch - and is
        # UnsupportedOperation when searched otherwise)
        if any(not isinstance(q, (TermQuery, BooleanQuery, PhraseQuery, PointRangeQuery, MatchAllDocsQuery, DisjunctionMaxQuery) + spans) for q in list(musts)) or \
                any(not isinstance(q, (TermQuery, BooleanQuery, PhraseQuery, DisjunctionMaxQuery) + spans) for q in list(shoulds)) or \
                any(not isinstance(q, (TermQuery, BooleanQuery, PhraseQuery, CachedFilter, PointRangeQuery) + spans) for q in list(must_nots) + list(filters)):
            raise RgpuError(-5, "only term, phrase and boolean clauses are known to this mirror")
        return BooleanQuery(list(musts), list(shoulds), msm, list(must_nots), list(filters))

    def normalized(self):
        """Nested clauses that do NOT score, in their exact flat forms (same docs, counts and f32 sums as the reference's scorer tree),
        or self when there is none of that shape:
          * a MUST_NOT clause that is a should-only BooleanQuery of terms, "-(b c)": ReqNotScorer excludes what the nested
            DisjunctionSumScorer matches — the MUST_NOT clauses b, c. (boolean_query.rs:236-252 puts ONE disjunction over the MUST_NOT
            scorers with the OUTER min_should_match: the same exclusion only while that is <= 1; above it the clause stays nested.)
          * a FILTER clause that is a must- / filter-only BooleanQuery of terms, "#(+b +c)": its weights are created with
            needs_scores = false (boolean_query.rs:106-108), each clause scores 0.0 and the nested conjunction's 0.0 + 0.0 joins the outer
            sum as one 0.0 — the FILTER clauses b, c (x + 0.0 == x wherever the cost order puts them).
          * a FILTER clause that is a should-only BooleanQuery of terms, "+a #(b c)": the required disjunction of zero-boost clauses."""
        must_nots, filters, changed = [], [], False
        for q in self.must_not_queries:
            if (isinstance(q, BooleanQuery) and self.min_should_match <= 1 and q.is_flat() and q.should_queries and q.min_should_match <= 1
                    and not (q.must_queries or q.must_not_queries or q.filter_queries)):
                must_nots.extend(q.should_queries)
                changed = True
            else:
                must_nots.append(q)
        musts = list(self.must_queries)
        for q in self.filter_queries:
            if (isinstance(q, BooleanQuery) and q.is_flat() and (q.must_queries or q.filter_queries)
                    and not (q.should_queries or q.must_not_queries)):
                filters.extend(q.must_queries + q.filter_queries)
                changed = True
            elif (isinstance(q, BooleanQuery) and q.is_flat() and 1 <= len(q.should_queries) <= 9 and q.min_should_match <= 1
                    and not (q.must_queries or q.filter_queries or q.must_not_queries)
                    and not self.should_queries and all(isinstance(m, TermQuery) for m in self.must_queries) and not any(isinstance(m, BooleanQuery) for m in musts)):
                # "+a #(b c)" — a filter by a disjunction ("category is b or c"): the required disjunction "+a +(b c)" whose clauses score
                # 0.0 (needs_scores = false): ConjunctionScorer([a ..., DisjunctionSumScorer(b, c)]) adds (0.0 + 0.0) somewhere in
                # the cost order, which leaves the f32 sum of the scoring clauses as it is. Behind the MUST clauses, where
                # BooleanQuery::create_weight puts the FILTER weights (boolean_query.rs:101-108). One such clause per query.
                musts.append(BooleanQuery([], [TermQuery(t.term, 0.0) for t in q.should_queries], q.min_should_match))
                changed = True
            else:
                filters.append(q)
        return BooleanQuery(musts, list(self.should_queries), self.min_should_match, must_nots, filters) if changed else self

    def is_flat(self):
        return all(isinstance(q, TermQuery) for q in self.must_queries + self.should_queries + self.must_not_queries + self.filter_queries)

    def flattened(self):
        """ONE level of nesting folded into this query, or None when the tree is not of that shape: a MUST clause that is itself a
        must-only BooleanQuery of terms, a SHOULD clause that is a should-only one (min_should_match <= 1) — what query builders that
        AND / OR sub-expressions together produce. The reference does not rewrite such trees (boolean_query.rs:195-279 builds a
        ConjunctionScorer over [a, ConjunctionScorer(b, c)]): doc ids and hit counts are those of the flat query, but its f32 sums
        are formed as a + (b + c) where the flat query forms (a + b) + c — equal within 1e-5 relative (north_star's tolerance for
        floats), NOT bit for bit; a top-k boundary inside such a rounding band may fall differently. Opt-in for that reason."""
        def fold(clauses, want_must):
            out = []
            for q in clauses:
                if isinstance(q, TermQuery):
                    out.append(q)
                    continue
                if not isinstance(q, BooleanQuery) or not q.is_flat() or q.must_not_queries or q.filter_queries:
                    return None
                if want_must and q.must_queries and not q.should_queries:
                    out.extend(q.must_queries)
                elif not want_must and q.should_queries and not q.must_queries and q.min_should_match <= 1:
                    out.extend(q.should_queries)
                else:
                    return None
            return out
        if not all(isinstance(q, TermQuery) for q in self.must_not_queries + self.filter_queries):
            return None
        musts = fold(self.must_queries, True)
        if musts is None:
            return None
        if musts or self.filter_queries:   # SHOULD clauses beside MUST ones stay as they are (ReqOptScorer's optional side)
            if not all(isinstance(q, TermQuery) for q in self.should_queries):
                return None
            return BooleanQuery(musts, list(self.should_queries), self.min_should_match, self.must_not_queries, self.filter_queries)
        shoulds = fold(self.should_queries, False)
        if shoulds is None or (self.min_should_match > 1 and len(shoulds) != len(self.should_queries)):
            return None   # (min_should_match counts the OUTER clauses: folding would change what it counts)
        return BooleanQuery([], shoulds, self.min_should_match, self.must_not_queries, [])

    def required_disjunction(self):
        """"+a +(b c)": MUST TermQuery clauses and exactly ONE MUST clause that is a should-only BooleanQuery of 1..9 terms
        (min_should_match <= 1), no SHOULD clause of its own -> (that nested query) else None. BooleanWeight::create_scorer builds
        ConjunctionScorer([TermScorer ..., DisjunctionSumScorer]) for it (boolean_query.rs:200-215); the C ABI takes it as
        RGPU_OP_WITH_SHOULD(AND, n) | RGPU_OP_SHOULD_REQUIRED."""
        if self.should_queries or not all(isinstance(q, TermQuery) for q in self.must_not_queries + self.filter_queries):
            return None
        nested = [q for q in self.must_queries if not isinstance(q, TermQuery)]
        if len(nested) != 1:
            return None
        d = nested[0]
        if (not isinstance(d, BooleanQuery) or not d.is_flat() or d.must_queries or d.must_not_queries or d.filter_queries or d.min_should_match > 1
                or not 1 <= len(d.should_queries) <= 9):
            return None
        return d

    def nested_disjunction_first(self):
        """"(b c) a d" / "a (b c) d": a should-only query whose FIRST or SECOND clause is itself a should-only BooleanQuery of terms ->
        the flat disjunction with the nested clauses moved to the front, else None. DisjunctionSumScorer sums its children in
        clause order from 0.0 (SimpleQueue, below ten children: disjunction_scorer.rs:41-45, 211-225), the nested scorer's own sum
        formed first: (a + (b + c)) + d. The flat query [b, c, a, d] forms ((b + c) + a) + d — the same f32, because the one add
        that differs has two operands and commutes (a doc without a, or without b / c, drops the absent terms from both sums alike).
        Same docs, same hit count, same score bits: no tolerance, no flag. Fewer than ten clauses in all (the clause-order kernel)."""
        if self.must_queries or self.filter_queries or self.min_should_match > 1:
            return None
        if not all(isinstance(q, TermQuery) for q in self.must_not_queries):
            return None
        nested = [i for i, q in enumerate(self.should_queries) if not isinstance(q, TermQuery)]
        if len(nested) != 1 or nested[0] > 1:
            return None
        d = self.should_queries[nested[0]]
        if (not isinstance(d, BooleanQuery) or not d.is_flat() or d.must_queries or d.must_not_queries or d.filter_queries or d.min_should_match > 1
                or not d.should_queries):
            return None
        rest = [q for q in self.should_queries if q is not d]
        if len(d.should_queries) + len(rest) >= 10:
            return None
        return BooleanQuery([], list(d.should_queries) + rest, self.min_should_match, self.must_not_queries, [])

    def nested_conjunction(self):
        """"+a +(+b +c)": MUST TermQuery clauses and exactly ONE MUST clause that is a must-only BooleanQuery of >= 2 terms, no SHOULD
        clause of its own -> (that nested query) else None. The reference builds ConjunctionScorer([TermScorer ...,
        ConjunctionScorer(b, c)]) (boolean_query.rs:200-215): the nested sum is formed first. The C ABI takes it as
        RGPU_OP_WITH_SHOULD(AND, n) | RGPU_OP_NESTED_MUST."""
        if self.should_queries or not all(isinstance(q, TermQuery) for q in self.must_not_queries + self.filter_queries):
            return None
        nested = [q for q in self.must_queries if not isinstance(q, TermQuery)]
        if len(nested) != 1:
            return None
        c = nested[0]
        if not isinstance(c, BooleanQuery) or not c.is_flat() or c.should_queries or c.must_not_queries or c.filter_queries or len(c.must_queries) < 2:
            return None
        return c

    def has_phrases(self):
        """some clause of this query (not of a nested one) is a PhraseQuery"""
        return any(isinstance(q, PhraseQuery) for q in self.must_queries + self.should_queries + self.must_not_queries + self.filter_queries)

    def required_clauses(self):
        """MUST clauses followed by the FILTER clauses as zero-weight MUST clauses (BooleanWeight puts both into must_weights)."""
        return list(self.must_queries) + [TermQuery(f.term, 0.0) for f in self.filter_queries]

    def extract_terms(self):  # boolean_query.rs:124-145: MUST, SHOULD and FILTER clauses only (a phrase clause: its terms)
        out = []
        for q in list(self.must_queries) + list(self.should_queries) + list(self.filter_queries):
            if isinstance(q, CachedFilter):
                continue   # a set of docs names no term
            out.extend(TermQuery(t, q.boost) for t in q.terms) if isinstance(q, PhraseQuery) else out.append(q)
        return out


class QueryStringQueryBuilder:
    """search/query/query_string.rs:28-250 restated: `+` makes the next clause a MUST clause, `|` and a blank a SHOULD clause,
    parentheses nest, "quoted terms", term^boost, and "a b"~n as one boosted PhraseQuery per field. Over one field a word is that
    field's TermQuery; over several it is a nested should-only BooleanQuery with one TermQuery per field (build_field_query,
    :183-196), boost = the field's boost times the word's. A level with one clause in all is that clause (:167-172). The reference's
    quirks are kept: `boost` is unused, min_should_match is handed to EVERY nested build (:174, :193), the character behind a closing
    quote is swallowed unless it is `^` or `~` (:90-100), a nested parse that fails is dropped silently (:73).
    fields: [(name, boost)]; term(field name, text) -> what TermQuery takes as its term (default: the text's UTF-8 bytes; leaves
    without a term dictionary are queried by term id)."""

    def __init__(self, query_string, fields, min_should_match=0, boost=1.0, term=None):
        self.query_string, self.fields = str(query_string), [(str(f), float(b)) for f, b in fields]
        self.min_should_match, self.boost = int(min_should_match), float(boost)
        self.term = term or (lambda field, text: text.encode("utf-8"))

    def build(self):
        return self._parse(iter(self.query_string), None)

    def _parse(self, chars, end_char):
        musts, shoulds = [], []
        is_option = True

        def push(q):
            (shoulds if is_option else musts).append(q)
        for ch in chars:
            if ch == "+":
                is_option = False
            elif ch == "|":
                is_option = True
            elif ch == "(":
                try:
                    push(self._parse(chars, ")"))
                except RgpuError:
                    pass
            elif ch == '"':
                text = []
                for c in chars:
                    if c == '"':
                        break
                    text.append(c)
                c = next(chars, None)
                if c is not None and c in "^~":
                    text.append(c)
                    for c in chars:
                        if c == " ":
                            break
                        text.append(c)
                if text:
                    push(self._field_query("".join(text)))
                is_option = True
            elif ch == " ":
                is_option = True
            elif ch == ")":
                if end_char != ")":
                    raise RgpuError(-2, "parenthesis not match!")
                break
            else:
                text, done = [ch], False
                for c in chars:
                    if c == " ":
                        break
                    if c == ")":
                        if end_char != ")":
                            raise RgpuError(-2, "parenthesis not match!")
                        done = True
                        break
                    text.append(c)
                push(self._field_query("".join(text)))
                is_option = True
                if done:
                    break
        if len(musts) + len(shoulds) == 1:
            return (musts or shoulds)[0]
        if not musts and not shoulds:
            raise RgpuError(-2, "empty query string!")
        return BooleanQuery.build(musts, shoulds, [], [], self.min_should_match)

    def _field_query(self, text):
        queries = self._phrases(text) if "~" in text else self._terms(text)
        return queries[0] if len(queries) == 1 else BooleanQuery.build([], queries, [], [], self.min_should_match)

    def _terms(self, text):
        boost = np.float32(1.0)
        if "^" in text:
            text, b = text.split("^", 1)
            try:
                boost = np.float32(b)
            except ValueError:
                raise RgpuError(-2, "invalid float literal")
        if text.startswith('"'):
            text = text[1:len(text) - 1]
        return [TermQuery(self.term(f, text), float(np.float32(fb) * boost), field=f) for f, fb in self.fields]

    def _phrases(self, text):
        words, slop = text.split("~", 1)
        try:
            slop = int(slop)
        except ValueError:
            raise RgpuError(-2, "invalid digit found in string")
        words = words.split()
        if len(words) < 2:
            raise RgpuError(-2, "phrase query terms size must not small than 2")
        out = []
        for f, fb in self.fields:
            q = PhraseQuery([self.term(f, w) for w in words], None, fb, slop)
            q.field = f
            out.append(q)
        return out


class DisjunctionMaxQuery:
    """query/disjunction_max_query.rs:43-114: the union of the disjuncts' docs, each scored max + (sum - max) * tie_breaker_multiplier
    over the disjuncts that hold it (DisjunctionMaxScorer, scorer/disjunction_scorer.rs:106-185, 246-286). The GPU path serves
    TermQuery disjuncts (RGPU_OP_DISMAX in include/rucene_gpu.h); any other disjunct is UnsupportedOperation when the query is
    searched, i.e. the caller's CPU path."""

    def __init__(self, disjuncts, tie_breaker_multiplier=0.0):
        self.disjuncts = list(disjuncts)
        self.tie_breaker_multiplier = float(np.float32(tie_breaker_multiplier))
        if not self.disjuncts:   # DisjunctionMaxQuery::build (:51-68)
            raise RgpuError(-2, "DisjunctionMaxQuery: sub query should not be empty!")

    @staticmethod
    def build(disjuncts, tie_breaker_multiplier=0.0):
        """DisjunctionMaxQuery::build: a lone disjunct IS that query."""
        q = DisjunctionMaxQuery(disjuncts, tie_breaker_multiplier)
        return q.disjuncts[0] if len(q.disjuncts) == 1 else q

    def tie_bits(self):
        """The multiplier's f32 bit pattern as the int32 that rgpu_query.n_must_not carries for RGPU_OP_DISMAX."""
        return int(np.float32(self.tie_breaker_multiplier).view(np.int32))

    def extract_terms(self):   # :91-97
        return [t for q in self.disjuncts for t in q.extract_terms()]

    def __str__(self):   # :104-114; the multiplier as Display prints an f32: its shortest round-trip digits, no exponent ("0.1", "1")
        tie = np.float32(self.tie_breaker_multiplier)
        shown = "NaN" if np.isnan(tie) else np.format_float_positional(tie, unique=True, trim="-")
        return "DisjunctionMaxQuery(disjunctions: %s, tie_breaker_multiplier: %s)" % (", ".join(str(q) for q in self.disjuncts), shown)


class BoostingQuery:
    """query/boosting_query.rs:29-118, scorer/boosting_scorer.rs:40-81: the positive query's docs, counts and scores, a doc's score
    multiplied once by negative_boost where the negative query also holds it; a leaf in which the negative query has no scorer
    matches nothing. The GPU path serves (RGPU_NOT_WITH_DEMOTE in include/rucene_gpu.h) a positive that is a TermQuery or a flat
    BooleanQuery packing to TERM / AND / OR (with or without MUST_NOT clauses), a negative that is a TermQuery or a should-only flat
    BooleanQuery with min_should_match <= 1, and 0 < negative_boost < 1 (BoostingScorer::new's debug_assert); anything else is
    UnsupportedOperation when the query is searched, i.e. the caller's CPU path."""

    def __init__(self, positive, negative, negative_boost):
        self.positive, self.negative = positive, negative
        self.negative_boost = float(np.float32(negative_boost))

    @staticmethod
    def build(positive, negative, negative_boost):
        return BoostingQuery(positive, negative, negative_boost)

    def demoting_terms(self):
        """The negative query as a union of TermQuery clauses, or None when it is not of that shape."""
        n = self.negative
        if isinstance(n, TermQuery):
            return [n]
        if (isinstance(n, BooleanQuery) and n.is_flat() and n.should_queries and n.min_should_match <= 1
                and not (n.must_queries or n.must_not_queries or n.filter_queries)):
            return list(n.should_queries)
        return None

    def boost_bits(self):
        """negative_boost's f32 bit pattern (what every demoting clause's `weight` carries)."""
        return int(np.float32(self.negative_boost).view(np.int32))

    def extract_terms(self):   # :62-64
        return self.positive.extract_terms()

    def __str__(self):   # :71-79
        shown = np.format_float_positional(np.float32(self.negative_boost), unique=True, trim="-")
        return "BoostingQuery(positive: %s, negative: %s, negative_boost: %s)" % (self.positive, self.negative, shown)


class TopDocs:
    def __init__(self, total_hits, score_docs):
        self._total, self._docs = int(total_hits), score_docs

    def total_hits(self):
        return self._total

    def score_docs(self):
        """[(doc, score)] best first: score desc, then doc asc (the canonical tie rule)."""
        return self._docs


class TopDocsCollector:
    def __init__(self, estimated_hits):
        self.estimated_hits = int(estimated_hits)
        self._result = TopDocs(0, [])

    def needs_scores(self):
        return True

    def top_docs(self):
        return self._result


class GpuIndexSearcher:
    """IndexSearcher over GPU-resident leaves. `search(query, collector)` mirrors searcher.rs:487-525;
    `search_batch` is the batched form the hardware wants (one launch set per leaf for many queries)."""

    range_filter_capacity = 256   # memoised range filters kept from one search_batch to the next (range_filter); set per searcher

    def __init__(self, leaves, ctx=None, similarity=None, next_limit=None, flatten_nested=False, cpu_fallback=None, filtered_phrases=False,
                 required_sets=False, unordered_spans=False, optional_phrases=False, field_trees=False):
        """field_trees: serve the trees QueryStringQueryBuilder builds over several fields - every word a nested should-only
        BooleanQuery with one TermQuery per field, those groups under MUST and SHOULD by the `+` sign ("gpu +search") - through
        rgpu_search_fields_tree_batch (ReqOptScorer's sequential rule kept; off by default: such rows are UnsupportedOperation, as
        they have been). Rows rgpu_search_fields_batch can express keep going there. Still refused with it on: a nested clause that
        is not a should-only BooleanQuery of TermQuery clauses, a nested min_should_match >= 2, phrases, FILTER clauses, ten or more
        groups on a side, k > 128.
        What it costs: with the flag on EVERY `+a b` query string takes the rule's path, where ONE wavefront walks the query's hits in
        doc order - about 7 ns per posting of the cheapest MUST group, so a `+word` that millions of docs hold costs tens of
        milliseconds by itself and a batch of 1024 such trees over 10 M docs took 1.3 s against 24 ms without the rule (DESIGN.md
        section 4.6). A context opened with req_opt_rule=-1 adds the optional sums everywhere instead, in one pass: same docs and
        counts, scores >= the reference's. `a b` trees (no `+`) never take that path.
        optional_phrases: serve MUST / FILTER + SHOULD trees with exact phrases on either side - +a +b "a b" (the phrase boost),
        +"a b" c, +"a b" +c "b c" d -n #f - through rgpu_search_phrase_opt_batch (ReqOptScorer over the phrase scorers, its
        sequential rule kept; off by default: such rows are UnsupportedOperation, as they have been). Still refused with it on:
        whatever phrase_opt_parts refuses (nested clauses beside a phrase, a phrase under MUST_NOT, sloppy clauses, ten or more
        optional clauses, more than 4 phrases on a side) and such a row beside doc-set clauses (the call has no masked form).
        unordered_spans: serve a top-level SpanNearQuery(in_order=False) over SpanTermQuery clauses through
        rgpu_search_span_unordered_batch (NearSpansUnordered, the heap's array order kept; off by default: such rows are
        UnsupportedOperation, as they have been). Still refused with it on: nested span clauses, a span query inside a boolean,
        filtered, dismax, boosting or rescoring query.
        required_sets: serve queries whose ONLY required clauses are doc sets - "b c #F", a lone #F, a lone PointRangeQuery,
        "+range b c", "-X", "-t", MatchAllDocsQuery alone and under MUST - through rgpu_search_batch_required_set: every doc of
        live AND sets is collected, the docs no SHOULD clause holds at score 0 (off by default: such rows are UnsupportedOperation,
        as they have been). With it on "b c -X" (min_should_match <= 1) is served too, masked: ReqNotScorer over the disjunction,
        which has a scorer of its own. Still refused: an exclusion beside min_should_match >= 2, and on the SHOULD side of such a
        row phrases, nested clauses and a clause of boost <= 0.
        filtered_phrases: serve EXACT phrases beside doc-set clauses - FilterQuery("a b", F), +"a b" #F -X, +"a b" +c #F -X,
        "a b" c -X with min_should_match <= 1, point ranges in those positions - through rgpu_search_phrase_batch_masked,
        _phrase_bool_batch_masked and _phrase_or_batch_masked (off by default: such rows are UnsupportedOperation, as they have been).
        Still refused with it on: any sloppy phrase under a mask, "a b" c #F (the doc set is the only required clause), -X beside
        min_should_match >= 2, and whatever phrase_bool_parts / phrase_or_parts refuse.
        flatten_nested: fold one level of nested BooleanQuery clauses (BooleanQuery.flattened: same docs and counts, scores
        within 1e-5 of the reference's — off by default because it is not bit-exact). cpu_fallback(query, collector): what
        SURVEY 8(f)1 calls "everything else to the CPU path" — search() hands every tree the GPU path does not serve
        (UnsupportedOperation) to it, as the Rust shim hands them to DefaultIndexSearcher (rust/gpu/searcher.rs); None: raise."""
        self.flatten_nested = bool(flatten_nested)
        self.filtered_phrases = bool(filtered_phrases)
        self.required_sets = bool(required_sets)
        self.unordered_spans = bool(unordered_spans)
        self.optional_phrases = bool(optional_phrases)
        self.field_trees = bool(field_trees)
        self.cpu_fallback = cpu_fallback
        self.leaves = list(leaves)
        # DefaultIndexSearcher::new(reader, next_limit: Option<usize>) (searcher.rs:291-296, :361): how many approximations of a
        # two-phase scorer (here: sloppy phrases) may go by on a leaf without a collected doc. None = the default, 500 000
        if next_limit is not None and int(next_limit) < 0:
            raise RgpuError(-2, "next_limit must be >= 0 (None: the reference's default of 500 000)")
        # (the C ABI spells Some(0) RGPU_NEXT_LIMIT_ZERO = -2: a zero there keeps meaning "the default")
        self.next_limit = 0 if next_limit is None else (-2 if int(next_limit) == 0 else int(next_limit))
        self.ctx = ctx or _lib.Context()
        self.similarity = similarity or BM25Similarity()
        for leaf in self.leaves:
            if leaf.segment is None:
                leaf.segment = _lib.Segment(self.ctx, leaf.doc_bytes, leaf.norms, leaf.max_doc, leaf.doc_base, leaf.live_docs,
                                            leaf.index_options | (_lib.FIELD_STORES_PAYLOADS if getattr(leaf, "has_payloads", False) else 0))
                if getattr(leaf, "pay_bytes", None) is not None:
                    leaf.segment.attach_payloads(leaf.pay_bytes)   # Lucene50PostingsReader::open checks the third file too
            for xf in getattr(leaf, "extra_fields", {}).values():   # the segment's further fields: slots 1.. in the order given
                if xf.slot is None:
                    xf.slot = leaf.segment.attach_field(xf.norms, xf.index_options | (_lib.FIELD_STORES_PAYLOADS if xf.has_payloads else 0))
        # searcher.rs:306-363: statistics of the first leaf with the largest max_doc stand in for the index
        self._stats_leaf = 0
        for i, leaf in enumerate(self.leaves):
            if leaf.max_doc > self.leaves[self._stats_leaf].max_doc:
                self._stats_leaf = i
        sl = self.leaves[self._stats_leaf]
        self.collection_statistics = CollectionStatistics(sl.field, sl.doc_base, self.max_doc(), sl.doc_count,
                                                          sl.sum_total_term_freq, sl.sum_doc_freq)
        self._weights = {}
        self._field_weights = {}  # (field name, term, boost) -> (weight, sim table): a further field's own statistics
        self._planners = {}       # per leaf: the native batch planner
        self._stats_terms = None  # override_statistics: another leaf's term table / dictionary
        self._masks = {}          # (filter sets, exclude sets) key -> (the CachedFilters, one combined DocSet per leaf)
        self._points = {}         # field -> (bytes per value, one _lib.Points per leaf or None)
        self._range_filters = {}  # (field, lower, upper) -> CachedFilter, least recently used first
        self._every_doc = None    # required_sets: MatchAllDocsQuery as a CachedFilter (rgpu_docset_combine of nothing, once per leaf)
        self._not_filters = {}    # required_sets: MUST_NOT term clauses as an excluded CachedFilter, by clause tuple; least recently used first

    def max_doc(self):
        return sum(leaf.max_doc for leaf in self.leaves)

    def term_statistics(self, term_id):
        """searcher.rs:732-767: df of the term in the statistics leaf only (0 when absent there)."""
        stats = getattr(self, "_stats_terms", None)
        if stats is None:
            st = self.leaves[self._stats_leaf].term_state(term_id)
            return 0 if st is None else int(st["doc_freq"])
        if isinstance(stats, _lib.TermDictionary):
            states, found = stats.lookup(self.leaves[self._stats_leaf].field_number, [term_id])
            return int(states[0]["doc_freq"]) if found[0] else 0
        return int(stats[term_id]["doc_freq"]) if 0 <= term_id < len(stats) else 0

    def _weight(self, term_id, boost):
        key = (term_id, boost)
        if key not in self._weights and len(self._weights) >= (1 << 20):
            self._weights.clear()
        if key not in self._weights:
            w, cache = self.similarity.compute_weight(self.collection_statistics, [self.term_statistics(term_id)], boost)
            self._weights[key] = (w, self.ctx.sim_table(cache, self.similarity.k1))
        return self._weights[key]

    # ---- cross-field queries (rgpu_search_fields_batch) ---------------------------------------------------------------------------
    def _primary(self, tq):
        return tq.field is None or tq.field == self.leaves[0].field

    def _names_other_field(self, query):
        """Does some TermQuery of the tree name a field other than the leaves' primary one?"""
        if isinstance(query, TermQuery):
            return not self._primary(query)
        if isinstance(query, PhraseQuery):   # (QueryStringQueryBuilder's phrases carry their field; no cross-field call takes one)
            return getattr(query, "field", None) is not None and query.field != self.leaves[0].field
        if isinstance(query, DisjunctionMaxQuery):
            return any(self._names_other_field(q) for q in query.disjuncts)
        if isinstance(query, BooleanQuery):
            return any(self._names_other_field(q) for q in list(query.must_queries) + list(query.should_queries) + list(query.must_not_queries) +
                       list(query.filter_queries) if not isinstance(q, CachedFilter))
        if isinstance(query, BoostingQuery):
            return self._names_other_field(query.positive) or self._names_other_field(query.negative)
        if isinstance(query, FilterQuery):
            return self._names_other_field(query.query)
        return False

    def _refuse_other_fields(self, query):
        """Only search_batch / search route a tree that names a further field (to rgpu_search_fields_batch). Every other path -
        count, count_batch, rescore_batch, cache_filter, the packers - reads the primary field alone and hands such a tree to the
        caller's CPU path instead of answering for the wrong field."""
        if self._names_other_field(query):
            raise RgpuError(-5, "a query that names a further field is served by search_batch / search only")

    def _field_weight(self, tq):
        """(weight, sim table) of a clause from ITS field's statistics: idf from the term's doc_freq in that field of the statistics
        leaf, the norm cache from that field's doc_count and sum_total_term_freq there (searcher.rs:306-363, 732-767)"""
        if self._primary(tq):
            return self._weight(tq.term, tq.boost)
        key = (tq.field, tq.term, tq.boost)
        if key not in self._field_weights:
            if len(self._field_weights) >= (1 << 20):
                self._field_weights.clear()
            sl = self.leaves[self._stats_leaf]
            if tq.field not in sl.extra_fields:
                raise RgpuError(-2, "no field %r among the leaves' extra_fields" % tq.field)
            xf = sl.extra_fields[tq.field]
            st = xf.term_state(tq.term)
            stats = CollectionStatistics(tq.field, sl.doc_base, self.max_doc(), xf.doc_count, xf.sum_total_term_freq, xf.sum_doc_freq)
            w, cache = self.similarity.compute_weight(stats, [0 if st is None else int(st["doc_freq"])], tq.boost)
            self._field_weights[key] = (w, self.ctx.sim_table(cache, self.similarity.k1))
        return self._field_weights[key]

    def _cross_spec(self, query):
        """A flat tree over TermQuery / DisjunctionMaxQuery-of-TermQuery clauses -> (occur, [(kind, tie bits, [TermQuery])], msm,
        [MUST_NOT TermQuery]); anything rgpu_search_fields_batch cannot express is UnsupportedOperation (the caller's CPU path)"""
        def group(q):
            if isinstance(q, TermQuery):
                return (_lib.GROUP_TERM, 0, [q])
            if isinstance(q, DisjunctionMaxQuery) and all(isinstance(d, TermQuery) for d in q.disjuncts):
                if not np.isfinite(np.float32(q.tie_breaker_multiplier)):
                    raise RgpuError(-2, "tie_breaker_multiplier is not finite")
                if len(q.disjuncts) > _lib.MAX_GROUP_DISJUNCTS:
                    raise RgpuError(-5, "ten or more disjuncts are summed in heap order by the reference")
                return (_lib.GROUP_DISMAX, int(np.float32(q.tie_breaker_multiplier).view(np.uint32)), list(q.disjuncts))
            raise RgpuError(-5, "a cross-field query is served over TermQuery and DisjunctionMaxQuery-of-TermQuery clauses")
        def known(spec):
            for tq in [t for g in spec[1] for t in g[2]] + spec[3]:
                if not self._primary(tq) and any(tq.field not in leaf.extra_fields for leaf in self.leaves):
                    raise RgpuError(-2, "no field %r among the leaves' extra_fields" % tq.field)
            return spec
        if isinstance(query, (TermQuery, DisjunctionMaxQuery)):
            return known((_lib.OCCUR_SHOULD, [group(query)], 0, []))
        if not isinstance(query, BooleanQuery):
            raise RgpuError(-5, "query type not served across fields by the GPU path: %r" % (query,))
        if query.filter_queries:
            raise RgpuError(-5, "FILTER clauses are not served across fields by the GPU path")
        if getattr(self, "field_trees", False) and ((query.must_queries and query.should_queries) or
                                                    any(isinstance(q, BooleanQuery) for q in list(query.must_queries) + list(query.should_queries))):
            return self._tree_spec(query, group)
        if query.must_queries and query.should_queries:
            raise RgpuError(-5, "MUST and SHOULD clauses in one cross-field query (ReqOptScorer) are not served by the GPU path")
        if not all(isinstance(q, TermQuery) for q in query.must_not_queries):
            raise RgpuError(-5, "a cross-field query's MUST_NOT clauses are TermQuerys")
        positive = list(query.must_queries) or list(query.should_queries)
        if not positive:
            raise RgpuError(-5, "a query of MUST_NOT clauses alone is not served across fields by the GPU path")
        if len(positive) > _lib.MAX_FIELD_GROUPS:
            raise RgpuError(-5, "ten or more clauses are summed in heap order by the reference")
        occur = _lib.OCCUR_MUST if query.must_queries else _lib.OCCUR_SHOULD
        msm = 0 if query.must_queries else int(query.min_should_match)
        if occur == _lib.OCCUR_SHOULD and msm >= 2 and query.must_not_queries:
            raise RgpuError(-5, "MUST_NOT clauses beside min_should_match >= 2 are not served across fields by the GPU path")
        groups = [group(q) for q in positive]
        if sum(len(g[2]) for g in groups) + len(query.must_not_queries) > _lib.MAX_FIELDS_QUERY_CLAUSES:
            raise RgpuError(-5, "too many clauses in one cross-field query")
        return known((occur, groups, msm, list(query.must_not_queries)))

    def _tree_spec(self, query, flat_group):
        """field_trees: a BooleanQuery with nested should-only BooleanQuery-of-TermQuery clauses and / or MUST beside SHOULD clauses ->
        ("tree", [MUST groups], [SHOULD groups], msm, [MUST_NOT TermQuery]), a group (kind, tie bits, [TermQuery], nested msm); what
        rgpu_search_fields_tree_batch cannot express is UnsupportedOperation"""
        def group(q):
            if not isinstance(q, BooleanQuery):
                return flat_group(q) + (0,)
            if (q.must_queries or q.must_not_queries or q.filter_queries or not q.should_queries
                    or not all(isinstance(t, TermQuery) for t in q.should_queries)):
                raise RgpuError(-5, "a nested clause of a cross-field tree is a should-only BooleanQuery of TermQuery clauses")
            if q.min_should_match >= 2:
                raise RgpuError(-5, "a nested min_should_match >= 2 is not served across fields by the GPU path")
            if len(q.should_queries) > _lib.MAX_GROUP_DISJUNCTS:
                raise RgpuError(-5, "ten or more disjuncts are summed in heap order by the reference")
            return (_lib.GROUP_SUM, 0, list(q.should_queries), int(q.min_should_match))
        if not all(isinstance(q, TermQuery) for q in query.must_not_queries):
            raise RgpuError(-5, "a cross-field query's MUST_NOT clauses are TermQuerys")
        if len(query.must_queries) > _lib.MAX_FIELD_GROUPS or len(query.should_queries) > _lib.MAX_FIELD_GROUPS:
            raise RgpuError(-5, "ten or more clauses on a side are summed in heap order by the reference")
        msm = int(query.min_should_match)
        if not query.must_queries and msm >= 2 and query.must_not_queries:
            raise RgpuError(-5, "MUST_NOT clauses beside min_should_match >= 2 are not served across fields by the GPU path")
        musts, shoulds = [group(q) for q in query.must_queries], [group(q) for q in query.should_queries]
        if sum(len(g[2]) for g in musts + shoulds) + len(query.must_not_queries) > _lib.MAX_FIELDS_QUERY_CLAUSES:
            raise RgpuError(-5, "too many clauses in one cross-field query")
        for tq in [t for g in musts + shoulds for t in g[2]] + list(query.must_not_queries):
            if not self._primary(tq) and any(tq.field not in leaf.extra_fields for leaf in self.leaves):
                raise RgpuError(-2, "no field %r among the leaves' extra_fields" % tq.field)
        return ("tree", musts, shoulds, msm, list(query.must_not_queries))

    def pack_fields_tree(self, specs, leaf):
        """_tree_spec rows -> (rgpu_fields_tree_query[], rgpu_field_tree_group[], rgpu_field_clause[]) for one leaf"""
        Q, G, C = [], [], []

        def clause(tq, scored=True):
            row = np.zeros(1, _lib.FIELD_CLAUSE_DTYPE)[0]
            xf = None if self._primary(tq) else leaf.extra_fields[tq.field]
            st = leaf.term_state(tq.term) if xf is None else xf.term_state(tq.term)
            if st is not None:
                row["state"] = st
            if scored:
                row["weight"], row["sim_table"] = self._field_weight(tq)
            row["field"] = 0 if xf is None else xf.slot
            C.append(row)
        for _, musts, shoulds, msm, nots in specs:
            g0 = len(G)
            for kind, tie_bits, tqs, gmsm in musts + shoulds:
                c0 = len(C)
                for tq in tqs:
                    clause(tq)
                G.append((c0, len(tqs), tie_bits, kind, gmsm, 0))
            n0 = len(C)
            for tq in nots:
                clause(tq, scored=False)
            Q.append((g0, len(musts), len(shoulds), msm, n0, len(nots)))
        return np.array(Q, _lib.FIELDS_TREE_QUERY_DTYPE), np.array(G, _lib.FIELD_TREE_GROUP_DTYPE), np.array(C, _lib.FIELD_CLAUSE_DTYPE)

    def pack_fields(self, specs, leaf):
        """_cross_spec rows -> (rgpu_fields_query[], rgpu_field_group[], rgpu_field_clause[]) for one leaf"""
        Q, G, C = [], [], []

        def clause(tq, scored=True):
            row = np.zeros(1, _lib.FIELD_CLAUSE_DTYPE)[0]
            xf = None if self._primary(tq) else leaf.extra_fields[tq.field]
            st = leaf.term_state(tq.term) if xf is None else xf.term_state(tq.term)
            if st is not None:
                row["state"] = st
            if scored:
                row["weight"], row["sim_table"] = self._field_weight(tq)
            row["field"] = 0 if xf is None else xf.slot
            C.append(row)
        for occur, groups, msm, nots in specs:
            g0 = len(G)
            for kind, tie_bits, tqs in groups:
                c0 = len(C)
                for tq in tqs:
                    clause(tq)
                G.append((c0, len(tqs), tie_bits, kind))
            n0 = len(C)
            for tq in nots:
                clause(tq, scored=False)
            Q.append((occur, g0, len(G) - g0, msm, n0, len(nots)))
        return np.array(Q, _lib.FIELDS_QUERY_DTYPE), np.array(G, _lib.FIELD_GROUP_DTYPE), np.array(C, _lib.FIELD_CLAUSE_DTYPE)

    def _cross_rows(self, specs, k):
        """(hits, totals) of _cross_spec rows (rows that name a further field), merged over the leaves"""
        if k > 128:
            raise RgpuError(-5, "a cross-field query is served for k <= 128")
        trees = [i for i, s in enumerate(specs) if s[0] == "tree"]   # field_trees: the rows rgpu_search_fields_batch cannot express
        if trees:
            flat = [i for i in range(len(specs)) if specs[i][0] != "tree"]
            hits, totals = np.zeros((len(specs), k), dtype=_lib.HIT_DTYPE), np.zeros(len(specs), dtype=np.int64)
            if flat:
                hits[flat], totals[flat] = self._cross_rows([specs[i] for i in flat], k)
            tree_specs = [specs[i] for i in trees]
            per_leaf = [leaf.segment.search_fields_tree_batch(*self.pack_fields_tree(tree_specs, leaf), k) for leaf in self.leaves]
            hits[trees], totals[trees] = per_leaf[0] if len(per_leaf) == 1 else self._merge_leaves(per_leaf, len(tree_specs), k)
            return hits, totals
        per_leaf = [leaf.segment.search_fields_batch(*self.pack_fields(specs, leaf), k) for leaf in self.leaves]
        return per_leaf[0] if len(per_leaf) == 1 else self._merge_leaves(per_leaf, len(specs), k)

    def _flatten(self, query):
        """-> (op, required / scored clauses, optional SHOULD clauses beside MUST ones, MUST_NOT clauses — a BoostingQuery's demoting
        clauses behind them: _boosting_fields)"""
        self._refuse_other_fields(query)
        if isinstance(query, TermQuery):
            return OP_TERM, [query], [], []
        if isinstance(query, PointRangeQuery) or (isinstance(query, BooleanQuery) and any(
                isinstance(q, PointRangeQuery) for q in list(query.must_queries) + list(query.filter_queries) + list(query.must_not_queries))):
            raise RgpuError(-5, "a point range clause is served as a doc set (search_batch peels it off): it packs to no clause")
        if isinstance(query, BoostingQuery):
            demoting = query.demoting_terms()
            if demoting is None:
                raise RgpuError(-5, "a BoostingQuery is served by the GPU path when its negative query is a term or a flat disjunction of terms")
            if not 0.0 < query.negative_boost < 1.0:   # (NaN fails both comparisons)
                raise RgpuError(-5, "a BoostingQuery is served by the GPU path for 0 < negative_boost < 1")
            if not isinstance(query.positive, (TermQuery, BooleanQuery)):
                raise RgpuError(-5, "a BoostingQuery is served by the GPU path when its positive query is a term or a flat boolean query")
            positive = query.positive.normalized() if isinstance(query.positive, BooleanQuery) else query.positive
            if isinstance(positive, BooleanQuery) and not positive.is_flat():
                raise RgpuError(-5, "a BoostingQuery over nested boolean clauses is not served by the GPU path")
            op, clauses, opts, nots = self._flatten(positive)
            if opts or (op & ~0xffff):
                raise RgpuError(-5, "a BoostingQuery over MUST + SHOULD clauses is not served by the GPU path")
            return op, clauses, [], list(nots) + demoting
        if isinstance(query, DisjunctionMaxQuery):
            if not all(isinstance(q, TermQuery) for q in query.disjuncts):
                raise RgpuError(-5, "a DisjunctionMaxQuery is served by the GPU path when every disjunct is a TermQuery")
            return OP_DISMAX, list(query.disjuncts), [], []   # (the tie-breaker rides in n_must_not: _dismax_fields)
        if isinstance(query, BooleanQuery):
            if any(isinstance(q, DisjunctionMaxQuery) for q in list(query.must_queries) + list(query.should_queries) + list(query.must_not_queries) +
                   list(query.filter_queries)):
                raise RgpuError(-5, "a DisjunctionMaxQuery clause inside a BooleanQuery is served across fields only (TermQuery(field=...))")
            query = query.normalized()
            if not query.is_flat():
                first = query.nested_disjunction_first()
                if first is not None:
                    return self._flatten(first)
                # "+a +(b c)" / "+a +(+b +c)": ONE nested should-only / must-only query among the MUST clauses. The library sorts the
                # conjunction's children by cost per leaf as ConjunctionScorer::new does and adds the nested sum where the reference
                # adds it (RGPU_OP_NESTED_AT breaks ties like the stable sort): the reference's f32 sums, whatever the costs.
                for nested, flag in ((query.required_disjunction(), OP_SHOULD_REQUIRED), (query.nested_conjunction(), OP_NESTED_MUST)):
                    if nested is None:
                        continue
                    at = [q is nested for q in query.must_queries].index(True)
                    musts = [q for q in query.must_queries if q is not nested]
                    if not (musts or query.filter_queries):
                        # (a lone nested MUST clause: BooleanQuery::build has already rewritten such a tree to the clause itself)
                        raise RgpuError(-5, "a nested query with no clause beside it is that query")
                    inner = list(nested.should_queries if flag == OP_SHOULD_REQUIRED else nested.must_queries)
                    required = musts + [TermQuery(f.term, 0.0) for f in query.filter_queries]
                    return _i32(OP_AND | (len(inner) << 16) | flag | (at << 26)), required, inner, query.must_not_queries
                folded = query.flattened() if getattr(self, "flatten_nested", False) else None
                if folded is None:
                    raise RgpuError(-5, "nested boolean clauses are not served by the GPU path (flatten_nested folds one level of MUST-of-MUSTs / SHOULD-of-SHOULDs)")
                query = folded
            required = query.required_clauses()
            if required:
                opts = query.should_queries
                return OP_AND | (len(opts) << 16), required, opts, query.must_not_queries   # RGPU_OP_WITH_SHOULD
            msm = query.min_should_match
            return (OP_OR | (msm << 8) if msm > 1 else OP_OR), query.should_queries, [], query.must_not_queries
        raise RgpuError(-5, "query type not served by the GPU path: %r" % (query,))

    def override_statistics(self, collection_statistics, stats_terms=None):
        """Score with the statistics of a leaf that lives elsewhere (segment-sharded search: every shard takes them from
        shard 0, the index-wide first largest leaf — SURVEY.md §8(e)): `stats_terms` = that leaf's flat term table
        (TERM_STATE_DTYPE, indexed by term id) or its TermDictionary; None keeps this searcher's own statistics leaf."""
        self.collection_statistics = collection_statistics
        self._stats_terms = stats_terms
        self._weights, self._planners = {}, {}

    def _planner(self, leaf):
        """The native batch planner (rgpu_planner, csrc/host/batch_planner.hpp) of one leaf: term resolution in the leaf
        and in the statistics leaf, BM25 weights, one sim table."""
        key = id(leaf)
        p = self._planners.get(key)
        if p is None:
            cs = self.collection_statistics
            stats = self._stats_terms
            if stats is None:
                sl = self.leaves[self._stats_leaf]
                stats = sl.term_dictionary if sl.term_dictionary is not None else sl.terms
            mine = leaf.term_dictionary if leaf.term_dictionary is not None else leaf.terms
            if isinstance(mine, _lib.TermDictionary) != isinstance(stats, _lib.TermDictionary):
                raise RgpuError(-2, "the searched leaf and the statistics leaf must name terms the same way (bytes or ids)")
            _w, cache = self.similarity.compute_weight(cs, [1], 1.0)   # the norm cache depends on the collection alone
            table = self.ctx.sim_table(cache, self.similarity.k1)
            p = _lib.Planner(None, cs.max_doc, cs.doc_count, cs.sum_total_term_freq, mine, None if stats is mine else stats,
                             self.similarity.k1, self.similarity.b, leaf.field_number, sim_table=table)
            self._planners[key] = p
        return p

    def pack_uniform(self, op, term_ids, leaf, min_should_match=0):
        """The planner for a batch handed over as an ARRAY: `term_ids[q, c]` = flat-table id of clause c of query q, every
        query the same shape — `op` OP_TERM (one column), OP_AND (all MUST) or OP_OR (all SHOULD, optionally with
        min_should_match), boost 1. Equals pack([TermQuery / BooleanQuery.build(...) ...]) on the same ids; the whole of it
        runs behind the C ABI (rgpu_plan_uniform_ids)."""
        term_ids = np.asarray(term_ids, dtype=np.int64)
        if term_ids.ndim == 1:
            term_ids = term_ids.reshape(-1, 1)
        nq, nc = term_ids.shape
        if op not in (OP_TERM, OP_AND, OP_OR) or (op == OP_TERM and nc != 1) or nc < 1:
            raise RgpuError(-1, "pack_uniform: op TERM takes one column, AND / OR at least one")
        if nc > _lib.MAX_QUERY_TERMS:
            raise RgpuError(-5, "more than %d clauses" % _lib.MAX_QUERY_TERMS)
        if nc == 1:
            op, min_should_match = OP_TERM, 0   # BooleanQuery::build with a single clause rewrites to that clause (boolean_query.rs:56-68)
        return self._planner(leaf).plan_uniform((op | (min_should_match << 8)) if (op == OP_OR and min_should_match > 1) else op, term_ids)

    def search_uniform_device(self, op, term_ids, leaf, k, hits_ptr, totals_ptr, stream=0, min_should_match=0, comm=None):
        """pack_uniform + rgpu_search_batch_device (comm: rgpu_search_batch_sharded) as ONE call behind the C ABI
        (rgpu_planner_search_uniform_ids_device): the serving path of a batch named by term ids. Enqueue-only; same rows as
        the two calls."""
        term_ids = np.asarray(term_ids, dtype=np.int64)
        if term_ids.ndim == 1:
            term_ids = term_ids.reshape(-1, 1)
        nc = term_ids.shape[1]
        if op not in (OP_TERM, OP_AND, OP_OR) or (op == OP_TERM and nc != 1) or nc < 1:
            raise RgpuError(-1, "search_uniform_device: op TERM takes one column, AND / OR at least one")
        if nc > _lib.MAX_QUERY_TERMS:
            raise RgpuError(-5, "more than %d clauses" % _lib.MAX_QUERY_TERMS)
        if nc == 1:
            op, min_should_match = OP_TERM, 0
        full_op = (op | (min_should_match << 8)) if (op == OP_OR and min_should_match > 1) else op
        self._planner(leaf).search_uniform_device(leaf.segment, full_op, term_ids, k, hits_ptr, totals_ptr, stream, comm=comm)

    def pack(self, queries, leaf):
        """queries -> (rgpu_query[], rgpu_query_term[]) for one leaf."""
        flat = [self._flatten(q) for q in queries]
        clauses = [c for _, t, o, n in flat for group in (t, o, n) for c in group]
        by_id = [type(c.term) is int for c in clauses]
        if clauses and (all(by_id) or not any(by_id)) and all(by_id) == (leaf.term_dictionary is None):
            # one naming scheme throughout (the usual case): the per-clause work — resolution, weights — happens natively
            if max(len(t) + len(o) + len(n) for _, t, o, n in flat) > _lib.MAX_QUERY_TERMS:
                raise RgpuError(-5, "more than %d clauses" % _lib.MAX_QUERY_TERMS)
            boosts = None if all(c.boost == 1.0 for c in clauses) else [c.boost for c in clauses]
            # (the planner resolves and weighs a dismax query's clauses as an OR query's; its op and tie-breaker are written afterwards)
            qs, ts = self._planner(leaf).plan_batch([OP_OR if f[0] == OP_DISMAX else f[0] for f in flat], [len(f[1]) for f in flat],
                                                    [c.term for c in clauses], [len(f[3]) for f in flat], boosts)
            return self._boosting_fields(queries, self._dismax_fields(queries, qs), ts)
        return self._pack_clause_by_clause(queries, leaf, flat)

    @staticmethod
    def _dismax_fields(queries, qs):
        """RGPU_OP_DISMAX: op 3 whatever the clause count, n_must_not = the bits of the f32 tie_breaker_multiplier."""
        for i, q in enumerate(queries):
            if isinstance(q, DisjunctionMaxQuery):
                qs[i]["op"], qs[i]["n_must_not"] = OP_DISMAX, q.tie_bits()
        return qs

    @staticmethod
    def _boosting_fields(queries, qs, ts):
        """RGPU_NOT_WITH_DEMOTE: the last n_demote of the clauses planned as MUST_NOT are the demoting ones — the count moves to the
        field's second byte, their weight is negative_boost, their table is never read."""
        for i, q in enumerate(queries):
            if isinstance(q, BoostingQuery):
                n_dem = len(q.demoting_terms())
                n_not = int(qs[i]["n_must_not"]) - n_dem
                qs[i]["n_must_not"] = n_not | (n_dem << 8)
                at = int(qs[i]["first_term"]) + int(qs[i]["n_terms"]) + n_not
                ts["weight"][at:at + n_dem] = np.float32(q.negative_boost)
                ts["sim_table"][at:at + n_dem] = 0
        return qs, ts

    def _pack_clause_by_clause(self, queries, leaf, flat=None):
        """pack() one clause at a time in Python: mixed naming schemes, numpy-scalar ids; also what tests hold the native
        planner against."""
        flat = flat or [self._flatten(q) for q in queries]
        byte_terms = [c.term for _, t, o, n in flat for c in list(t) + list(o) + list(n) if isinstance(c.term, bytes)]
        if byte_terms:
            leaf.resolve(byte_terms)
            self.leaves[self._stats_leaf].resolve(byte_terms)
        n_terms = sum(len(t) + len(o) + len(n) for _, t, o, n in flat)
        qs = np.zeros(len(flat), dtype=QUERY_DTYPE)
        ts = np.zeros(max(n_terms, 1), dtype=QUERY_TERM_DTYPE)
        pos = 0
        for i, (op, clauses, opts, nots) in enumerate(flat):
            if len(clauses) + len(opts) + len(nots) > _lib.MAX_QUERY_TERMS:
                raise RgpuError(-5, "more than %d clauses" % _lib.MAX_QUERY_TERMS)
            qs[i] = (op, len(clauses), pos, len(nots))   # clause order: MUST / scored, optional SHOULD, MUST_NOT
            for c in list(clauses) + list(opts) + list(nots):
                w, table = self._weight(c.term, c.boost)
                st = leaf.term_state(c.term)
                if st is not None:
                    ts[pos]["state"] = st
                else:
                    ts[pos]["state"]["doc_freq"] = 0
                    ts[pos]["state"]["skip_offset"] = -1
                    ts[pos]["state"]["singleton_doc_id"] = -1
                ts[pos]["weight"] = w
                ts[pos]["sim_table"] = table
                pos += 1
        return self._boosting_fields(queries, self._dismax_fields(queries, qs), ts)

    def search_phrase_batch(self, queries, k):
        """IndexSearcher::search(PhraseQuery, TopDocsCollector(k)) for a batch of exact phrases -> (hits, total_hits).
        PhraseQuery::create_weight (phrase_query.rs:136-186): one BM25 weight from the statistics of ALL the phrase's terms."""
        per_leaf = []
        for leaf in self.leaves:
            qs, ts = self.pack_phrases(queries, leaf)
            per_leaf.append(leaf.segment.search_phrase_batch(qs, ts, k))
        if len(per_leaf) == 1:
            return per_leaf[0]
        return self._merge_leaves(per_leaf, len(queries), k)

    def pack_phrases(self, queries, leaf):
        """PhraseQuery objects -> the rgpu_phrase_query[] / rgpu_phrase_term[] of rgpu_search_phrase_batch for one leaf (attaches the
        leaf's .pos file on first use)."""
        if leaf.pos_bytes is None:
            raise RgpuError(-1, "phrase search needs a positions field (LeafReader.pos_bytes)")
        if not getattr(leaf, "_pos_attached", False):
            leaf.segment.attach_positions(leaf.pos_bytes)
            leaf._pos_attached = True
        qs = np.zeros(len(queries), dtype=_lib.PHRASE_QUERY_DTYPE)
        ts = np.zeros(sum(len(q.terms) for q in queries), dtype=_lib.PHRASE_TERM_DTYPE)
        at = 0
        for i, q in enumerate(queries):
            w, cache = self.similarity.compute_weight(self.collection_statistics, [self.term_statistics(t) for t in q.terms], q.boost)
            qs[i] = (len(q.terms), at, w, self.ctx.sim_table(cache, self.similarity.k1), q.slop, self.next_limit)
            for t, p in zip(q.terms, q.positions):
                sp = leaf.positions_state(t)
                if sp is not None:
                    ts[at]["state"], ts[at]["positions"] = sp
                else:
                    ts[at]["state"]["doc_freq"] = 0
                ts[at]["position"] = p
                at += 1
        return qs, ts

    def rescore_batch(self, hits, rescore_queries, query_weight=1.0, rescore_weight=1.0, mode=_lib.RESCORE_TOTAL, window_size=None):
        """QueryRescorer::rescore (search/scorer/rescorer.rs:376-390) for a batch: row i of `hits` (a first pass's output) is
        re-ranked by rescore_queries[i] — a TermQuery, an all-MUST / all-SHOULD BooleanQuery, or a PhraseQuery (exact, or sloppy
        without a repeated term; k up to 128 when the batch holds other kinds than phrases). A batch may mix the kinds: the
        phrase rows go through rgpu_rescore_phrase_batch, the others through rgpu_rescore_batch, and a row's result does not
        depend on the other rows. One call per kind and leaf, the last leaf's sorts the windows and re-weights the tails."""
        k = hits.shape[1]
        req = np.zeros(len(rescore_queries), dtype=_lib.RESCORE_REQUEST_DTYPE)
        req["query_weight"], req["rescore_weight"], req["mode"] = query_weight, rescore_weight, mode
        req["window_size"] = k if window_size is None else window_size
        is_phrase = np.array([isinstance(q, PhraseQuery) for q in rescore_queries], dtype=bool)
        if any(_holds_span(q) for q in rescore_queries):
            raise RgpuError(-5, "rescoring with a span query is not served by the GPU path")
        for q in rescore_queries:   # refused before any leaf is touched (a leaf that lacks the term would serve the row, the next one not)
            self._refuse_other_fields(q)
            if isinstance(q, PhraseQuery) and q.slop > 0 and len(set(q.terms)) < len(q.terms):
                raise RgpuError(-5, "phrase rescoring: a sloppy phrase that names a term twice is not served")
        out = np.ascontiguousarray(hits, dtype=_lib.HIT_DTYPE).copy()
        for phrase, rows in ((False, np.flatnonzero(~is_phrase)), (True, np.flatnonzero(is_phrase))):
            if rows.size == 0:
                continue
            mine, part = [rescore_queries[i] for i in rows], out[rows]
            for i, leaf in enumerate(self.leaves):
                finish = i == len(self.leaves) - 1
                if phrase:
                    qs, ts = self.pack_phrases(mine, leaf)
                    part = leaf.segment.rescore_phrase_batch(qs, ts, req[rows], part, finish=finish)
                else:
                    qs, ts = self.pack(mine, leaf)
                    part = leaf.segment.rescore_batch(qs, ts, req[rows], part, finish=finish)
            out[rows] = part
        return out

    @staticmethod
    def phrase_bool_parts(query):
        """A BooleanQuery with PhraseQuery clauses -> (required clauses in BooleanWeight::must_weights order: MUST clauses in query
        order, then FILTER clauses; how many of them are MUST clauses; MUST_NOT TermQuery clauses) when the GPU path serves the tree
        (rgpu_search_phrase_bool_batch), else UnsupportedOperation: a sloppy phrase clause (inside a conjunction the reference matches
        it on its approximation and scores a stale sloppy_freq — not reproduced), a phrase under SHOULD or MUST_NOT, a SHOULD clause
        of any kind beside a required phrase (ReqOptScorer), a nested BooleanQuery clause beside a phrase, more than 4 phrases."""
        if any(isinstance(q, PhraseQuery) for q in query.should_queries + query.must_not_queries):
            raise RgpuError(-5, "a phrase clause under SHOULD or MUST_NOT is not served by the GPU path")
        if query.should_queries:
            raise RgpuError(-5, "SHOULD clauses beside a required phrase are not served by the GPU path")
        required = list(query.must_queries) + list(query.filter_queries)
        if any(isinstance(q, BooleanQuery) for q in required + query.must_not_queries):
            raise RgpuError(-5, "nested boolean clauses beside a phrase are not served by the GPU path")
        phrases = [q for q in required if isinstance(q, PhraseQuery)]
        if any(q.slop > 0 for q in phrases):
            raise RgpuError(-5, "a sloppy phrase inside a boolean query is not served by the GPU path")
        if len(phrases) > _lib.MAX_BOOL_PHRASES:
            raise RgpuError(-5, "more than %d phrases in one boolean query" % _lib.MAX_BOOL_PHRASES)
        return required, len(query.must_queries), list(query.must_not_queries)

    def pack_phrase_bool(self, queries, leaf):
        """BooleanQuery objects with phrase clauses -> the (rgpu_phrase_bool_query[], rgpu_phrase_query[], rgpu_phrase_term[],
        rgpu_query_term[]) of rgpu_search_phrase_bool_batch for one leaf. A FILTER clause rides with weight 0 (needs_scores = false)."""
        parts = [self.phrase_bool_parts(q) for q in queries]
        phrase_qs, filtered, term_cs = [], [], []
        qs = np.zeros(len(queries), dtype=_lib.PHRASE_BOOL_QUERY_DTYPE)
        for i, (required, n_must, nots) in enumerate(parts):
            slots = [s for s, c in enumerate(required) if isinstance(c, PhraseQuery)]
            mine = [TermQuery(c.term, c.boost if s < n_must else 0.0) for s, c in enumerate(required) if not isinstance(c, PhraseQuery)]
            qs[i]["n_phrases"], qs[i]["first_phrase"] = len(slots), len(phrase_qs)
            qs[i]["n_terms"], qs[i]["first_term"], qs[i]["n_must_not"] = len(mine), len(term_cs), len(nots)
            qs[i]["phrase_slot"][:len(slots)] = slots
            phrase_qs += [required[s] for s in slots]
            filtered += [s >= n_must for s in slots]
            term_cs += mine + nots
        ps, pts = self.pack_phrases(phrase_qs, leaf)
        ps["weight"][np.array(filtered, dtype=bool)] = 0.0
        ps["next_limit"] = 0
        return qs, ps, pts, self._pack_term_clauses(term_cs, leaf)

    def _pack_term_clauses(self, term_cs, leaf):
        """TermQuery clauses -> rgpu_query_term[] for one leaf (a term the leaf lacks: doc_freq 0)"""
        byte_terms = [c.term for c in term_cs if isinstance(c.term, bytes)]
        if byte_terms:
            leaf.resolve(byte_terms)
            self.leaves[self._stats_leaf].resolve(byte_terms)
        ts = np.zeros(len(term_cs), dtype=QUERY_TERM_DTYPE)
        for at, c in enumerate(term_cs):
            w, table = self._weight(c.term, c.boost)
            st = leaf.term_state(c.term)
            if st is not None:
                ts[at]["state"] = st
            else:
                ts[at]["state"]["doc_freq"] = 0
                ts[at]["state"]["skip_offset"] = -1
                ts[at]["state"]["singleton_doc_id"] = -1
            ts[at]["weight"], ts[at]["sim_table"] = w, table
        return ts

    @staticmethod
    def phrase_or_parts(query):
        """A BooleanQuery without MUST and FILTER clauses, with PhraseQuery clauses -> (SHOULD clauses in query order, i.e.
        BooleanWeight::should_weights; MUST_NOT TermQuery clauses; min_should_match) when the GPU path serves the tree
        (rgpu_search_phrase_or_batch), else UnsupportedOperation: a sloppy phrase clause (two-phase), a phrase under MUST_NOT, a nested
        BooleanQuery clause, more than 4 phrases, ten or more SHOULD clauses (the reference then sums in heap order)."""
        if query.must_queries or query.filter_queries:
            raise RgpuError(-5, "phrase_or_parts: a disjunction has no MUST and no FILTER clause (phrase_bool_parts)")
        if any(isinstance(q, PhraseQuery) for q in query.must_not_queries):
            raise RgpuError(-5, "a phrase clause under MUST_NOT is not served by the GPU path")
        if any(isinstance(q, BooleanQuery) for q in query.should_queries + query.must_not_queries):
            raise RgpuError(-5, "nested boolean clauses beside a phrase are not served by the GPU path")
        phrases = [q for q in query.should_queries if isinstance(q, PhraseQuery)]
        if any(q.slop > 0 for q in phrases):
            raise RgpuError(-5, "a sloppy phrase inside a boolean query is not served by the GPU path")
        if len(phrases) > _lib.MAX_BOOL_PHRASES:
            raise RgpuError(-5, "more than %d phrases in one boolean query" % _lib.MAX_BOOL_PHRASES)
        if len(query.should_queries) > _lib.PHRASE_OR_MAX_SHOULD:
            raise RgpuError(-5, "ten or more SHOULD clauses with a phrase among them sum in heap order")
        return list(query.should_queries), list(query.must_not_queries), query.min_should_match

    def pack_phrase_or(self, queries, leaf):
        """BooleanQuery objects of SHOULD / MUST_NOT clauses with phrase clauses -> the (rgpu_phrase_or_query[], rgpu_phrase_query[],
        rgpu_phrase_term[], rgpu_query_term[]) of rgpu_search_phrase_or_batch for one leaf."""
        parts = [self.phrase_or_parts(q) for q in queries]
        phrase_qs, term_cs = [], []
        qs = np.zeros(len(queries), dtype=_lib.PHRASE_OR_QUERY_DTYPE)
        for i, (shoulds, nots, msm) in enumerate(parts):
            slots = [s for s, c in enumerate(shoulds) if isinstance(c, PhraseQuery)]
            mine = [c for c in shoulds if not isinstance(c, PhraseQuery)]
            qs[i]["n_phrases"], qs[i]["first_phrase"] = len(slots), len(phrase_qs)
            qs[i]["n_terms"], qs[i]["first_term"], qs[i]["n_must_not"] = len(mine), len(term_cs), len(nots)
            qs[i]["min_should_match"] = msm
            qs[i]["phrase_slot"][:len(slots)] = slots
            phrase_qs += [shoulds[s] for s in slots]
            term_cs += mine + nots
        ps, pts = self.pack_phrases(phrase_qs, leaf)
        ps["next_limit"] = 0
        return qs, ps, pts, self._pack_term_clauses(term_cs, leaf)

    @staticmethod
    def phrase_opt_parts(query):
        """A BooleanQuery with required (MUST / FILTER) AND SHOULD clauses and a PhraseQuery among them -> (required clauses in
        BooleanWeight::must_weights order: MUST clauses in query order, then FILTER clauses; how many of them are MUST clauses; SHOULD
        clauses in query order, i.e. should_weights; MUST_NOT TermQuery clauses; min_should_match) when the GPU path serves the tree
        (rgpu_search_phrase_opt_batch), else UnsupportedOperation: no required or no SHOULD clause (phrase_or_parts /
        phrase_bool_parts), a sloppy phrase clause, a phrase under MUST_NOT, a nested BooleanQuery clause, more than 4 phrases on
        either side, ten or more SHOULD clauses (the reference then sums in heap order)."""
        required = list(query.must_queries) + list(query.filter_queries)
        shoulds = list(query.should_queries)
        if not required or not shoulds:
            raise RgpuError(-5, "phrase_opt_parts: a MUST + SHOULD tree has a required and an optional clause")
        if any(isinstance(q, PhraseQuery) for q in query.must_not_queries):
            raise RgpuError(-5, "a phrase clause under MUST_NOT is not served by the GPU path")
        if any(not isinstance(q, (PhraseQuery, TermQuery)) for q in required + shoulds + list(query.must_not_queries)):
            raise RgpuError(-5, "nested boolean clauses beside a phrase are not served by the GPU path")
        if any(q.slop > 0 for q in required + shoulds if isinstance(q, PhraseQuery)):
            raise RgpuError(-5, "a sloppy phrase inside a boolean query is not served by the GPU path")
        for side in (required, shoulds):
            if sum(isinstance(q, PhraseQuery) for q in side) > _lib.MAX_BOOL_PHRASES:
                raise RgpuError(-5, "more than %d phrases on one side of a boolean query" % _lib.MAX_BOOL_PHRASES)
        if len(shoulds) > _lib.PHRASE_OR_MAX_SHOULD:
            raise RgpuError(-5, "ten or more SHOULD clauses sum in heap order")
        return required, len(query.must_queries), shoulds, list(query.must_not_queries), query.min_should_match

    def pack_phrase_opt(self, queries, leaf):
        """BooleanQuery objects of required and optional clauses with phrase clauses -> the (rgpu_phrase_opt_query[],
        rgpu_phrase_query[], rgpu_phrase_term[], rgpu_query_term[]) of rgpu_search_phrase_opt_batch for one leaf. A FILTER clause
        rides with weight 0 (needs_scores = false)."""
        parts = [self.phrase_opt_parts(q) for q in queries]
        phrase_qs, filtered, term_cs = [], [], []
        qs = np.zeros(len(queries), dtype=_lib.PHRASE_OPT_QUERY_DTYPE)
        for i, (required, n_must, shoulds, nots, msm) in enumerate(parts):
            rslots = [s for s, c in enumerate(required) if isinstance(c, PhraseQuery)]
            oslots = [s for s, c in enumerate(shoulds) if isinstance(c, PhraseQuery)]
            rterms = [TermQuery(c.term, c.boost if s < n_must else 0.0) for s, c in enumerate(required) if not isinstance(c, PhraseQuery)]
            oterms = [c for c in shoulds if not isinstance(c, PhraseQuery)]
            qs[i]["n_req_phrases"], qs[i]["n_opt_phrases"], qs[i]["first_phrase"] = len(rslots), len(oslots), len(phrase_qs)
            qs[i]["n_req_terms"], qs[i]["n_opt_terms"], qs[i]["first_term"], qs[i]["n_must_not"] = len(rterms), len(oterms), len(term_cs), len(nots)
            qs[i]["min_should_match"] = msm
            qs[i]["req_phrase_slot"][:len(rslots)] = rslots
            qs[i]["opt_phrase_slot"][:len(oslots)] = oslots
            phrase_qs += [required[s] for s in rslots] + [shoulds[s] for s in oslots]
            filtered += [s >= n_must for s in rslots] + [False] * len(oslots)
            term_cs += rterms + oterms + nots
        ps, pts = self.pack_phrases(phrase_qs, leaf)
        if len(filtered):
            ps["weight"][np.array(filtered, dtype=bool)] = 0.0
        ps["next_limit"] = 0
        return qs, ps, pts, self._pack_term_clauses(term_cs, leaf)

    # ---- doc sets: cached filters as FILTER / MUST_NOT masks ---------------------------------------------------------------------
    def _cached(self, sets):
        if len(sets) != len(self.leaves):
            raise RgpuError(-2, "a cached filter holds one doc set per leaf")
        return CachedFilter(self, sets)

    def cache_filter(self, query):
        """LRUQueryCache::do_cache for a query the GPU can collect itself (rgpu_docset_collect_batch): a TermQuery or a flat
        BooleanQuery that packs to TERM / AND / OR with min_should_match <= 1, MUST_NOT term clauses allowed. Per leaf the docs the
        query matches, live docs NOT applied (query_cache.rs:335-342). Anything else: UnsupportedOperation."""
        op, _clauses, opts, _nots = self._flatten(query)
        if opts or op not in (OP_TERM, OP_AND, OP_OR):
            raise RgpuError(-5, "a filter is collected on the GPU from a term query or a flat all-MUST / all-SHOULD boolean query")
        return self._cached([leaf.segment.docset_collect_batch(*self.pack([query], leaf))[0] for leaf in self.leaves])

    def filter_from_docs(self, global_doc_ids):
        """A filter from GLOBAL doc ids (any order, repeats allowed), split by the leaves' doc bases."""
        ids = np.asarray(global_doc_ids, dtype=np.int64).ravel()
        if ids.size and (ids.min() < 0 or ids.max() >= max(leaf.doc_base + leaf.max_doc for leaf in self.leaves)):
            raise RgpuError(-2, "a doc id outside the index")
        sets, taken = [], 0
        for leaf in self.leaves:
            mine = ids[(ids >= leaf.doc_base) & (ids < leaf.doc_base + leaf.max_doc)]
            taken += mine.size
            sets.append(leaf.segment.docset_from_docs((mine - leaf.doc_base).astype(np.int32)))
        if taken != ids.size:
            raise RgpuError(-2, "a doc id outside every leaf")
        return self._cached(sets)

    def filter_from_bits(self, per_leaf_words):
        """A filter from FixedBitSet words, one u64 array of ceil(max_doc / 64) words per leaf (what a cached BitDocIdSet holds)."""
        if len(per_leaf_words) != len(self.leaves):
            raise RgpuError(-2, "a cached filter holds one bit set per leaf")
        return self._cached([leaf.segment.docset_from_words(w) for leaf, w in zip(self.leaves, per_leaf_words)])

    def attach_points(self, field, per_leaf, bytes_per_dim=None):
        """The one-dimensional points of `field`: per leaf a (docs, values) pair — leaf-local doc ids in any order, a doc may repeat,
        and the sortable bytes of the values as a u8 array [n, bytes] (or n byte strings) — or None for a leaf without the field
        (the reference has no scorer there: nothing matches under MUST / FILTER, nothing is excluded under MUST_NOT). open_directory
        attaches nothing: this mirror reads no .dim file."""
        if len(per_leaf) != len(self.leaves):
            raise RgpuError(-2, "points are attached per leaf")
        held, width = [], bytes_per_dim
        for leaf, pair in zip(self.leaves, per_leaf):
            if pair is None:
                held.append(None)
                continue
            docs, values = pair
            if isinstance(values, (list, tuple)):
                values = np.frombuffer(b"".join(bytes(v) for v in values), np.uint8).reshape(len(values), -1) if len(values) else np.zeros((0, width or 4), np.uint8)
            values = np.asarray(values, dtype=np.uint8)
            w = values.shape[1] if values.ndim == 2 else width
            if w is None or (width is not None and w != width):
                raise RgpuError(-2, "the values of a point field have one width (pass [n, bytes] arrays, or bytes_per_dim)")
            width = w
            held.append(leaf.segment.attach_points(w, docs, values))
        if width is None:
            raise RgpuError(-2, "no leaf holds the field")
        old = self._points.pop(field, None)
        for key in [k for k in self._range_filters if k[0] == field]:
            del self._range_filters[key]
        self._points[field] = (int(width), held)
        if old:
            for pts in old[1]:
                if pts is not None:
                    pts.close()

    def range_filter(self, query, path=0):
        """PointRangeQuery -> CachedFilter, built on the GPU from the attached points (rgpu_docset_from_point_ranges), one set per
        leaf; memoised per (field, lower, upper). A field never attached: UnsupportedOperation; bounds whose length is not the
        field's: IllegalArgument (point_range_query.rs:510-522). The memo holds the `range_filter_capacity` most recently used
        ranges (search_batch trims it before it peels a batch; drop_range_filters empties it): a range that moves with every query
        would otherwise leave ceil(max_doc / 64) * 8 bytes per leaf in HBM per query. A CachedFilter the caller still holds stays
        usable after it left the memo; its sets are freed with its last reference."""
        return self._range_filters_for([query], path)[0]

    def _check_ranges(self, queries):
        """what can be wrong with a PointRangeQuery, before anything is built: dimensions, field, width"""
        for q in queries:
            if q.num_dims != 1:
                raise RgpuError(-5, "a multi-dimensional point range is not served by the GPU path (its matches depend on the BKD cell layout)")
            if q.field not in self._points:
                raise RgpuError(-5, "no points are attached for field %r: the range stays on the CPU path" % q.field)
            width = self._points[q.field][0]
            if len(q.lower) != width:
                raise RgpuError(-2, "field=%r was indexed with bytesPerDim=%d but this query has bytesPerDim=%d" % (q.field, width, len(q.lower)))

    def _range_filters_for(self, queries, path=0):
        """the memoised CachedFilters of `queries` (PointRangeQuery); the missing ones of a field are built in ONE call per leaf"""
        self._check_ranges(queries)
        todo = {}
        for q in queries:
            key = (q.field, q.lower, q.upper)
            if key in self._range_filters:
                self._range_filters[key] = self._range_filters.pop(key)   # most recently used last
            else:
                todo.setdefault(q.field, {})[key] = None
        for field, keys in todo.items():
            keys = list(keys)
            width, held = self._points[field]
            bounds = _lib.point_ranges([(k[1], k[2]) for k in keys], width)
            per_leaf = []
            for leaf, pts in zip(self.leaves, held):
                if pts is None:   # no such field in this leaf: the empty set
                    per_leaf.append([leaf.segment.docset_from_docs(np.zeros(0, np.int32)) for _ in keys])
                else:
                    per_leaf.append(pts.range_docsets(bounds, path))
            for j, key in enumerate(keys):
                self._range_filters[key] = self._cached([sets[j] for sets in per_leaf])
        return [self._range_filters[(q.field, q.lower, q.upper)] for q in queries]

    def drop_range_filters(self, keep=0):
        """Forget all but the `keep` most recently used memoised range filters, and every memoised combination (_mask) that names a
        forgotten one: their doc sets are freed once nobody else holds the CachedFilter."""
        while len(self._range_filters) > max(0, int(keep)):
            gone = self._range_filters.pop(next(iter(self._range_filters)))
            for key in [k for k in self._masks if id(gone) in k[0] or id(gone) in k[1]]:
                del self._masks[key]

    def _filtered_phrase(self, rest):
        """A phrase, or a BooleanQuery over phrases, left under a mask: served when the searcher opted in (filtered_phrases) and every
        phrase is exact - on a leaf whose live docs are live AND filters AND NOT excludes an exact phrase collects the reference's docs,
        counts and scores, a sloppy one does not (next_limit counts deleted docs, not docs outside a filter)."""
        if not getattr(self, "filtered_phrases", False) or (isinstance(rest, PhraseQuery) and rest.slop > 0):
            raise RgpuError(-5, "a filtered phrase is not served by the GPU path")
        if isinstance(rest, BooleanQuery):   # (their refusals: sloppy clauses, nested clauses, SHOULD beside a required phrase ...)
            (self.phrase_bool_parts if (rest.must_queries or rest.filter_queries) else self.phrase_or_parts)(rest)

    def _peel(self, query, build=True):
        """query -> (the query without its doc-set clauses, (FILTER CachedFilters, MUST_NOT CachedFilters)). The rest, searched on
        live docs AND filters AND NOT excludes, collects the reference's docs, counts and f32 scores when (1) it contributes a MUST
        or FILTER clause of its own — "b c #F" is ReqOptScorer(F, b | c) in the reference and matches ALL of F, a lone #F likewise —
        and (2) for -X, min_should_match <= 1 (boolean_query.rs:235-251 reuses it for the MUST_NOT union). FilterQuery(Q, F) asks
        only that Q has a scorer of its own. Phrases are not served under a mask unless the searcher opted in (filtered_phrases), and
        then exact ones only (a sloppy phrase's next_limit counts deleted docs, not docs outside a filter); with the opt-in
        "a b" c -X (min_should_match <= 1) is served too: ReqNotScorer over the disjunction, whose phrase clause is a scorer of its own.
        Anything else: UnsupportedOperation — unless the searcher opted in to required_sets: a query whose only required clauses are doc
        sets (MatchAllDocsQuery among them, which a query of MUST_NOT clauses alone gets from build()) then comes back as a
        _RequiredSet holding its SHOULD clauses (_peel_required), and "b c -X" as the masked disjunction it is.
        A PointRangeQuery under MUST / FILTER / MUST_NOT is checked first (dimensions, field, width), the rules above are applied, and
        only then is its doc set built; build=False stops short of that (the sets are then the queries themselves) — search_batch
        runs it over the whole batch first, so a refused row launches nothing. min_should_match stays the query's own: "+range #a b"
        has 0 (it had a MUST clause), where build() would give the rest "#a b" 1."""
        self._refuse_other_fields(query)
        if isinstance(query, FilterQuery):
            inner, (f, x) = self._peel(query.query, build)
            if isinstance(inner, PhraseQuery) or (isinstance(inner, BooleanQuery) and inner.has_phrases()):
                self._filtered_phrase(inner)
            return inner, (f + list(query.filters), x)
        required_sets = getattr(self, "required_sets", False)
        if isinstance(query, PointRangeQuery):
            if not required_sets:
                raise RgpuError(-5, "a lone point range is not served by the GPU path (the reference matches all of it)")
            self._check_ranges([query])
            return _RequiredSet([]), (self._sets_of([query]) if build else [query], [])
        if isinstance(query, MatchAllDocsQuery):
            if not required_sets:
                raise RgpuError(-5, "MatchAllDocsQuery is not served by the GPU path (required_sets)")
            return _RequiredSet([]), (self._sets_of([query]) if build else [query], [])
        if not isinstance(query, BooleanQuery):
            return query, ([], [])
        sets = (CachedFilter, PointRangeQuery, MatchAllDocsQuery)
        f = [q for q in list(query.must_queries) + list(query.filter_queries) if isinstance(q, sets)]   # a range under MUST adds + 0.0 as under FILTER
        x = [q for q in query.must_not_queries if isinstance(q, sets)]
        # "-t": BooleanQuery::build gives a query of MUST_NOT clauses alone a MatchAllDocsQuery MUST clause (boolean_query.rs:76-79)
        only_nots = required_sets and bool(query.must_not_queries) and not (query.must_queries or query.filter_queries or query.should_queries)
        if not f and not x and not only_nots:
            return query, ([], [])
        if not required_sets and any(isinstance(q, MatchAllDocsQuery) for q in f + x):
            raise RgpuError(-5, "MatchAllDocsQuery is not served by the GPU path (required_sets)")
        self._check_ranges([q for q in f + x if isinstance(q, PointRangeQuery)])
        musts = [q for q in query.must_queries if not isinstance(q, sets)]
        filters = [q for q in query.filter_queries if not isinstance(q, sets)]
        must_nots = [q for q in query.must_not_queries if not isinstance(q, sets)]
        phrase_or = getattr(self, "filtered_phrases", False) and not f and any(isinstance(q, PhraseQuery) for q in query.should_queries)
        if not (musts or filters) and not phrase_or:
            if not required_sets:
                raise RgpuError(-5, "a doc set as the only required clause is not served by the GPU path (the reference matches all of it)")
            if f or not query.should_queries:
                return self._peel_required(query, f, x, must_nots, build)
            # "b c -X": no MatchAllDocsQuery is inserted beside SHOULD clauses; ReqNotScorer(DisjunctionSumScorer(b, c), X) collects
            # the disjunction's docs outside X — the disjunction has a scorer of its own, so the masked search below is that query
        if x and query.min_should_match > 1:
            raise RgpuError(-5, "a MUST_NOT doc set beside min_should_match >= 2 is not served by the GPU path")
        rest = BooleanQuery.build(musts, list(query.should_queries), filters=filters, must_nots=must_nots,
                                  min_should_match=query.min_should_match)
        if isinstance(rest, BooleanQuery) and rest.min_should_match != query.min_should_match:
            # (the peeled clauses were the only MUST ones: build() has derived the default of a query without MUST clauses)
            rest = BooleanQuery(musts, list(query.should_queries), query.min_should_match, must_nots, filters)
        if isinstance(rest, PhraseQuery) or (isinstance(rest, BooleanQuery) and rest.has_phrases()):
            self._filtered_phrase(rest)
        if build:
            made = self._sets_of(f + x)
            f, x = made[:len(f)], made[len(f):]
        return rest, (f, x)

    def _sets_of(self, clauses):
        """doc-set clauses as CachedFilters: a PointRangeQuery's memoised range filter (the missing ones built in one call per leaf),
        MatchAllDocsQuery's every-doc set, a CachedFilter itself"""
        made = iter(self._range_filters_for([q for q in clauses if isinstance(q, PointRangeQuery)]))
        out = []
        for q in clauses:
            if isinstance(q, PointRangeQuery):
                out.append(next(made))
            elif isinstance(q, MatchAllDocsQuery):
                if self._every_doc is None:   # rgpu_docset_combine of no operands: every doc of the leaf, once per leaf
                    self._every_doc = self._cached([leaf.segment.docset_combine() for leaf in self.leaves])
                out.append(self._every_doc)
            else:
                out.append(q)
        return out

    def _not_filter(self, must_nots):
        """MUST_NOT term clauses of a row whose required clauses are doc sets, as one excluded CachedFilter: the union of their docs,
        collected per leaf by one rgpu_docset_collect_batch OR row, memoised per clause tuple and bounded like the range filters"""
        key = tuple(c.term for c in must_nots)
        if key in self._not_filters:
            self._not_filters[key] = self._not_filters.pop(key)   # most recently used last
        else:
            union = TermQuery(key[0]) if len(key) == 1 else BooleanQuery([], [TermQuery(t) for t in key], 1)
            self._not_filters[key] = self._cached([leaf.segment.docset_collect_batch(*self.pack([union], leaf))[0] for leaf in self.leaves])
            while len(self._not_filters) > max(1, int(self.range_filter_capacity)):
                gone = self._not_filters.pop(next(iter(self._not_filters)))
                for mk in [m for m in self._masks if id(gone) in m[0] or id(gone) in m[1]]:
                    del self._masks[mk]
        return self._not_filters[key]

    def _peel_required(self, query, f, x, must_nots, build):
        """The required-set route of _peel: doc sets f (none: build()'s MatchAllDocsQuery) are the only required clauses. ->
        (_RequiredSet(the SHOULD clauses), (filters, excludes)) with the MUST_NOT term clauses among the excludes. The reference
        builds ReqOptScorer(sets, DisjunctionSumScorer(shoulds)), in a ReqNotScorer when there are exclusions; min_should_match
        reaches the MUST_NOT union only (boolean_query.rs:235-251), hence the existing rule for exclusions."""
        if (x or must_nots) and query.min_should_match > 1:
            raise RgpuError(-5, "an exclusion beside min_should_match >= 2 is not served by the GPU path")
        for q in query.should_queries:
            if not isinstance(q, TermQuery):
                raise RgpuError(-5, "beside a doc set as the only required clause the SHOULD clauses are term queries")
            if not q.boost > 0.0:
                raise RgpuError(-5, "beside a doc set as the only required clause a SHOULD clause has a boost > 0")
        if any(not isinstance(q, TermQuery) for q in must_nots):
            raise RgpuError(-5, "beside a doc set as the only required clause the MUST_NOT clauses are terms and doc sets")
        if len(query.should_queries) > _lib.MAX_QUERY_TERMS or len(must_nots) > _lib.MAX_QUERY_TERMS:
            raise RgpuError(-5, "more than %d clauses" % _lib.MAX_QUERY_TERMS)
        f = list(f) or [MatchAllDocsQuery()]
        if build:
            made = self._sets_of(f + x)
            f, x = made[:len(f)], made[len(f):]
            if must_nots:
                x = x + [self._not_filter(must_nots)]
        else:
            x = x + list(must_nots)
        return _RequiredSet(query.should_queries), (f, x)

    def _mask(self, filters, excludes):
        """One DocSet per leaf for a (filters, excludes) combination: combined once per combination and leaf
        (rgpu_docset_combine), memoised on the searcher; a single filter without excludes is its own mask."""
        for c in filters + excludes:
            if c.searcher is not self:
                raise RgpuError(-2, "a cached filter belongs to the searcher that made it")
        key = (tuple(sorted({id(c) for c in filters})), tuple(sorted({id(c) for c in excludes})))
        if key not in self._masks:
            if len(key[0]) == 1 and not key[1]:
                sets = filters[0].sets
            else:
                fs, xs = list({id(c): c for c in filters}.values()), list({id(c): c for c in excludes}.values())
                sets = [leaf.segment.docset_combine([c.sets[i] for c in fs], [c.sets[i] for c in xs]) for i, leaf in enumerate(self.leaves)]
            self._masks[key] = (filters + excludes, sets)   # (the CachedFilters stay alive as long as their ids are keys)
        return key, self._masks[key][1]

    def search_batch(self, queries, k):
        """-> (hits[n][k] structured {doc, score}, total_hits[n]) merged over all leaves. A batch may mix term / boolean / dismax /
        boosting queries (rgpu_search_batch), PhraseQuery rows (rgpu_search_phrase_batch), BooleanQuery rows with phrases among their
        required clauses (rgpu_search_phrase_bool_batch) and BooleanQuery rows of SHOULD / MUST_NOT clauses with phrases among the
        SHOULD ones (rgpu_search_phrase_or_batch) and top-level ordered SpanNearQuery rows over SpanTermQuery clauses
        (rgpu_search_span_near_batch; with unordered_spans the unordered ones through rgpu_search_span_unordered_batch; any other span
        query is UnsupportedOperation): one call per kind and leaf, rows keep their order. Rows with doc-set clauses
        (CachedFilter under FILTER / MUST_NOT, FilterQuery) are grouped by their combination of sets and searched masked
        (rgpu_search_batch_masked; with filtered_phrases the phrase kinds through their masked calls), one call per group, kind and leaf.
        Rows that name a further field of the leaves (TermQuery(field=...)) go to rgpu_search_fields_batch, which serves k <= 128: a
        batch that holds such a row is UnsupportedOperation as a whole for k > 128, its primary-field rows included (they are served
        up to k = 1024 in a batch of their own) - a batch has one k, and a refused batch launches nothing."""
        # rows that name a further field of the leaves (TermQuery(field=...)) go to rgpu_search_fields_batch; a batch without one
        # goes exactly where it went
        cross = [i for i, q in enumerate(queries) if self._names_other_field(q)]
        if cross:
            crossed = set(cross)
            rest = [i for i in range(len(queries)) if i not in crossed]
            specs = [self._cross_spec(queries[i]) for i in cross]   # refused before any leaf is touched
            if k > 128:
                raise RgpuError(-5, "a cross-field query is served for k <= 128")
            hits, totals = np.zeros((len(queries), k), dtype=_lib.HIT_DTYPE), np.zeros(len(queries), dtype=np.int64)
            if rest:
                hits[rest], totals[rest] = self.search_batch([queries[i] for i in rest], k)
            hits[cross], totals[cross] = self._cross_rows(specs, k)
            return hits, totals
        for q in queries:   # refused before any leaf is touched and before any range's set is built
            _refuse_unserved_spans(q, getattr(self, "unordered_spans", False))
            self._peel(q, build=False)
        if getattr(self, "_range_filters", None):   # (a batch on a searcher that never built a range filter goes the way it went)
            self.drop_range_filters(keep=self.range_filter_capacity)
        peeled = [self._peel(q) for q in queries]
        if not any(f or x for _, (f, x) in peeled):
            per_leaf = self._rows_per_leaf(queries, k, None)
        else:
            groups = {}   # key -> (masks per leaf or None, caller rows): first appearance first, caller order inside a group
            for i, (rest, (f, x)) in enumerate(peeled):
                key, masks = self._mask(f, x) if (f or x) else (None, None)
                if isinstance(rest, _RequiredSet):   # the same sets as the ONLY required clauses: a group, and a call, of its own
                    key = (key, "required")
                groups.setdefault(key, (masks, []))[1].append(i)
            per_leaf = [(np.zeros((len(queries), k), dtype=_lib.HIT_DTYPE), np.zeros(len(queries), dtype=np.int64)) for _ in self.leaves]
            for masks, rows in groups.values():
                part = self._rows_per_leaf([peeled[i][0] for i in rows], k, masks)
                for (hits, totals), (h, t) in zip(per_leaf, part):
                    hits[rows], totals[rows] = h, t
        if len(per_leaf) == 1:
            return per_leaf[0]
        return self._merge_leaves(per_leaf, len(queries), k)

    def _rows_per_leaf(self, queries, k, masks):
        """[(hits, totals)] per leaf for queries without doc-set clauses; masks: one DocSet per leaf the search is restricted to"""
        def kind(q):
            if isinstance(q, PhraseQuery):
                return 1
            if isinstance(q, SpanNearQuery):
                return 4 if q.in_order else 5
            if isinstance(q, BooleanQuery) and q.has_phrases():   # no MUST, no FILTER: the disjunction route; else phrase_bool_parts decides
                if (q.must_queries or q.filter_queries) and q.should_queries and getattr(self, "optional_phrases", False):
                    return 6   # required AND optional clauses (optional_phrases): phrase_opt_parts decides
                return 2 if (q.must_queries or q.filter_queries) else 3
            return 0
        if queries and isinstance(queries[0], _RequiredSet):   # (a group holds such rows alone: search_batch)
            return self._required_rows_per_leaf(queries, k, masks)
        kinds = [kind(q) for q in queries]
        if not any(kinds):
            per_leaf = []
            for i, leaf in enumerate(self.leaves):
                qs, ts = self.pack(queries, leaf)
                per_leaf.append(leaf.segment.search_batch(qs, ts, k) if masks is None else leaf.segment.search_batch_masked(masks[i], qs, ts, k))
        else:
            if masks is not None and (not getattr(self, "filtered_phrases", False) or any(q.slop > 0 for q in queries if isinstance(q, PhraseQuery))):
                raise RgpuError(-5, "a filtered phrase is not served by the GPU path")
            if masks is not None and (4 in kinds or 5 in kinds):
                raise RgpuError(-5, "a filtered span query is not served by the GPU path")
            if 5 in kinds and not getattr(self, "unordered_spans", False):   # (search_batch has refused it already)
                raise RgpuError(-5, "an unordered SpanNearQuery is not served by the GPU path")
            if masks is not None and 6 in kinds:
                raise RgpuError(-5, "a filtered MUST + SHOULD tree over phrases is not served by the GPU path")
            rows = [np.flatnonzero(np.array(kinds) == kd) for kd in (0, 1, 2, 3, 4, 5, 6)]
            groups = [[queries[i] for i in r] for r in rows]
            for q in groups[2]:   # refused before any leaf is touched
                self.phrase_bool_parts(q)
            for q in groups[3]:
                self.phrase_or_parts(q)
            for q in groups[6]:
                self.phrase_opt_parts(q)
            per_leaf = []
            for i, leaf in enumerate(self.leaves):
                hits, totals = np.zeros((len(queries), k), dtype=_lib.HIT_DTYPE), np.zeros(len(queries), dtype=np.int64)
                seg = leaf.segment
                if groups[0]:
                    qs, ts = self.pack(groups[0], leaf)
                    hits[rows[0]], totals[rows[0]] = seg.search_batch(qs, ts, k) if masks is None else seg.search_batch_masked(masks[i], qs, ts, k)
                if groups[1]:
                    qs, ts = self.pack_phrases(groups[1], leaf)
                    hits[rows[1]], totals[rows[1]] = seg.search_phrase_batch(qs, ts, k) if masks is None else seg.search_phrase_batch_masked(masks[i], qs, ts, k)
                if groups[2]:
                    packed = self.pack_phrase_bool(groups[2], leaf)
                    hits[rows[2]], totals[rows[2]] = (seg.search_phrase_bool_batch(*packed, k) if masks is None
                                                      else seg.search_phrase_bool_batch_masked(masks[i], *packed, k))
                if groups[3]:
                    packed = self.pack_phrase_or(groups[3], leaf)
                    hits[rows[3]], totals[rows[3]] = (seg.search_phrase_or_batch(*packed, k) if masks is None
                                                      else seg.search_phrase_or_batch_masked(masks[i], *packed, k))
                if groups[4]:   # ordered SpanNearQuery rows: packed as phrases, clause i at position i
                    qs, ts = self.pack_phrases(groups[4], leaf)
                    hits[rows[4]], totals[rows[4]] = seg.search_span_near_batch(qs, ts, k)
                if groups[5]:   # unordered SpanNearQuery rows (unordered_spans): packed exactly as the ordered ones
                    qs, ts = self.pack_phrases(groups[5], leaf)
                    hits[rows[5]], totals[rows[5]] = seg.search_span_unordered_batch(qs, ts, k)
                if groups[6]:   # MUST + SHOULD trees over phrases (optional_phrases)
                    hits[rows[6]], totals[rows[6]] = seg.search_phrase_opt_batch(*self.pack_phrase_opt(groups[6], leaf), k)
                per_leaf.append((hits, totals))
        return per_leaf

    def _required_rows_per_leaf(self, rests, k, masks):
        """[(hits, totals)] per leaf for rows whose only required clauses are the doc sets behind `masks`
        (rgpu_search_batch_required_set): the rows' SHOULD sides as TERM / OR queries, {OR, no clause} where there is none"""
        some = [i for i, r in enumerate(rests) if r.shoulds]
        scored = [rests[i].shoulds[0] if len(rests[i].shoulds) == 1 else BooleanQuery([], list(rests[i].shoulds), 1) for i in some]
        per_leaf = []
        for i, leaf in enumerate(self.leaves):
            qs = np.zeros(len(rests), dtype=QUERY_DTYPE)
            qs["op"] = OP_OR
            ts = np.zeros(0, dtype=QUERY_TERM_DTYPE)
            if scored:
                qs[some], ts = self.pack(scored, leaf)
            per_leaf.append(leaf.segment.search_batch_required_set(masks[i], qs, ts, k))
        return per_leaf

    def _merge_leaves(self, per_leaf, n_queries, k):
        # TopDocsCollector::finish_parallel (top_docs.rs:157-172) on the device: [leaf][query][k] -> [query][k]
        import torch
        hits = torch.from_numpy(np.stack([h.view(np.int64).reshape(n_queries, k) for h, _ in per_leaf])).cuda()
        totals = torch.from_numpy(np.stack([t for _, t in per_leaf])).cuda()
        out_h = torch.empty((n_queries, k), dtype=torch.int64, device="cuda")
        out_t = torch.empty((n_queries,), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        self.ctx.merge_topk_device(hits.data_ptr(), totals.data_ptr(), len(per_leaf), n_queries, k, out_h.data_ptr(), out_t.data_ptr())
        self.ctx.synchronize()  # the merge is only enqueued (on the ctx's stream)
        return out_h.cpu().numpy().view(_lib.HIT_DTYPE).reshape(n_queries, k), out_t.cpu().numpy()

    def search(self, query, collector):
        """IndexSearcher::search(query, collector) for a TopDocsCollector."""
        try:
            if not isinstance(collector, TopDocsCollector):
                raise RgpuError(-5, "only TopDocsCollector is served by the GPU path")
            hits, totals = self.search_batch([query], collector.estimated_hits)
        except RgpuError as e:
            # ErrorKind::UnsupportedOperation -> the CPU searcher, exactly where rust/gpu/searcher.rs falls back to DefaultIndexSearcher
            if e.status == -5 and self.cpu_fallback is not None:
                return self.cpu_fallback(query, collector)
            raise
        row = hits[0]
        docs = [(int(d), float(s)) for d, s in zip(row["doc"], row["score"]) if d >= 0]
        collector._result = TopDocs(int(totals[0]), docs)

    # ---- IndexSearcher::count (search/searcher.rs:632-654): hit counts without scoring ------------------------------------------
    cpu_count_fallback = None   # cpu_count_fallback(query) -> int: where count() hands what the GPU path refuses (UnsupportedOperation); None: raise

    def _leaf_num_docs(self, leaf):
        if leaf.live_docs is None:
            return int(leaf.max_doc)
        words = np.ascontiguousarray(leaf.live_docs, dtype=np.uint64)
        return int(np.unpackbits(words.view(np.uint8), bitorder="little")[:leaf.max_doc].sum())

    def count(self, query):
        """IndexSearcher::count. MatchAllDocsQuery: num_docs from the leaves' live docs, no GPU call (searcher.rs:636-638); a TermQuery on
        leaves without deletions: the sum of doc_freq, no GPU call (:640-648); anything else through count_batch. What the GPU path
        refuses (UnsupportedOperation: phrases, spans, nested trees) goes to cpu_count_fallback(query) when that is set."""
        if isinstance(query, MatchAllDocsQuery):
            return sum(self._leaf_num_docs(leaf) for leaf in self.leaves)
        if isinstance(query, TermQuery) and self._primary(query) and all(leaf.live_docs is None for leaf in self.leaves):
            states = [leaf.term_state(query.term) for leaf in self.leaves]
            return sum(int(st["doc_freq"]) for st in states if st is not None)
        try:
            return int(self.count_batch([query])[0])
        except RgpuError as e:
            if e.status == -5 and self.cpu_count_fallback is not None:
                return int(self.cpu_count_fallback(query))
            raise

    def count_batch(self, queries):
        """-> int64[n]: the live docs each query matches, summed over the leaves (rgpu_count_batch per leaf; nothing is scored). Rows
        with doc-set clauses are grouped by their combination of sets exactly as search_batch groups them and counted under the group's
        mask; a row whose only required clauses are doc sets (required_sets=True) matches all of live AND sets whatever its SHOULD
        clauses say: the live cardinality of its mask (rgpu_docset_head with n = 0). Whatever search_batch refuses, and phrases and
        spans in any position, are UnsupportedOperation."""
        for q in queries:   # refused before any leaf is touched and before any range's set is built
            self._refuse_other_fields(q)
            if _holds_span(q) or isinstance(q, (PhraseQuery, SpanNearQuery)) or (isinstance(q, BooleanQuery) and q.has_phrases()):
                raise RgpuError(-5, "a count is served by the GPU path for term, boolean, dismax and boosting queries")
            rest, _ = self._peel(q, build=False)
            if isinstance(rest, PhraseQuery) or (isinstance(rest, BooleanQuery) and rest.has_phrases()):
                raise RgpuError(-5, "a count is served by the GPU path for term, boolean, dismax and boosting queries")
        if getattr(self, "_range_filters", None):
            self.drop_range_filters(keep=self.range_filter_capacity)
        peeled = [self._peel(q) for q in queries]
        counts = np.zeros(len(queries), dtype=np.int64)
        groups = {}   # key -> (masks per leaf or None, caller rows): first appearance first, caller order inside a group
        for i, (rest, (f, x)) in enumerate(peeled):
            key, masks = self._mask(f, x) if (f or x) else (None, None)
            if isinstance(rest, _RequiredSet):
                key = (key, "required")
            groups.setdefault(key, (masks, []))[1].append(i)
        for masks, rows in groups.values():
            rests = [peeled[i][0] for i in rows]
            for li, leaf in enumerate(self.leaves):
                if isinstance(rests[0], _RequiredSet):   # (a group holds such rows alone)
                    counts[rows] += leaf.segment.docset_head(masks[li], 0)[1]
                    continue
                qs, ts = self.pack(rests, leaf)
                counts[rows] += leaf.segment.count_batch(qs, ts, None if masks is None else masks[li])
        return counts
