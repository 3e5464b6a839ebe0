// GpuIndexSearcher — the drop-in seam of SURVEY §8(b) / §8(f)1, as a file a Rucene maintainer copies to
// src/core/search/gpu/searcher.rs (next to ffi.rs, which scripts/gen_rust_ffi.py writes from include/rucene_gpu.h).
//
// NOT COMPILED IN THIS REPOSITORY: the image has no rustc, the reference needs nightly-2020-03-12 and 24 un-vendored crates.
// The file is written against the reference's own PUBLIC items (paths relative to src/core/) plus the four small accessors of
// rust/rucene_accessors.patch, and kept deliberately thin: every decision that affects results lives behind the C ABI and
// is tested there (tests/, through ctypes and C++). What this file adds is pattern-matching of query trees, term resolution
// through Rucene's own term dictionary, BM25 weights from Rucene's own statistics (the arithmetic itself is the library's
// rgpu_bm25_compute_weight, bit-exact with bm25_similarity.rs:99-177 — BM25Similarity keeps idf / avg_field_length private),
// and the hand-over of hits to the caller's collector. The same logic exists, compiled and tested, as the C++ mirror
// rucene_amd/csrc/host/gpu_index_searcher.hpp and the Python mirror rucene_amd/searcher.py.
//
// Crate-side hooks (rust/rucene_accessors.patch; the fields exist, they are only private today):
//   * search/query/boolean_query.rs   pub(crate) fn clauses(&self) -> (&[Box<dyn Query<C>>], &[..should], &[..filter], &[..must_not], i32)
//   * search/query/phrase_query.rs    pub(crate) fn parts(&self) -> (&str, &[Term], &[i32], i32)
//   * search/collector/top_docs.rs    pub(crate) fn estimated_hits(&self) -> usize
//                                     pub(crate) fn add_leaf_result(&mut self, hits: &[(DocId, f32)], total_hits: usize)
//       = what finish_parallel does with one LeafTopDocs (top_docs.rs:157-172): total_hits += n; add_doc(doc, score) per hit.
// and, for `unordered_spans` (rust/rucene_span_accessor.patch, a file of its own):
//   * search/query/spans/span_near.rs pub(crate) fn parts(&self) -> (&str, &[SpanQueryEnum], i32, bool)
use std::collections::HashMap;
use std::ops::Deref;
use std::sync::Mutex;

use core::codec::points::{IntersectVisitor, PointValues, Relation};
use core::codec::postings::blocktree::BlockTermState;
use core::codec::{Codec, TermIterator, Terms};
use core::doc::Term;
use core::index::reader::{IndexReader, LeafReader, LeafReaderContext};
use core::search::collector::{SearchCollector, TopDocsCollector};
use core::search::query::spans::{SpanNearQuery, SpanQueryEnum};
use core::search::query::{BooleanQuery, DisjunctionMaxQuery, PhraseQuery, Query, TermQuery};
use core::search::searcher::{DefaultIndexSearcher, IndexSearcher, SearchPlanBuilder};
use core::search::similarity::SimilarityProducer;
use core::search::statistics::{CollectionStatistics, TermStatistics};
use core::util::DocId;
use error::{Error, ErrorKind, Result};

use super::ffi::*;

/// BM25Similarity::default() (bm25_similarity.rs:55-59) — what DefaultSimilarityProducer hands every field. A searcher built
/// with another SimilarityProducer must not be wrapped by this shim (open() cannot see the producer's parameters).
const BM25_K1: f32 = 1.2;
const BM25_B: f32 = 0.75;

/// status -> error.rs ErrorKind (error.rs:24-91); nothing panics across the boundary
pub fn check(rc: i32, ctx: *mut RgpuCtx) -> Result<()> {
    use error::ErrorKind::*;
    if rc >= 0 {
        return Ok(());
    }
    let msg = unsafe { std::ffi::CStr::from_ptr(rgpu_last_error(ctx)) }.to_string_lossy().into_owned();
    bail!(match rc {
        RGPU_ERR_ILLEGAL_STATE => IllegalState(msg),
        RGPU_ERR_ILLEGAL_ARGUMENT => IllegalArgument(msg),
        RGPU_ERR_UNEXPECTED_EOF => UnexpectedEOF(msg),
        RGPU_ERR_CORRUPT_INDEX => CorruptIndex(msg),
        RGPU_ERR_UNSUPPORTED => UnsupportedOperation(msg.into()),
        RGPU_ERR_IO => IOError(msg),
        _ => RuntimeError(msg),
    })
}

struct GpuLeaf {
    seg: *mut RgpuSegment, // rgpu_segment_upload_field of the leaf's .doc + norms + live docs, once per segment open
    has_positions: bool,   // .pos attached (rgpu_segment_attach_positions): PhraseQuery can be served
}

/// A filter that is not a term, as the query cache holds it: one doc set per leaf (by LeafReaderContext::ord), in HBM. What
/// CachingWrapperWeight::cache leaves for a leaf (search/cache/query_cache.rs:301-372) — made by `cache_filter_bits` from the cached
/// FixedBitSet words or by `cache_filter_query` on the GPU — and what `try_filtered` takes as FILTER / MUST_NOT sets. Keep it beside the
/// cache entry it mirrors (same key, same eviction); it is freed before the searcher that made it (doc sets go before their segments).
pub struct GpuCachedFilter {
    sets: Vec<*mut RgpuDocset>,
}

impl Drop for GpuCachedFilter {
    fn drop(&mut self) {
        for s in self.sets.drain(..) { unsafe { rgpu_docset_free(s) }; } // waits for the masked searches in flight that read the set
    }
}

/// What PointValues::intersect shows a visitor whose compare() always answers CellCrossesQuery: every (doc, packed value) of the field,
/// leaf by BKD leaf — the flat arrays rgpu_points_attach takes. One enumeration per leaf and field, at attach time.
struct AllPointsVisitor {
    docs: Vec<i32>,
    values: Vec<u8>,
}

impl IntersectVisitor for AllPointsVisitor {
    fn visit(&mut self, _doc_id: DocId) -> Result<()> {
        bail!(ErrorKind::IllegalState("visit() without a value: compare() never answers CellInsideQuery".into()))
    }
    fn visit_by_packed_value(&mut self, doc_id: DocId, packed_value: &[u8]) -> Result<()> {
        self.docs.push(doc_id);
        self.values.extend_from_slice(packed_value);
        Ok(())
    }
    fn compare(&self, _min_packed_value: &[u8], _max_packed_value: &[u8]) -> Relation {
        Relation::CellCrossesQuery
    }
}

/// The one-dimensional points of one field, resident in HBM: one rgpu_points per leaf (null: the leaf has no such field), made by
/// `attach_points`, read by `try_range_filter`. Freed before the searcher that made it (points go before their segments).
pub struct GpuPoints {
    field: String,
    bytes_per_dim: usize,
    per_leaf: Vec<*mut RgpuPoints>,
}

impl Drop for GpuPoints {
    fn drop(&mut self) {
        for p in self.per_leaf.drain(..) { if !p.is_null() { unsafe { rgpu_points_free(p) }; } }
    }
}

/// One flat clause list — what the C ABI takes (rgpu_query + rgpu_query_term[]): MUST / SHOULD first, then MUST_NOT.
struct FlatQuery<'q> {
    op: i32,
    positive: Vec<(&'q TermQuery, f32 /* boost, 0.0 for FILTER */)>,
    optional: Vec<&'q TermQuery>, // SHOULD beside MUST: ReqOptScorer
    optional_zero: bool,          // the optional clauses score 0.0 (a FILTER by a disjunction, "+a #(b c)": needs_scores = false)
    must_not: Vec<&'q TermQuery>,
}

impl<'q> FlatQuery<'q> {
    fn n_clauses(&self) -> usize { self.positive.len() + self.optional.len() + self.must_not.len() }
    fn clauses(&self) -> impl Iterator<Item = &'q TermQuery> + '_ {
        self.positive.iter().map(|(t, _)| *t).chain(self.optional.iter().cloned()).chain(self.must_not.iter().cloned())
    }
}

/// One group of a cross-field query (rgpu_field_group / rgpu_field_tree_group): a TermQuery, a DisjunctionMaxQuery of TermQuery
/// disjuncts in any fields or - `field_trees` - a nested should-only BooleanQuery of TermQuery clauses (`sum`, with its own
/// min_should_match `sum_msm`): what QueryStringQueryBuilder builds per word over several fields
struct CrossGroup<'q> {
    dismax: bool,
    tie: f32,
    terms: Vec<&'q TermQuery>,
    sum: bool,
    sum_msm: i32,
}
/// A BooleanQuery of all-SHOULD or all-MUST groups whose terms live in the uploaded field or in attached ones (rgpu_fields_query);
/// `field_trees`: `should_groups` beside MUST groups (ReqOptScorer) and sum groups (rgpu_fields_tree_query)
struct CrossQuery<'q> {
    must: bool,
    msm: i32,
    groups: Vec<CrossGroup<'q>>,
    should_groups: Vec<CrossGroup<'q>>,
    must_not: Vec<&'q TermQuery>,
}

impl<'q> CrossQuery<'q> {
    /// a tree rgpu_search_fields_batch cannot express: rgpu_search_fields_tree_batch's
    fn is_tree(&self) -> bool { !self.should_groups.is_empty() || self.groups.iter().any(|g| g.sum) }
}

pub struct GpuIndexSearcher<C: Codec, R: IndexReader<Codec = C> + ?Sized, IR: Deref<Target = R>, SP: SimilarityProducer<C>> {
    cpu: DefaultIndexSearcher<C, R, IR, SP>, // statistics (searcher.rs:306-363, :732-767) and the fallback for everything else
    ctx: *mut RgpuCtx,
    field: String,                            // the uploaded field: field 0 of every rgpu_segment (further fields: extra_fields)
    leaves: Vec<GpuLeaf>,                     // by LeafReaderContext::ord
    extra_fields: Vec<(String, Vec<i32>)>,    // attach_field: further fields of the same segments -> their slot per leaf (by ord)
    sim_tables: Mutex<HashMap<u32, i32>>,     // avgdl bits -> rgpu_sim_table_upload handle (k1, b fixed above)
    next_limit: i32,                          // DefaultIndexSearcher::next_limit (searcher.rs:285): None -> 0, Some(0) -> RGPU_NEXT_LIMIT_ZERO
    /// Fold ONE level of nested BooleanQuery into its parent (see flatten). Off by default, as in the C++ and Python mirrors
    /// (flatten_nested = false): the folded f32 sum is within 1e-5 of the CPU's, not bit-equal.
    allow_flatten: bool,
    /// try_filtered serves EXACT phrases — a PhraseQuery, a BooleanQuery over phrases — through rgpu_search_phrase_batch_masked,
    /// rgpu_search_phrase_bool_batch_masked and rgpu_search_phrase_or_batch_masked instead of leaving them to the CPU searcher. Off by
    /// default, as `filtered_phrases` of the Python and C++ mirrors. Still the CPU's with it on: any sloppy phrase under a mask (its
    /// next_limit counts deleted docs, not docs outside a filter), "\"a b\" c #F" (the doc set is the only required clause), a MUST_NOT
    /// set beside min_should_match >= 2, and whatever try_phrase_bool / try_phrase_or leave to it.
    pub filtered_phrases: bool,
    /// try_filtered serves queries whose ONLY required clauses are doc sets — "b c #F", a lone "#F" or range, "-X" — through
    /// rgpu_search_batch_required_set (try_required_set: every doc of live AND sets is collected, the docs no SHOULD clause holds at
    /// score 0, as the reference's ReqOptScorer(F, b | c) does), and "b c -X" masked. Off by default, as `required_sets` of the
    /// Python and C++ mirrors. Still the CPU's with it on: an exclusion beside min_should_match >= 2, MUST_NOT term clauses beside
    /// the sets, a SHOULD clause of boost <= 0, phrases and nested clauses on the SHOULD side.
    pub required_sets: bool,
    /// try_gpu serves a top-level SpanNearQuery(in_order = false) whose clauses are all SpanTermQuery through
    /// rgpu_search_span_unordered_batch (try_span_unordered: NearSpansUnordered with the heap's array order kept, bit-exact) instead of
    /// leaving it to the CPU searcher. Off by default, as `unordered_spans` of the Python and C++ mirrors. The CPU's either way:
    /// nested span clauses, SpanOrQuery and SpanGapQuery clauses, a span query inside a boolean, filtered, dismax, boosting or
    /// rescoring query (no tree this shim flattens holds one), and - in this shim - the ordered SpanNearQuery.
    pub unordered_spans: bool,
    /// try_gpu serves a BooleanQuery with required (MUST / FILTER) AND SHOULD clauses and exact PhraseQuery clauses on either side -
    /// +a +b "a b", +"a b" c, +"a b" +c "b c" d -n #f - through rgpu_search_phrase_opt_batch (try_phrase_opt: ReqOptScorer over the
    /// phrase scorers, its sequential rule kept, bit-exact) instead of leaving it to the CPU searcher. Off by default, as
    /// `optional_phrases` of the Python and C++ mirrors. The CPU's either way: a sloppy clause, a nested clause, a phrase under
    /// MUST_NOT, ten or more SHOULD clauses, more than RGPU_MAX_BOOL_PHRASES phrases on a side, and such a tree beside doc-set clauses.
    pub optional_phrases: bool,
    /// try_gpu serves the trees QueryStringQueryBuilder builds over several fields - every word a nested should-only BooleanQuery
    /// with one TermQuery per field, those groups under MUST and SHOULD by the `+` sign: "gpu +search" - through
    /// rgpu_search_fields_tree_batch (try_fields_tree: ReqOptScorer's sequential rule kept, bit-exact) instead of leaving them to the
    /// CPU searcher. Off by default, as `field_trees` of the Python and C++ mirrors; trees rgpu_search_fields_batch can express keep
    /// going to try_fields. Under the rule a query's hits are walked by ONE wavefront, about 7 ns per posting of its cheapest MUST
    /// group: a `+word` that millions of docs hold costs tens of milliseconds (rgpu_config.req_opt_rule = -1 adds the optional sums
    /// everywhere instead, in one pass). The CPU's either way: a nested clause that is not a should-only BooleanQuery of TermQuery
    /// clauses, a nested min_should_match >= 2, phrases, FILTER clauses, ten or more groups on a side, k > 128.
    pub field_trees: bool,
}

unsafe impl<C: Codec, R: IndexReader<Codec = C> + ?Sized, IR: Deref<Target = R>, SP: SimilarityProducer<C>> Send for GpuIndexSearcher<C, R, IR, SP> {}
unsafe impl<C: Codec, R: IndexReader<Codec = C> + ?Sized, IR: Deref<Target = R>, SP: SimilarityProducer<C>> Sync for GpuIndexSearcher<C, R, IR, SP> {}

impl<C: Codec, R: IndexReader<Codec = C> + ?Sized, IR: Deref<Target = R>, SP: SimilarityProducer<C>> GpuIndexSearcher<C, R, IR, SP> {
    /// `files(leaf)` hands over what SegmentReadState already names for the leaf: the mmapped `.doc` bytes, the field's norms as
    /// one byte per doc (or the `.nvm` / `.nvd` bytes through rgpu_norms_from_lucene53), the live-docs words
    /// (FixedBitSet::bits, util/bit_set.rs:117-124) and, for a positions field, the `.pos` bytes.
    pub fn open<F>(cpu: DefaultIndexSearcher<C, R, IR, SP>, device: i32, field: &str, index_options: i32, next_limit: Option<usize>, allow_flatten: bool,
                   files: F) -> Result<Self>
    where
        F: Fn(&LeafReaderContext<'_, C>) -> Result<(&[u8], Option<&[u8]>, Option<&[u64]>, Option<&[u8]>)>,
    {
        let mut ctx: *mut RgpuCtx = std::ptr::null_mut();
        check(unsafe { rgpu_init(device, std::ptr::null(), &mut ctx) }, std::ptr::null_mut())?;
        let mut leaves = Vec::new();
        for leaf in cpu.reader().leaves() {
            let (doc, norms, live, pos) = files(&leaf)?;
            let mut seg: *mut RgpuSegment = std::ptr::null_mut();
            check(
                unsafe {
                    rgpu_segment_upload_field(ctx, doc.as_ptr(), doc.len(), norms.map_or(std::ptr::null(), |n| n.as_ptr()), leaf.reader.max_doc(),
                                              leaf.doc_base, live.map_or(std::ptr::null(), |l| l.as_ptr()), index_options, &mut seg)
                },
                ctx,
            )?;
            if let Some(p) = pos {
                check(unsafe { rgpu_segment_attach_positions(seg, p.as_ptr(), p.len()) }, ctx)?;
            }
            leaves.push(GpuLeaf { seg, has_positions: pos.is_some() });
        }
        let next_limit = match next_limit { None => 0, Some(0) => RGPU_NEXT_LIMIT_ZERO, Some(n) => n.min(i32::max_value() as usize) as i32 };
        Ok(GpuIndexSearcher { cpu, ctx, field: field.to_string(), leaves, extra_fields: Vec::new(), sim_tables: Mutex::new(HashMap::new()), next_limit, allow_flatten, filtered_phrases: false, required_sets: false, unordered_spans: false, optional_phrases: false, field_trees: false })
    }

    /// A further indexed field of the same segments (rgpu_segment_attach_field): `norms(leaf)` hands over the field's norms as one
    /// byte per doc (None: the field omits them); `index_options` as for open(). Queries that name it - "title:gpu | body:gpu",
    /// "(title:a | body:a) (title:b | body:b)" - are then served by try_fields; every other path of this shim keeps reading the
    /// uploaded field alone (flatten's term_of drops any other field: those trees stay the CPU searcher's).
    pub fn attach_field<F>(&mut self, field: &str, index_options: i32, norms: F) -> Result<()>
    where
        F: Fn(&LeafReaderContext<'_, C>) -> Result<Option<&[u8]>>,
    {
        let mut slots = vec![0i32; self.leaves.len()];
        for leaf in self.cpu.reader().leaves() {
            let bytes = norms(&leaf)?;
            let mut slot: i32 = -1;
            check(unsafe { rgpu_segment_attach_field(self.leaves[leaf.ord].seg, bytes.map_or(std::ptr::null(), |n| n.as_ptr()), index_options, &mut slot) }, self.ctx)?;
            slots[leaf.ord] = slot;
        }
        self.extra_fields.push((field.to_string(), slots));
        Ok(())
    }

    /// The field slot of `field` in leaf `ord`: 0 for the uploaded field, an attached field's slot, None for any other field
    fn slot_of(&self, field: &str, ord: usize) -> Option<i32> {
        if field == self.field { return Some(0); }
        self.extra_fields.iter().find(|(name, _)| name == field).map(|(_, slots)| slots[ord])
    }

    /// Trees rgpu_search_fields_batch serves, when they name an attached field: a TermQuery, a DisjunctionMaxQuery of 1..=9 TermQuery
    /// disjuncts, a BooleanQuery of 1..=9 such clauses that are all MUST or all SHOULD, with MUST_NOT TermQuery clauses. None = not
    /// this call's: a tree over the uploaded field alone goes the way it went (flatten), FILTER clauses, MUST beside SHOULD
    /// (ReqOptScorer), ten or more groups or disjuncts (the heap-order arm), MUST_NOT beside min_should_match >= 2 and a field that
    /// is not attached stay the CPU searcher's. With `field_trees` a clause may also be a nested should-only BooleanQuery of 1..=9
    /// TermQuery clauses (min_should_match <= 1) and MUST clauses may stand beside SHOULD clauses, up to nine on a side.
    fn cross_spec<'q>(&self, query: &'q dyn Query<C>) -> Option<CrossQuery<'q>> {
        let known = |t: &TermQuery| self.slot_of(&t.term.field, 0).is_some();
        let group = |q: &'q dyn Query<C>| -> Option<CrossGroup<'q>> {
            if let Some(t) = q.as_any().downcast_ref::<TermQuery>() {
                return if known(t) { Some(CrossGroup { dismax: false, tie: 0.0, terms: vec![t], sum: false, sum_msm: 0 }) } else { None };
            }
            if let Some(n) = q.as_any().downcast_ref::<BooleanQuery<C>>() {   // (title:w body:w)
                if !self.field_trees { return None; }
                let (must, should, filter, must_not, msm) = n.clauses();
                if !must.is_empty() || !filter.is_empty() || !must_not.is_empty() || should.is_empty() { return None; }
                if should.len() > RGPU_MAX_GROUP_DISJUNCTS as usize || msm >= 2 { return None; }
                let mut terms = Vec::with_capacity(should.len());
                for c in should {
                    let t = c.as_any().downcast_ref::<TermQuery>()?;
                    if !known(t) { return None; }
                    terms.push(t);
                }
                return Some(CrossGroup { dismax: false, tie: 0.0, terms, sum: true, sum_msm: msm.max(0) });
            }
            let d = q.as_any().downcast_ref::<DisjunctionMaxQuery<C>>()?;
            if d.disjuncts.is_empty() || d.disjuncts.len() > RGPU_MAX_GROUP_DISJUNCTS as usize || !d.tie_breaker_multiplier.is_finite() { return None; }
            let mut terms = Vec::with_capacity(d.disjuncts.len());
            for c in &d.disjuncts {
                let t = c.as_any().downcast_ref::<TermQuery>()?;
                if !known(t) { return None; }
                terms.push(t);
            }
            Some(CrossGroup { dismax: true, tie: d.tie_breaker_multiplier, terms, sum: false, sum_msm: 0 })
        };
        let spec = if let Some(b) = query.as_any().downcast_ref::<BooleanQuery<C>>() {
            let (must, should, filter, must_not, msm) = b.clauses();
            let both = !must.is_empty() && !should.is_empty();
            if !filter.is_empty() || (both && !self.field_trees) || (must.is_empty() && should.is_empty()) { return None; }
            let positive = if must.is_empty() { should } else { must };
            if positive.len() > RGPU_MAX_FIELD_GROUPS as usize || (both && should.len() > RGPU_MAX_FIELD_GROUPS as usize) { return None; }
            let mut groups = Vec::with_capacity(positive.len());
            for q in positive { groups.push(group(q.as_ref())?); }
            let mut should_groups = Vec::new();
            if both { for q in should { should_groups.push(group(q.as_ref())?); } }
            let mut prohibited = Vec::with_capacity(must_not.len());
            for q in must_not {
                let t = q.as_any().downcast_ref::<TermQuery>()?;
                if !known(t) { return None; }
                prohibited.push(t);
            }
            if must.is_empty() && msm >= 2 && !prohibited.is_empty() { return None; }
            CrossQuery { must: !must.is_empty(), msm: if must.is_empty() { msm } else { 0 }, groups, should_groups, must_not: prohibited }
        } else {
            CrossQuery { must: false, msm: 0, groups: vec![group(query)?], should_groups: vec![], must_not: vec![] }
        };
        let n: usize = spec.groups.iter().chain(spec.should_groups.iter()).map(|g| g.terms.len()).sum::<usize>() + spec.must_not.len();
        if n > RGPU_MAX_FIELDS_QUERY_CLAUSES as usize { return None; }
        // a tree over the uploaded field alone is flatten's, as it has been
        let other = spec.groups.iter().chain(spec.should_groups.iter()).flat_map(|g| g.terms.iter()).chain(spec.must_not.iter())
            .any(|t| t.term.field != self.field);
        if other { Some(spec) } else { None }
    }

    /// weight = idf x boost of a clause and the norm cache of ITS field: collections_statistics(term.field), the searcher's
    /// term_statistics (df of the largest leaf), BM25Similarity::compute_weight - weight_of with the field taken from the term
    fn field_weight_of(&self, term: &Term, boost: f32) -> Result<(f32, i32)> {
        let coll: &CollectionStatistics = self.cpu.collections_statistics(&term.field).ok_or_else(|| Error::from(ErrorKind::IllegalState("no statistics".into())))?;
        let s: TermStatistics = self.cpu.term_statistics(term)?;
        let dfs = [s.doc_freq];
        let mut w = 0f32;
        check(unsafe { rgpu_bm25_compute_weight(BM25_K1, BM25_B, coll.max_doc, coll.doc_count, coll.sum_total_term_freq, dfs.as_ptr(), 1, boost,
                                                &mut w, std::ptr::null_mut(), std::ptr::null_mut()) }, self.ctx)?;
        Ok((w, self.sim_table(coll)?))
    }

    /// A cross-field tree through rgpu_search_fields_batch, one call per leaf: each clause carries its field's slot in that leaf,
    /// its own field's weight and norm cache; the library sums in the reference's order (clause order under SHOULD, the leaf's stable
    /// cost order under MUST) - bit-equal rows. k above 128 stays the CPU searcher's.
    fn try_fields(&self, spec: &CrossQuery<'_>, top: &mut TopDocsCollector, k: usize) -> Result<bool> {
        if k > 128 { return Ok(false); }
        let mut weights = Vec::new();
        for g in &spec.groups { for t in &g.terms { weights.push(self.field_weight_of(&t.term, t.boost)?); } }
        for leaf in self.cpu.reader().leaves() {
            let mut clauses: Vec<RgpuFieldClause> = Vec::with_capacity(weights.len() + spec.must_not.len());
            let mut groups: Vec<RgpuFieldGroup> = Vec::with_capacity(spec.groups.len());
            let mut at = 0usize;
            for g in &spec.groups {
                groups.push(RgpuFieldGroup { first_term: clauses.len() as i32, n_terms: g.terms.len() as i32, tie_bits: g.tie.to_bits(),
                                             kind: if g.dismax { RGPU_GROUP_DISMAX } else { RGPU_GROUP_TERM } });
                for t in &g.terms {
                    let slot = self.slot_of(&t.term.field, leaf.ord).unwrap_or(0);
                    clauses.push(RgpuFieldClause { state: Self::term_state(&self.block_state(&leaf, &t.term)?), weight: weights[at].0, sim_table: weights[at].1,
                                                   field: slot, reserved: 0 });
                    at += 1;
                }
            }
            let first_must_not = clauses.len() as i32;
            for t in &spec.must_not {
                let slot = self.slot_of(&t.term.field, leaf.ord).unwrap_or(0);
                clauses.push(RgpuFieldClause { state: Self::term_state(&self.block_state(&leaf, &t.term)?), weight: 0.0, sim_table: 0, field: slot, reserved: 0 });
            }
            let q = RgpuFieldsQuery { occur: if spec.must { RGPU_OCCUR_MUST } else { RGPU_OCCUR_SHOULD }, first_group: 0, n_groups: groups.len() as i32,
                                      min_should_match: spec.msm, first_must_not, n_must_not: spec.must_not.len() as i32 };
            let mut hits = vec![RgpuHit { doc: -1, score: 0.0 }; k];
            let mut total: i64 = 0;
            check(unsafe { rgpu_search_fields_batch(self.leaves[leaf.ord].seg, &q, 1, groups.as_ptr(), groups.len() as i32, clauses.as_ptr(), clauses.len() as i32,
                                                    k as i32, hits.as_mut_ptr(), &mut total) }, self.ctx)?;
            Self::hand_over(top, &hits, total);
        }
        Ok(true)
    }

    /// A cross-field tree with sum groups and / or SHOULD groups beside MUST groups (`field_trees`) through
    /// rgpu_search_fields_tree_batch, one call per leaf, as try_fields: the MUST groups first, then the SHOULD groups; the library
    /// sums the MUST side in the leaf's stable cost order, the SHOULD side in clause order, and applies ReqOptScorer's rule per leaf -
    /// bit-equal rows. k above 128 stays the CPU searcher's.
    fn try_fields_tree(&self, spec: &CrossQuery<'_>, top: &mut TopDocsCollector, k: usize) -> Result<bool> {
        if k > 128 { return Ok(false); }
        let mut weights = Vec::new();
        for g in spec.groups.iter().chain(spec.should_groups.iter()) { for t in &g.terms { weights.push(self.field_weight_of(&t.term, t.boost)?); } }
        for leaf in self.cpu.reader().leaves() {
            let mut clauses: Vec<RgpuFieldClause> = Vec::with_capacity(weights.len() + spec.must_not.len());
            let mut groups: Vec<RgpuFieldTreeGroup> = Vec::with_capacity(spec.groups.len() + spec.should_groups.len());
            let mut at = 0usize;
            for g in spec.groups.iter().chain(spec.should_groups.iter()) {
                groups.push(RgpuFieldTreeGroup { first_term: clauses.len() as i32, n_terms: g.terms.len() as i32, tie_bits: g.tie.to_bits(),
                                                 kind: if g.sum { RGPU_GROUP_SUM } else if g.dismax { RGPU_GROUP_DISMAX } else { RGPU_GROUP_TERM },
                                                 min_should_match: if g.sum { g.sum_msm } else { 0 }, reserved: 0 });
                for t in &g.terms {
                    let slot = self.slot_of(&t.term.field, leaf.ord).unwrap_or(0);
                    clauses.push(RgpuFieldClause { state: Self::term_state(&self.block_state(&leaf, &t.term)?), weight: weights[at].0, sim_table: weights[at].1,
                                                   field: slot, reserved: 0 });
                    at += 1;
                }
            }
            let first_must_not = clauses.len() as i32;
            for t in &spec.must_not {
                let slot = self.slot_of(&t.term.field, leaf.ord).unwrap_or(0);
                clauses.push(RgpuFieldClause { state: Self::term_state(&self.block_state(&leaf, &t.term)?), weight: 0.0, sim_table: 0, field: slot, reserved: 0 });
            }
            let (n_must, n_should) = if spec.must { (spec.groups.len(), spec.should_groups.len()) } else { (0, spec.groups.len()) };
            let q = RgpuFieldsTreeQuery { first_group: 0, n_must: n_must as i32, n_should: n_should as i32, min_should_match: spec.msm, first_must_not,
                                          n_must_not: spec.must_not.len() as i32 };
            let mut hits = vec![RgpuHit { doc: -1, score: 0.0 }; k];
            let mut total: i64 = 0;
            check(unsafe { rgpu_search_fields_tree_batch(self.leaves[leaf.ord].seg, &q, 1, groups.as_ptr(), groups.len() as i32, clauses.as_ptr(),
                                                         clauses.len() as i32, k as i32, hits.as_mut_ptr(), &mut total) }, self.ctx)?;
            Self::hand_over(top, &hits, total);
        }
        Ok(true)
    }

    /// BooleanQuery trees the C ABI serves, flattened to one clause list (query/boolean_query.rs:195-279 is what the CPU builds
    /// from the same tree). None = not ours: the caller falls back to DefaultIndexSearcher.
    ///   TermQuery                                   -> TERM
    ///   must / filter only                          -> AND (a FILTER clause is a MUST clause of weight 0: it scores 0.0)
    ///   should only                                 -> OR, RGPU_OP_OR_MSM(msm) when min_should_match > 1
    ///   must + should                               -> RGPU_OP_WITH_SHOULD(AND, n): ReqOptScorer, its sequential rule included
    ///   must + ONE nested should-only query         -> ... | RGPU_OP_SHOULD_REQUIRED | RGPU_OP_NESTED_AT(i) ("+a +(b c)": nested_must_child), bit-exact
    ///   must + ONE nested must-only query           -> ... | RGPU_OP_NESTED_MUST | RGPU_OP_NESTED_AT(i) ("+a +(+b +c)": the nested sum formed first), bit-exact
    ///   any of them + must_not                      -> n_must_not > 0: ReqNotScorer
    ///   a nested should-only MUST_NOT clause, a nested must-only FILTER clause -> their term clauses ("-(b c)" = "-b -c", "#(+b +c)" = "#b #c"), bit-exact
    ///   must / filter + ONE nested should-only FILTER clause -> ... | RGPU_OP_SHOULD_REQUIRED with zero-weight clauses ("+a #(b c)": filter_disjunction), bit-exact
    /// With `allow_flatten` (off by default): a MUST clause that is itself a must-only BooleanQuery, a SHOULD clause that is a
    /// should-only one (msm <= 1) with no other kind of clause inside it — ONE level is folded into the parent: same doc ids;
    /// the f32 sum is then formed over the flat list (a + b + c) where the CPU forms a + (b + c): within 1e-5 relative
    /// (north_star's float tolerance), not bit-equal. Two guards, as BooleanQuery.flattened() of the Python and C++ mirrors:
    /// the folded inner list must be non-empty (an inner query without clauses of the wanted kind is not a clause that can be
    /// dropped), and an outer min_should_match > 1 is never combined with a fold (SHOULD [a, (b OR c)] with msm = 2 needs `a`
    /// and one of b / c — OR_MSM(2) over {a, b, c} would also match b and c without a).
    fn flatten<'q>(&self, query: &'q dyn Query<C>) -> Option<FlatQuery<'q>> {
        if let Some(t) = query.as_any().downcast_ref::<TermQuery>() {
            if t.term.field != self.field { return None; }
            return Some(FlatQuery { op: RGPU_OP_TERM, positive: vec![(t, t.boost)], optional: vec![], optional_zero: false, must_not: vec![] });
        }
        let b = query.as_any().downcast_ref::<BooleanQuery<C>>()?;
        let (must, should, filter, must_not, msm) = b.clauses();
        let term_of = |q: &'q Box<dyn Query<C>>| q.as_any().downcast_ref::<TermQuery>().filter(|t| t.term.field == self.field);
        let mut positive = Vec::new();
        let mut optional = Vec::new();
        let mut prohibited = Vec::new();
        let mut folded = false;
        for q in must_not {
            if let Some(t) = term_of(q) { prohibited.push(t); continue; }
            // "-(b c)": a should-only BooleanQuery of terms as a MUST_NOT clause is the MUST_NOT clauses b, c — ReqNotScorer excludes
            // what the nested DisjunctionSumScorer matches (boolean_query.rs:236-273), nothing of it is ever scored: exact. The CPU puts
            // ONE disjunction with the OUTER min_should_match over the MUST_NOT scorers: expanded only while that is <= 1.
            let inner = q.as_any().downcast_ref::<BooleanQuery<C>>()?;
            let (m, s, f, n, inner_msm) = inner.clauses();
            if msm > 1 || !m.is_empty() || !f.is_empty() || !n.is_empty() || s.is_empty() || inner_msm > 1 { return None; }
            for c in s { prohibited.push(term_of(c)?); }
        }
        let allow = self.allow_flatten;
        let mut fold = |q: &'q Box<dyn Query<C>>, want_must: bool, out: &mut Vec<(&'q TermQuery, f32)>| -> Option<()> {
            if let Some(t) = term_of(q) { out.push((t, t.boost)); return Some(()); }
            if !allow { return None; }
            let inner = q.as_any().downcast_ref::<BooleanQuery<C>>()?;
            let (m, s, f, n, inner_msm) = inner.clauses();
            if !n.is_empty() || !f.is_empty() { return None; }
            let list = if want_must && s.is_empty() { m } else if !want_must && m.is_empty() && inner_msm <= 1 { s } else { return None };
            if list.is_empty() { return None; }
            for c in list { let t = term_of(c)?; out.push((t, t.boost)); }
            folded = true;
            Some(())
        };
        if !must.is_empty() || !filter.is_empty() {
            // "+a +(b c)" / "+a +(+b +c)": exactly ONE MUST clause that is a should-only BooleanQuery of 1..=9 term clauses (msm <= 1)
            // or a must-only one of >= 2, term clauses beside it, no SHOULD clause of the outer query ->
            // RGPU_OP_WITH_SHOULD(op, n) | RGPU_OP_SHOULD_REQUIRED / RGPU_OP_NESTED_MUST | RGPU_OP_NESTED_AT(its place): the CPU builds
            // ConjunctionScorer([TermScorer ..., nested scorer]) (boolean_query.rs:200-215); the library sorts those children by cost
            // per leaf as ConjunctionScorer::new does and adds the nested sum where score() adds it — bit-equal whatever the costs.
            if should.is_empty() && must.iter().filter(|q| term_of(q).is_none()).count() == 1 {
                if let Some(f) = self.nested_must_child(must, filter, &prohibited, false) { return Some(f); }
                if let Some(f) = self.nested_must_child(must, filter, &prohibited, true) { return Some(f); }
            }
            // "+a #(b c)": ONE FILTER clause that is a should-only BooleanQuery of 1..=9 term clauses (msm <= 1), term clauses everywhere else
            if should.is_empty() && must.iter().all(|q| term_of(q).is_some()) && filter.iter().filter(|q| term_of(q).is_none()).count() == 1 {
                if let Some(f) = self.filter_disjunction(must, filter, &prohibited) { return Some(f); }
            }
            for q in must { fold(q, true, &mut positive)?; }
            for q in filter { self.filter_terms(q, &mut positive)?; }
            for q in should { optional.push(term_of(q)?); }
            let op = if positive.len() == 1 { RGPU_OP_TERM } else { RGPU_OP_AND };
            Some(FlatQuery { op: rgpu_op_with_should(op, optional.len() as i32), positive, optional, optional_zero: false, must_not: prohibited })
        } else {
            // "a (b c) d": a nested should-only query (msm <= 1) as FIRST or SECOND clause -> the flat disjunction [b, c, a, d], bit-equal:
            // DisjunctionSumScorer adds its children in clause order from 0.0 (SimpleQueue below ten children, disjunction_scorer.rs:
            // 211-225), (a + (b + c)) + d, and the flat query's ((b + c) + a) + d differs in one two-operand add, which commutes.
            if msm <= 1 && should.iter().filter(|q| term_of(q).is_none()).count() == 1 {
                let at = should.iter().position(|q| term_of(q).is_none())?;
                if let Some(inner) = should[at].as_any().downcast_ref::<BooleanQuery<C>>() {
                    let (m, s, f, n, inner_msm) = inner.clauses();
                    if at <= 1 && m.is_empty() && f.is_empty() && n.is_empty() && inner_msm <= 1 && !s.is_empty() && s.len() + should.len() - 1 < 10 {
                        let mut exact = Vec::new();
                        for c in s { let t = term_of(c)?; exact.push((t, t.boost)); }
                        for (i, q) in should.iter().enumerate() { if i != at { let t = term_of(q)?; exact.push((t, t.boost)); } }
                        return Some(FlatQuery { op: RGPU_OP_OR, positive: exact, optional: vec![], optional_zero: false, must_not: prohibited });
                    }
                }
            }
            for q in should { fold(q, false, &mut positive)?; }
            if msm > 1 && folded { return None; }
            let op = if msm > 1 { rgpu_op_or_msm(msm) } else { RGPU_OP_OR };
            Some(FlatQuery { op, positive, optional, optional_zero: false, must_not: prohibited })
        }
    }

    /// "+a #(b c)" — a filter by a disjunction ("category is b or c") is the required disjunction "+a +(b c)" whose clauses score 0.0: the
    /// CPU builds ConjunctionScorer([TermScorer(a) ..., DisjunctionSumScorer(b, c)]) with the nested weights created with needs_scores =
    /// false (boolean_query.rs:101-108, 200-215); its 0.0 + 0.0 leaves the f32 sum of the scoring clauses as it is wherever the cost order
    /// adds it. RGPU_OP_SHOULD_REQUIRED with zero-weight optional clauses, behind the MUST clauses (RGPU_OP_NESTED_AT(must.len())).
    fn filter_disjunction<'q>(&self, must: &'q [Box<dyn Query<C>>], filter: &'q [Box<dyn Query<C>>], prohibited: &[&'q TermQuery]) -> Option<FlatQuery<'q>> {
        let term_of = |q: &'q Box<dyn Query<C>>| q.as_any().downcast_ref::<TermQuery>().filter(|t| t.term.field == self.field);
        let mut positive = Vec::new();
        let mut optional = Vec::new();
        for q in must { let t = term_of(q)?; positive.push((t, t.boost)); }
        for q in filter {
            if let Some(t) = term_of(q) { positive.push((t, 0.0)); continue; }
            let inner = q.as_any().downcast_ref::<BooleanQuery<C>>()?;
            let (m, s, f, n, inner_msm) = inner.clauses();
            if !m.is_empty() || !f.is_empty() || !n.is_empty() || inner_msm > 1 || s.is_empty() || s.len() > 9 { return None; }
            for c in s { optional.push(term_of(c)?); }
        }
        if positive.is_empty() || optional.is_empty() { return None; }
        let op = if positive.len() == 1 { RGPU_OP_TERM } else { RGPU_OP_AND };
        Some(FlatQuery { op: rgpu_op_with_should(op, optional.len() as i32) | RGPU_OP_SHOULD_REQUIRED | rgpu_op_nested_at(must.len() as i32), positive, optional,
                         optional_zero: true, must_not: prohibited.to_vec() })
    }

    /// A FILTER clause as MUST clauses of weight 0: a term, or "#(+b +c)" — a must- / filter-only BooleanQuery of terms, whose weights the
    /// CPU creates with needs_scores = false (boolean_query.rs:106-108): every clause scores 0.0, the nested conjunction's 0.0 + 0.0
    /// joins the outer sum as one 0.0, and x + 0.0 == x wherever the cost order puts the clauses — the FILTER clauses b, c, exact.
    fn filter_terms<'q>(&self, q: &'q Box<dyn Query<C>>, out: &mut Vec<(&'q TermQuery, f32)>) -> Option<()> {
        let term_of = |q: &'q Box<dyn Query<C>>| q.as_any().downcast_ref::<TermQuery>().filter(|t| t.term.field == self.field);
        if let Some(t) = term_of(q) { out.push((t, 0.0)); return Some(()); }
        let inner = q.as_any().downcast_ref::<BooleanQuery<C>>()?;
        let (m, s, f, n, _) = inner.clauses();
        if !s.is_empty() || !n.is_empty() || (m.is_empty() && f.is_empty()) { return None; }
        for c in m.iter().chain(f.iter()) { out.push((term_of(c)?, 0.0)); }
        Some(())
    }

    /// The one nested MUST clause of "+a +(b c)" (conjunction = false: a should-only BooleanQuery of 1..=9 terms, msm <= 1) or
    /// "+a +(+b +c)" (conjunction = true: a must-only one of >= 2 terms) with the term clauses beside it, as the C ABI takes them.
    fn nested_must_child<'q>(&self, must: &'q [Box<dyn Query<C>>], filter: &'q [Box<dyn Query<C>>], prohibited: &[&'q TermQuery], conjunction: bool)
                             -> Option<FlatQuery<'q>> {
        let term_of = |q: &'q Box<dyn Query<C>>| q.as_any().downcast_ref::<TermQuery>().filter(|t| t.term.field == self.field);
        let mut positive = Vec::new();
        let mut optional = Vec::new();
        let mut at = 0i32;
        for q in must {
            if let Some(t) = term_of(q) { positive.push((t, t.boost)); continue; }
            let inner = q.as_any().downcast_ref::<BooleanQuery<C>>()?;
            at = positive.len() as i32; // the nested clause's place among the MUST clauses (FILTER clauses follow them: boolean_query.rs:101-108)
            let (m, s, f, n, inner_msm) = inner.clauses();
            if !f.is_empty() || !n.is_empty() { return None; }
            if conjunction {
                if !s.is_empty() || m.len() < 2 { return None; }
                for c in m { optional.push(term_of(c)?); }
            } else {
                if !m.is_empty() || inner_msm > 1 || s.is_empty() || s.len() > 9 { return None; }
                for c in s { optional.push(term_of(c)?); }
            }
        }
        for q in filter { self.filter_terms(q, &mut positive)?; }
        if positive.is_empty() || optional.is_empty() { return None; }
        let op = if positive.len() == 1 { RGPU_OP_TERM } else { RGPU_OP_AND };
        let flag = if conjunction { RGPU_OP_NESTED_MUST } else { RGPU_OP_SHOULD_REQUIRED };
        Some(FlatQuery { op: rgpu_op_with_should(op, optional.len() as i32) | flag | rgpu_op_nested_at(at), positive, optional, optional_zero: false, must_not: prohibited.to_vec() })
    }

    /// The 256-entry norm cache of the field's statistics, uploaded once per avgdl (bm25_similarity.rs:160-166)
    fn sim_table(&self, coll: &CollectionStatistics) -> Result<i32> {
        let mut cache = [0f32; 256];
        let df = [1i64];
        check(unsafe { rgpu_bm25_compute_weight(BM25_K1, BM25_B, coll.max_doc, coll.doc_count, coll.sum_total_term_freq, df.as_ptr(), 1, 1.0,
                                                std::ptr::null_mut(), std::ptr::null_mut(), cache.as_mut_ptr()) }, self.ctx)?;
        let key = cache[255].to_bits() ^ cache[1].to_bits().rotate_left(16); // the cache is a function of avgdl alone
        let mut tables = self.sim_tables.lock().unwrap();
        if let Some(h) = tables.get(&key) { return Ok(*h); }
        let h = unsafe { rgpu_sim_table_upload(self.ctx, cache.as_ptr(), BM25_K1) };
        check(h, self.ctx)?;
        tables.insert(key, h);
        Ok(h)
    }

    /// weight = idf x boost of a clause (or of a phrase: idf summed over its terms) exactly as TermQuery::create_weight /
    /// PhraseQuery::create_weight (term_query.rs:58-95, phrase_query.rs:136-186): the searcher's term_statistics — df of the
    /// LARGEST leaf, searcher.rs:732-767 —, collections_statistics(field), BM25Similarity::compute_weight.
    fn weight_of(&self, terms: &[&Term], boost: f32) -> Result<(f32, i32)> {
        let coll: &CollectionStatistics = self.cpu.collections_statistics(&self.field).ok_or_else(|| Error::from(ErrorKind::IllegalState("no statistics".into())))?;
        let mut dfs = Vec::with_capacity(terms.len());
        for t in terms { let s: TermStatistics = self.cpu.term_statistics(t)?; dfs.push(s.doc_freq); }
        let mut w = 0f32;
        check(unsafe { rgpu_bm25_compute_weight(BM25_K1, BM25_B, coll.max_doc, coll.doc_count, coll.sum_total_term_freq, dfs.as_ptr(), dfs.len() as i32, boost,
                                                &mut w, std::ptr::null_mut(), std::ptr::null_mut()) }, self.ctx)?;
        Ok((w, self.sim_table(coll)?))
    }

    /// BlockTermState of `term` in `leaf` (None: absent; TermWeight::create_scorer -> None)
    fn block_state(&self, leaf: &LeafReaderContext<'_, C>, term: &Term) -> Result<Option<BlockTermState>> {
        let terms = match leaf.reader.terms(&term.field)? { Some(t) => t, None => return Ok(None) };
        let mut it = terms.iterator()?;
        if !it.seek_exact(&term.bytes)? { return Ok(None); }
        Ok(Some(it.term_state()?)) // blocktree_reader.rs:1779-1808 -> posting_reader.rs:264-306
    }

    fn term_state(st: &Option<BlockTermState>) -> RgpuTermState {
        match st {
            None => RgpuTermState { doc_start_fp: 0, skip_offset: -1, total_term_freq: 0, doc_freq: 0, singleton_doc_id: -1 },
            Some(st) => RgpuTermState { doc_start_fp: st.doc_start_fp, skip_offset: st.skip_offset, total_term_freq: st.total_term_freq, doc_freq: st.doc_freq,
                                        singleton_doc_id: st.singleton_doc_id },
        }
    }

    fn hand_over(top: &mut TopDocsCollector, hits: &[RgpuHit], total: i64) {
        let rows: Vec<(DocId, f32)> = hits.iter().filter(|h| h.doc >= 0).map(|h| (h.doc, h.score)).collect(); // doc + doc_base already
        top.add_leaf_result(&rows, total as usize);
    }

    /// Every clause's (weight, sim table) in the ABI's clause order
    fn clause_weights(&self, flat: &FlatQuery<'_>) -> Result<Vec<(f32, i32)>> {
        let mut weights = Vec::with_capacity(flat.n_clauses());
        for (t, boost) in &flat.positive { weights.push(if *boost == 0.0 { (0.0, 0) } else { self.weight_of(&[&t.term], *boost)? }); }
        for t in &flat.optional { weights.push(if flat.optional_zero { (0.0, 0) } else { self.weight_of(&[&t.term], t.boost)? }); }
        for _ in &flat.must_not { weights.push((0.0, 0)); } // needs_scores = false: never read
        Ok(weights)
    }

    fn try_gpu(&self, query: &dyn Query<C>, top: &mut TopDocsCollector, k: usize) -> Result<bool> {
        if k == 0 || k > RGPU_MAX_K as usize { return Ok(false); }
        if let Some(p) = query.as_any().downcast_ref::<PhraseQuery>() { return self.try_phrase(p, None, top, k); }
        if let Some(n) = query.as_any().downcast_ref::<SpanNearQuery>() {
            return if self.unordered_spans { self.try_span_unordered(n, top, k) } else { Ok(false) };
        }
        if let Some(b) = query.as_any().downcast_ref::<BooleanQuery<C>>() {
            let (must, should, filter, must_not, _) = b.clauses();
            if must.iter().chain(should).chain(filter).chain(must_not).any(|q| q.as_any().downcast_ref::<PhraseQuery>().is_some()) {
                // no MUST and no FILTER clause: one DisjunctionSumScorer over the SHOULD clauses; else the conjunction's rules decide
                if must.is_empty() && filter.is_empty() { return self.try_phrase_or(b, None, top, k); }
                if !should.is_empty() && self.optional_phrases { return self.try_phrase_opt(b, top, k); }
                return self.try_phrase_bool(b, None, top, k);
            }
        }
        if !self.extra_fields.is_empty() {   // a tree that names an attached field: rgpu_search_fields_batch
            if let Some(spec) = self.cross_spec(query) {
                return if spec.is_tree() { self.try_fields_tree(&spec, top, k) } else { self.try_fields(&spec, top, k) };   // (a tree only with field_trees)
            }
        }
        let flat = match self.flatten(query) { Some(f) => f, None => return Ok(false) };
        let n = flat.n_clauses();
        if n > RGPU_MAX_QUERY_TERMS as usize { return Ok(false); }
        let weights = self.clause_weights(&flat)?;
        for leaf in self.cpu.reader().leaves() {
            let mut terms = Vec::with_capacity(n);
            for (i, t) in flat.clauses().enumerate() {
                terms.push(RgpuQueryTerm { state: Self::term_state(&self.block_state(&leaf, &t.term)?), weight: weights[i].0, sim_table: weights[i].1 });
            }
            let q = RgpuQuery { op: flat.op, n_terms: flat.positive.len() as i32, first_term: 0, n_must_not: flat.must_not.len() as i32 };
            let mut hits = vec![RgpuHit { doc: -1, score: 0.0 }; k];
            let mut total: i64 = 0;
            check(unsafe { rgpu_search_batch(self.leaves[leaf.ord].seg, &q, 1, terms.as_ptr(), n as i32, k as i32, hits.as_mut_ptr(), &mut total) }, self.ctx)?;
            Self::hand_over(top, &hits, total);
        }
        Ok(true)
    }

    /// The live docs `query` matches, summed over the leaves (TotalHitCountCollector, searcher.rs:650-653); None: not a tree of term
    /// clauses `flatten` accepts. The clause weights are computed as for a search - the library ignores them, but a conjunction runs
    /// the search's conjunction kernel, which wants the similarity table uploaded.
    fn try_count(&self, query: &dyn Query<C>) -> Result<Option<i32>> {
        let flat = match self.flatten(query) { Some(f) => f, None => return Ok(None) };
        let n = flat.n_clauses();
        if n > RGPU_MAX_QUERY_TERMS as usize { return Ok(None); }
        let weights = self.clause_weights(&flat)?;
        let mut sum: i64 = 0;
        for leaf in self.cpu.reader().leaves() {
            let mut terms = Vec::with_capacity(n);
            for (i, t) in flat.clauses().enumerate() {
                terms.push(RgpuQueryTerm { state: Self::term_state(&self.block_state(&leaf, &t.term)?), weight: weights[i].0, sim_table: weights[i].1 });
            }
            let q = RgpuQuery { op: flat.op, n_terms: flat.positive.len() as i32, first_term: 0, n_must_not: flat.must_not.len() as i32 };
            let mut count: i64 = 0;
            check(unsafe { rgpu_count_batch(self.leaves[leaf.ord].seg, std::ptr::null_mut(), &q, 1, terms.as_ptr(), n as i32, &mut count) }, self.ctx)?;
            sum += count;
        }
        Ok(Some(sum as i32))
    }

    /// The phrase's terms in one leaf, in the query's order: postings + position-stream pointers (a term absent from the leaf:
    /// doc_freq = 0, which tells the library what PhraseWeight::create_scorer -> None tells the reference)
    fn phrase_terms(&self, leaf: &LeafReaderContext<'_, C>, terms: &[Term], positions: &[i32]) -> Result<Vec<RgpuPhraseTerm>> {
        let mut pterms = Vec::with_capacity(terms.len());
        for (t, pos) in terms.iter().zip(positions.iter()) {
            let st = self.block_state(leaf, t)?;
            let ptrs = match &st {
                Some(s) => RgpuTermPositions { pos_start_fp: s.pos_start_fp, pay_start_fp: s.pay_start_fp, last_pos_block_offset: s.last_pos_block_offset },
                None => RgpuTermPositions { pos_start_fp: 0, pay_start_fp: 0, last_pos_block_offset: -1 },
            };
            pterms.push(RgpuPhraseTerm { state: Self::term_state(&st), positions: ptrs, position: *pos, reserved: 0 });
        }
        Ok(pterms)
    }

    /// QueryRescorer::rescore (rescorer.rs:376-390) of one first-pass row with a PhraseQuery as the second query: `row` is the
    /// first pass's (doc, score) list, best first, at most RGPU_MAX_K long; on Ok(true) it holds the rescored row —
    /// iterative_rescore (:229-298) with an Exact- / SloppyPhraseScorer advanced from hit to hit, combine_score, the window sorted
    /// (score desc, doc asc), the tail re-weighted (combine_docs). mode: RescoreMode's ordinal (0 Avg .. 4 Multiply). One
    /// rgpu_rescore_phrase_batch per leaf, the last one finishing. window_size is RescoreRequest::window_size as the reference
    /// means it: the number of leading hits that are rescored, 0 = none (every hit only takes query_weight); it is clipped to the
    /// row's length (the C++ host mirror's "0 = the whole row" is that mirror's own shorthand). Ok(false): not served here — another field, a leaf without
    /// positions, a sloppy phrase that names a term twice (its repetition groups depend on a doc that is no hit) — and `row` is
    /// untouched: the caller runs QueryRescorer on the CPU searcher.
    pub fn rescore_phrase(&self, p: &PhraseQuery, query_weight: f32, rescore_weight: f32, mode: i32, window_size: usize,
                          row: &mut Vec<(DocId, f32)>) -> Result<bool> {
        let (field, terms, positions, slop) = p.parts();
        let k = row.len();
        if field != self.field || terms.len() < 2 || terms.len() > RGPU_MAX_PHRASE_TERMS as usize || terms.len() != positions.len()
            || k == 0 || k > RGPU_MAX_K as usize || self.leaves.iter().any(|l| !l.has_positions) {
            return Ok(false);
        }
        if slop > 0 && terms.iter().enumerate().any(|(i, t)| terms[..i].iter().any(|u| u.bytes == t.bytes)) { return Ok(false); }
        let term_refs: Vec<&Term> = terms.iter().collect();
        let (weight, sim_table) = self.weight_of(&term_refs, 1.0)?;
        let req = RgpuRescoreRequest { query_weight, rescore_weight, mode, window_size: window_size.min(k) as i32 };
        let mut hits: Vec<RgpuHit> = row.iter().map(|&(doc, score)| RgpuHit { doc, score }).collect();
        let leaves = self.cpu.reader().leaves();
        let n_leaves = leaves.len();
        for (i, leaf) in leaves.into_iter().enumerate() {
            let pterms = self.phrase_terms(&leaf, terms, positions)?;
            let q = RgpuPhraseQuery { n_terms: pterms.len() as i32, first_term: 0, weight, sim_table, slop, next_limit: self.next_limit };
            check(unsafe { rgpu_rescore_phrase_batch(self.leaves[leaf.ord].seg, &q, 1, pterms.as_ptr(), pterms.len() as i32, &req, k as i32,
                                                     hits.as_mut_ptr(), if i + 1 == n_leaves { 1 } else { 0 }) }, self.ctx)?;
        }
        row.clear();
        row.extend(hits.iter().filter(|h| h.doc >= 0).map(|h| (h.doc, h.score)));
        Ok(true)
    }

    /// PhraseQuery { any slop } on a positions field (payloads / offsets included): terms + phrase offsets from the query,
    /// weight = summed idf x boost as PhraseQuery::create_weight (phrase_query.rs:136-186; its boost is 1.0). Per leaf as
    /// PhraseWeight::create_scorer (:268-333): a term absent from the leaf -> no scorer for that leaf (doc_freq = 0 tells the
    /// library the same); slop 0 -> ExactPhraseScorer, slop > 0 -> SloppyPhraseScorer under the searcher's next_limit.
    /// `masks` (try_filtered: one doc set per leaf, by LeafReaderContext::ord): the search restricted to them, exact phrases only.
    fn try_phrase(&self, p: &PhraseQuery, masks: Option<&[*mut RgpuDocset]>, top: &mut TopDocsCollector, k: usize) -> Result<bool> {
        let (field, terms, positions, slop) = p.parts();
        if field != self.field || terms.len() < 2 || terms.len() > RGPU_MAX_PHRASE_TERMS as usize || terms.len() != positions.len()
            || self.leaves.iter().any(|l| !l.has_positions) || (masks.is_some() && slop != 0) {
            return Ok(false);
        }
        let term_refs: Vec<&Term> = terms.iter().collect();
        let (weight, sim_table) = self.weight_of(&term_refs, 1.0)?;
        for leaf in self.cpu.reader().leaves() {
            let pterms = self.phrase_terms(&leaf, terms, positions)?;
            let q = RgpuPhraseQuery { n_terms: pterms.len() as i32, first_term: 0, weight, sim_table, slop, next_limit: self.next_limit };
            let mut hits = vec![RgpuHit { doc: -1, score: 0.0 }; k];
            let mut total: i64 = 0;
            let seg = self.leaves[leaf.ord].seg;
            check(unsafe {
                match masks {
                    Some(m) => rgpu_search_phrase_batch_masked(seg, m[leaf.ord], &q, 1, pterms.as_ptr(), pterms.len() as i32, k as i32, hits.as_mut_ptr(), &mut total),
                    None => rgpu_search_phrase_batch(seg, &q, 1, pterms.as_ptr(), pterms.len() as i32, k as i32, hits.as_mut_ptr(), &mut total),
                }
            }, self.ctx)?;
            Self::hand_over(top, &hits, total);
        }
        Ok(true)
    }

    /// SpanNearQuery { in_order: false } over SpanTermQuery clauses (`unordered_spans`): NearSpansUnordered (span_near.rs:333-528) +
    /// SpanScorer (span.rs:489-519) -> rgpu_search_span_unordered_batch per leaf. The row is packed exactly as an ordered one: clause
    /// i is phrase term i at position i, `slop` the allowed slop; weight = idf summed over every clause's term, a term named by two
    /// clauses counted twice (build_sim_weight over extract_term_keys, span.rs:574-602), boost 1.0. Per leaf as
    /// SpanNearWeight::get_spans: a clause whose term the leaf lacks -> no spans for that leaf (doc_freq = 0 tells the library the
    /// same). The searcher's next_limit applies at every slop: spans are always two-phase. Ok(false) - the CPU searcher - for an
    /// ordered query, another field, a clause that is not a SpanTermQuery (nested near, SpanOrQuery, SpanGapQuery, SpanBoostQuery),
    /// more than RGPU_MAX_PHRASE_TERMS clauses, a negative slop, a clause that carries a KeyedContext (its idf is not the
    /// statistics'), a leaf without positions.
    fn try_span_unordered(&self, n: &SpanNearQuery, top: &mut TopDocsCollector, k: usize) -> Result<bool> {
        let (field, clauses, slop, in_order) = n.parts();
        if in_order || field != self.field || clauses.len() < 2 || clauses.len() > RGPU_MAX_PHRASE_TERMS as usize || slop < 0
            || self.leaves.iter().any(|l| !l.has_positions) {
            return Ok(false);
        }
        let mut terms: Vec<Term> = Vec::with_capacity(clauses.len());
        for c in clauses {
            match c {
                SpanQueryEnum::Term(t) if t.ctx.is_none() => terms.push(t.term.clone()),
                _ => return Ok(false),
            }
        }
        let positions: Vec<i32> = (0..terms.len() as i32).collect();
        let term_refs: Vec<&Term> = terms.iter().collect();
        let (weight, sim_table) = self.weight_of(&term_refs, 1.0)?;
        for leaf in self.cpu.reader().leaves() {
            let pterms = self.phrase_terms(&leaf, &terms, &positions)?;
            let q = RgpuPhraseQuery { n_terms: pterms.len() as i32, first_term: 0, weight, sim_table, slop, next_limit: self.next_limit };
            let mut hits = vec![RgpuHit { doc: -1, score: 0.0 }; k];
            let mut total: i64 = 0;
            check(unsafe {
                rgpu_search_span_unordered_batch(self.leaves[leaf.ord].seg, &q, 1, pterms.as_ptr(), pterms.len() as i32, k as i32, hits.as_mut_ptr(), &mut total)
            }, self.ctx)?;
            Self::hand_over(top, &hits, total);
        }
        Ok(true)
    }

    /// BooleanQuery whose MUST / FILTER clauses hold 1..=RGPU_MAX_BOOL_PHRASES exact PhraseQuery clauses beside TermQuery clauses, with
    /// MUST_NOT TermQuery clauses: "+\"a b\" +c -d #e" -> rgpu_search_phrase_bool_batch per leaf. phrase_slot = the phrase's index in
    /// BooleanWeight::must_weights (MUST clauses in query order, then FILTER clauses, boolean_query.rs:96-125); a FILTER clause rides
    /// with weight 0 (needs_scores = false). The library sorts the children by cost per leaf and sums in that order, as
    /// ConjunctionScorer does. Ok(false) — the CPU searcher — under try_phrase's rules (another field, a leaf without positions, a
    /// phrase of the wrong size) and for every shape the library does not serve: a sloppy phrase clause (inside a conjunction the CPU
    /// matches it on its approximation and scores a stale sloppy_freq), a phrase under SHOULD or MUST_NOT, a SHOULD clause or a
    /// nested BooleanQuery beside a phrase, more than RGPU_MAX_BOOL_PHRASES phrases, more than RGPU_MAX_QUERY_TERMS clause terms.
    /// `masks` as for try_phrase: rgpu_search_phrase_bool_batch_masked.
    fn try_phrase_bool(&self, b: &BooleanQuery<C>, masks: Option<&[*mut RgpuDocset]>, top: &mut TopDocsCollector, k: usize) -> Result<bool> {
        let (must, should, filter, must_not, _) = b.clauses();
        if !should.is_empty() || self.leaves.iter().any(|l| !l.has_positions) { return Ok(false); }
        let term_of = |q: &Box<dyn Query<C>>| q.as_any().downcast_ref::<TermQuery>().filter(|t| t.term.field == self.field);
        let mut phrases: Vec<(&PhraseQuery, usize, bool)> = Vec::new(); // (the phrase, its slot in must_weights, under FILTER)
        let mut required: Vec<(&TermQuery, bool)> = Vec::new();
        for (slot, q) in must.iter().chain(filter.iter()).enumerate() {
            let filtering = slot >= must.len();
            if let Some(p) = q.as_any().downcast_ref::<PhraseQuery>() {
                let (field, terms, positions, slop) = p.parts();
                if field != self.field || slop != 0 || terms.len() < 2 || terms.len() > RGPU_MAX_PHRASE_TERMS as usize || terms.len() != positions.len() {
                    return Ok(false);
                }
                phrases.push((p, slot, filtering));
            } else if let Some(t) = term_of(q) {
                required.push((t, filtering));
            } else {
                return Ok(false);
            }
        }
        if phrases.is_empty() || phrases.len() > RGPU_MAX_BOOL_PHRASES as usize { return Ok(false); }
        let mut prohibited: Vec<&TermQuery> = Vec::with_capacity(must_not.len());
        for q in must_not {
            match term_of(q) { Some(t) => prohibited.push(t), None => return Ok(false) }
        }
        let n_phrase_terms: usize = phrases.iter().map(|(p, _, _)| p.parts().1.len()).sum();
        if n_phrase_terms + required.len() + prohibited.len() > RGPU_MAX_QUERY_TERMS as usize { return Ok(false); }
        let mut phrase_weights = Vec::with_capacity(phrases.len());
        for (p, _, filtering) in &phrases {
            let term_refs: Vec<&Term> = p.parts().1.iter().collect();
            let (weight, sim_table) = self.weight_of(&term_refs, 1.0)?;
            phrase_weights.push((if *filtering { 0.0 } else { weight }, sim_table));
        }
        let mut term_weights = Vec::with_capacity(required.len());
        for (t, filtering) in &required {
            let (weight, sim_table) = self.weight_of(&[&t.term], t.boost)?;
            term_weights.push((if *filtering { 0.0 } else { weight }, sim_table));
        }
        let mut bq = RgpuPhraseBoolQuery { n_phrases: phrases.len() as i32, first_phrase: 0, n_terms: required.len() as i32, first_term: 0,
                                           n_must_not: prohibited.len() as i32, phrase_slot: [0; 4], reserved: [0; 3] };
        for (i, (_, slot, _)) in phrases.iter().enumerate() { bq.phrase_slot[i] = *slot as i32; }
        for leaf in self.cpu.reader().leaves() {
            let mut pqs = Vec::with_capacity(phrases.len());
            let mut pterms: Vec<RgpuPhraseTerm> = Vec::with_capacity(n_phrase_terms);
            for (i, (p, _, _)) in phrases.iter().enumerate() {
                let (_, terms, positions, _) = p.parts();
                let mine = self.phrase_terms(&leaf, terms, positions)?;
                pqs.push(RgpuPhraseQuery { n_terms: mine.len() as i32, first_term: pterms.len() as i32, weight: phrase_weights[i].0, sim_table: phrase_weights[i].1,
                                           slop: 0, next_limit: 0 });
                pterms.extend(mine);
            }
            let mut terms = Vec::with_capacity(required.len() + prohibited.len());
            for (i, (t, _)) in required.iter().enumerate() {
                terms.push(RgpuQueryTerm { state: Self::term_state(&self.block_state(&leaf, &t.term)?), weight: term_weights[i].0, sim_table: term_weights[i].1 });
            }
            for t in &prohibited {
                terms.push(RgpuQueryTerm { state: Self::term_state(&self.block_state(&leaf, &t.term)?), weight: 0.0, sim_table: 0 }); // never scored
            }
            let mut hits = vec![RgpuHit { doc: -1, score: 0.0 }; k];
            let mut total: i64 = 0;
            let seg = self.leaves[leaf.ord].seg;
            let terms_ptr = if terms.is_empty() { std::ptr::null() } else { terms.as_ptr() };
            check(unsafe {
                match masks {
                    Some(m) => rgpu_search_phrase_bool_batch_masked(seg, m[leaf.ord], &bq, 1, pqs.as_ptr(), pqs.len() as i32, pterms.as_ptr(), pterms.len() as i32,
                                                                    terms_ptr, terms.len() as i32, k as i32, hits.as_mut_ptr(), &mut total),
                    None => rgpu_search_phrase_bool_batch(seg, &bq, 1, pqs.as_ptr(), pqs.len() as i32, pterms.as_ptr(), pterms.len() as i32,
                                                          terms_ptr, terms.len() as i32, k as i32, hits.as_mut_ptr(), &mut total),
                }
            }, self.ctx)?;
            Self::hand_over(top, &hits, total);
        }
        Ok(true)
    }

    /// BooleanQuery without MUST and FILTER clauses whose 1..=9 SHOULD clauses hold 1..=RGPU_MAX_BOOL_PHRASES exact PhraseQuery clauses
    /// beside TermQuery clauses, with MUST_NOT TermQuery clauses and any min_should_match up to 255: "\"a b\" \"c d\" e -f" ->
    /// rgpu_search_phrase_or_batch per leaf. phrase_slot = the phrase's index in BooleanWeight::should_weights (the SHOULD clauses in
    /// query order); the library drops the clauses a leaf lacks and sums the others in that order, as DisjunctionSumScorer's
    /// SimpleQueue arm does (disjunction_scorer.rs:213-225). Ok(false) — the CPU searcher — under try_phrase's rules (another field,
    /// a leaf without positions, a phrase of the wrong size) and for every shape the library does not serve: a sloppy phrase clause
    /// (two-phase), ten or more SHOULD clauses (the heap-order arm), a phrase under MUST_NOT, a nested BooleanQuery, more than
    /// RGPU_MAX_BOOL_PHRASES phrases, more than RGPU_MAX_QUERY_TERMS clause terms.
    /// `masks` as for try_phrase: rgpu_search_phrase_or_batch_masked.
    fn try_phrase_or(&self, b: &BooleanQuery<C>, masks: Option<&[*mut RgpuDocset]>, top: &mut TopDocsCollector, k: usize) -> Result<bool> {
        let (must, should, filter, must_not, min_should_match) = b.clauses();
        if !must.is_empty() || !filter.is_empty() || should.is_empty() || should.len() > 9 || min_should_match < 0 || min_should_match > 255
            || self.leaves.iter().any(|l| !l.has_positions) {
            return Ok(false);
        }
        let term_of = |q: &Box<dyn Query<C>>| q.as_any().downcast_ref::<TermQuery>().filter(|t| t.term.field == self.field);
        let mut phrases: Vec<(&PhraseQuery, usize)> = Vec::new(); // (the phrase, its slot in should_weights)
        let mut optional: Vec<&TermQuery> = Vec::new();
        for (slot, q) in should.iter().enumerate() {
            if let Some(p) = q.as_any().downcast_ref::<PhraseQuery>() {
                let (field, terms, positions, slop) = p.parts();
                if field != self.field || slop != 0 || terms.len() < 2 || terms.len() > RGPU_MAX_PHRASE_TERMS as usize || terms.len() != positions.len() {
                    return Ok(false);
                }
                phrases.push((p, slot));
            } else if let Some(t) = term_of(q) {
                optional.push(t);
            } else {
                return Ok(false);
            }
        }
        if phrases.is_empty() || phrases.len() > RGPU_MAX_BOOL_PHRASES as usize { return Ok(false); }
        let mut prohibited: Vec<&TermQuery> = Vec::with_capacity(must_not.len());
        for q in must_not {
            match term_of(q) { Some(t) => prohibited.push(t), None => return Ok(false) }
        }
        let n_phrase_terms: usize = phrases.iter().map(|(p, _)| p.parts().1.len()).sum();
        if n_phrase_terms + optional.len() + prohibited.len() > RGPU_MAX_QUERY_TERMS as usize { return Ok(false); }
        let mut phrase_weights = Vec::with_capacity(phrases.len());
        for (p, _) in &phrases {
            let term_refs: Vec<&Term> = p.parts().1.iter().collect();
            phrase_weights.push(self.weight_of(&term_refs, 1.0)?);
        }
        let mut term_weights = Vec::with_capacity(optional.len());
        for t in &optional { term_weights.push(self.weight_of(&[&t.term], t.boost)?); }
        let mut oq = RgpuPhraseOrQuery { n_phrases: phrases.len() as i32, first_phrase: 0, n_terms: optional.len() as i32, first_term: 0,
                                         n_must_not: prohibited.len() as i32, min_should_match, phrase_slot: [0; 4], reserved: [0; 2] };
        for (i, (_, slot)) in phrases.iter().enumerate() { oq.phrase_slot[i] = *slot as i32; }
        for leaf in self.cpu.reader().leaves() {
            let mut pqs = Vec::with_capacity(phrases.len());
            let mut pterms: Vec<RgpuPhraseTerm> = Vec::with_capacity(n_phrase_terms);
            for (i, (p, _)) in phrases.iter().enumerate() {
                let (_, terms, positions, _) = p.parts();
                let mine = self.phrase_terms(&leaf, terms, positions)?;
                pqs.push(RgpuPhraseQuery { n_terms: mine.len() as i32, first_term: pterms.len() as i32, weight: phrase_weights[i].0, sim_table: phrase_weights[i].1,
                                           slop: 0, next_limit: 0 });
                pterms.extend(mine);
            }
            let mut terms = Vec::with_capacity(optional.len() + prohibited.len());
            for (i, t) in optional.iter().enumerate() {
                terms.push(RgpuQueryTerm { state: Self::term_state(&self.block_state(&leaf, &t.term)?), weight: term_weights[i].0, sim_table: term_weights[i].1 });
            }
            for t in &prohibited {
                terms.push(RgpuQueryTerm { state: Self::term_state(&self.block_state(&leaf, &t.term)?), weight: 0.0, sim_table: 0 }); // never scored
            }
            let mut hits = vec![RgpuHit { doc: -1, score: 0.0 }; k];
            let mut total: i64 = 0;
            let seg = self.leaves[leaf.ord].seg;
            let terms_ptr = if terms.is_empty() { std::ptr::null() } else { terms.as_ptr() };
            check(unsafe {
                match masks {
                    Some(m) => rgpu_search_phrase_or_batch_masked(seg, m[leaf.ord], &oq, 1, pqs.as_ptr(), pqs.len() as i32, pterms.as_ptr(), pterms.len() as i32,
                                                                  terms_ptr, terms.len() as i32, k as i32, hits.as_mut_ptr(), &mut total),
                    None => rgpu_search_phrase_or_batch(seg, &oq, 1, pqs.as_ptr(), pqs.len() as i32, pterms.as_ptr(), pterms.len() as i32,
                                                        terms_ptr, terms.len() as i32, k as i32, hits.as_mut_ptr(), &mut total),
                }
            }, self.ctx)?;
            Self::hand_over(top, &hits, total);
        }
        Ok(true)
    }

    /// BooleanQuery with at least one required (MUST / FILTER) clause AND 1..=9 SHOULD clauses, up to RGPU_MAX_BOOL_PHRASES exact
    /// PhraseQuery clauses on each side beside TermQuery clauses, with MUST_NOT TermQuery clauses: "+a +b \"a b\"", "+\"a b\" c -d #e" ->
    /// rgpu_search_phrase_opt_batch per leaf (`optional_phrases`). req_phrase_slot / opt_phrase_slot = the phrase's index in
    /// BooleanWeight::must_weights (MUST clauses in query order, then FILTER clauses, which ride with weight 0) / should_weights; the
    /// library sums the required side in the leaf's stable cost order, the optional side from 0.0 in clause order over the clauses
    /// the leaf holds, and applies ReqOptScorer's sequential rule (req_opt_scorer.rs:41-66) per leaf. min_should_match is carried and
    /// without effect, as in the reference. Ok(false) - the CPU searcher - under try_phrase's rules (another field, a leaf without
    /// positions, a phrase of the wrong size) and for every shape the library does not serve: a sloppy phrase clause, ten or more SHOULD
    /// clauses, a phrase under MUST_NOT, a nested BooleanQuery, more than RGPU_MAX_BOOL_PHRASES phrases on a side, more than
    /// RGPU_MAX_QUERY_TERMS clause terms. There is no masked form: a filtered tree of this kind stays the CPU's.
    fn try_phrase_opt(&self, b: &BooleanQuery<C>, top: &mut TopDocsCollector, k: usize) -> Result<bool> {
        let (must, should, filter, must_not, min_should_match) = b.clauses();
        if (must.is_empty() && filter.is_empty()) || should.is_empty() || should.len() > 9 || min_should_match < 0 || min_should_match > 255
            || self.leaves.iter().any(|l| !l.has_positions) {
            return Ok(false);
        }
        let term_of = |q: &Box<dyn Query<C>>| q.as_any().downcast_ref::<TermQuery>().filter(|t| t.term.field == self.field);
        // (the phrase, its slot on its side, scores?) - required ones first, then optional ones: the call's phrase order
        let mut req_phrases: Vec<(&PhraseQuery, usize, bool)> = Vec::new();
        let mut opt_phrases: Vec<(&PhraseQuery, usize, bool)> = Vec::new();
        let mut required: Vec<(&TermQuery, bool)> = Vec::new();
        let mut optional: Vec<(&TermQuery, bool)> = Vec::new();
        let n_must = must.len();
        let sides: [(Vec<&Box<dyn Query<C>>>, bool); 2] = [(must.iter().chain(filter.iter()).collect(), true), (should.iter().collect(), false)];
        for (side, is_required) in sides.iter() {
            for (slot, q) in side.iter().enumerate() {
                let scoring = !*is_required || slot < n_must;
                if let Some(p) = q.as_any().downcast_ref::<PhraseQuery>() {
                    let (field, terms, positions, slop) = p.parts();
                    if field != self.field || slop != 0 || terms.len() < 2 || terms.len() > RGPU_MAX_PHRASE_TERMS as usize || terms.len() != positions.len() {
                        return Ok(false);
                    }
                    if *is_required { req_phrases.push((p, slot, scoring)); } else { opt_phrases.push((p, slot, scoring)); }
                } else if let Some(t) = term_of(q) {
                    if *is_required { required.push((t, scoring)); } else { optional.push((t, scoring)); }
                } else {
                    return Ok(false);
                }
            }
        }
        if req_phrases.len() > RGPU_MAX_BOOL_PHRASES as usize || opt_phrases.len() > RGPU_MAX_BOOL_PHRASES as usize { return Ok(false); }
        let mut prohibited: Vec<&TermQuery> = Vec::with_capacity(must_not.len());
        for q in must_not {
            match term_of(q) { Some(t) => prohibited.push(t), None => return Ok(false) }
        }
        let phrases: Vec<&(&PhraseQuery, usize, bool)> = req_phrases.iter().chain(opt_phrases.iter()).collect();
        let scored: Vec<&(&TermQuery, bool)> = required.iter().chain(optional.iter()).collect();
        let n_phrase_terms: usize = phrases.iter().map(|(p, _, _)| p.parts().1.len()).sum();
        if n_phrase_terms + scored.len() + prohibited.len() > RGPU_MAX_QUERY_TERMS as usize { return Ok(false); }
        let mut phrase_weights = Vec::with_capacity(phrases.len());
        for (p, _, scoring) in &phrases {
            let term_refs: Vec<&Term> = p.parts().1.iter().collect();
            let w = self.weight_of(&term_refs, 1.0)?;
            phrase_weights.push((if *scoring { w.0 } else { 0.0 }, w.1)); // a FILTER phrase scores 0 (needs_scores = false)
        }
        let mut term_weights = Vec::with_capacity(scored.len());
        for (t, scoring) in &scored {
            let w = self.weight_of(&[&t.term], t.boost)?;
            term_weights.push((if *scoring { w.0 } else { 0.0 }, w.1));
        }
        let mut oq = RgpuPhraseOptQuery { n_req_phrases: req_phrases.len() as i32, n_opt_phrases: opt_phrases.len() as i32, first_phrase: 0,
                                          n_req_terms: required.len() as i32, n_opt_terms: optional.len() as i32, first_term: 0,
                                          n_must_not: prohibited.len() as i32, min_should_match, req_phrase_slot: [0; 4], opt_phrase_slot: [0; 4] };
        for (i, (_, slot, _)) in req_phrases.iter().enumerate() { oq.req_phrase_slot[i] = *slot as i32; }
        for (i, (_, slot, _)) in opt_phrases.iter().enumerate() { oq.opt_phrase_slot[i] = *slot as i32; }
        for leaf in self.cpu.reader().leaves() {
            let mut pqs = Vec::with_capacity(phrases.len());
            let mut pterms: Vec<RgpuPhraseTerm> = Vec::with_capacity(n_phrase_terms);
            for (i, (p, _, _)) in phrases.iter().enumerate() {
                let (_, terms, positions, _) = p.parts();
                let mine = self.phrase_terms(&leaf, terms, positions)?;
                pqs.push(RgpuPhraseQuery { n_terms: mine.len() as i32, first_term: pterms.len() as i32, weight: phrase_weights[i].0, sim_table: phrase_weights[i].1,
                                           slop: 0, next_limit: 0 });
                pterms.extend(mine);
            }
            let mut terms = Vec::with_capacity(scored.len() + prohibited.len());
            for (i, (t, _)) in scored.iter().enumerate() {
                terms.push(RgpuQueryTerm { state: Self::term_state(&self.block_state(&leaf, &t.term)?), weight: term_weights[i].0, sim_table: term_weights[i].1 });
            }
            for t in &prohibited {
                terms.push(RgpuQueryTerm { state: Self::term_state(&self.block_state(&leaf, &t.term)?), weight: 0.0, sim_table: 0 }); // never scored
            }
            let mut hits = vec![RgpuHit { doc: -1, score: 0.0 }; k];
            let mut total: i64 = 0;
            let seg = self.leaves[leaf.ord].seg;
            let terms_ptr = if terms.is_empty() { std::ptr::null() } else { terms.as_ptr() };
            check(unsafe {
                rgpu_search_phrase_opt_batch(seg, &oq, 1, pqs.as_ptr(), pqs.len() as i32, pterms.as_ptr(), pterms.len() as i32,
                                             terms_ptr, terms.len() as i32, k as i32, hits.as_mut_ptr(), &mut total)
            }, self.ctx)?;
            Self::hand_over(top, &hits, total);
        }
        Ok(true)
    }

    /// Many queries at once — what the GPU is for (bench.py: 1024 single-term queries take 0.05 ms as one batch; one at a time
    /// each call costs a launch + a synchronisation, see `latency_batch_of_one` there). queries[i] is collected into
    /// collectors[i] (all built with the same estimated_hits = k). Term / boolean trees go to the GPU as ONE
    /// rgpu_search_batch per leaf; phrases as one rgpu_search_phrase_batch per leaf; whatever the C ABI does not serve (and
    /// any batch the library refuses with RGPU_ERR_UNSUPPORTED) runs through DefaultIndexSearcher::search one by one.
    /// (A batch of identical shape whose terms are known by id or bytes can skip this per-clause work altogether:
    /// rgpu_planner_create + rgpu_plan_uniform_ids / rgpu_plan_batch_bytes resolve, weigh and pack natively.)
    /// The cached BitDocIdSet of every leaf (`FixedBitSet::bits`, ceil(max_doc / 64) words each, by LeafReaderContext::ord) -> doc sets.
    pub fn cache_filter_bits(&self, per_leaf_words: &[&[u64]]) -> Result<GpuCachedFilter> {
        if per_leaf_words.len() != self.leaves.len() { bail!(ErrorKind::IllegalArgument("one bit set per leaf".into())); }
        let mut made = GpuCachedFilter { sets: Vec::with_capacity(self.leaves.len()) };
        for (leaf, words) in self.leaves.iter().zip(per_leaf_words.iter()) {
            let mut set: *mut RgpuDocset = std::ptr::null_mut();
            check(unsafe { rgpu_docset_from_words(leaf.seg, words.as_ptr(), &mut set) }, self.ctx)?;
            made.sets.push(set);
        }
        Ok(made)
    }

    /// LRUQueryCache::do_cache on the GPU for a query that flattens to TERM / all-MUST / all-SHOULD (msm <= 1) with or without MUST_NOT
    /// terms: per leaf the docs it matches, live docs not applied (query_cache.rs:335-342). None: not such a query — fill on the CPU.
    pub fn cache_filter_query(&self, query: &dyn Query<C>) -> Result<Option<GpuCachedFilter>> {
        let flat = match self.flatten(query) { Some(f) => f, None => return Ok(None) };
        let base = flat.op & 0xff;
        if !flat.optional.is_empty() || (flat.op >> 8) != 0 || !(base == RGPU_OP_TERM || base == RGPU_OP_AND || base == RGPU_OP_OR) { return Ok(None); }
        let n = flat.n_clauses();
        if n > RGPU_MAX_QUERY_TERMS as usize { return Ok(None); }
        let table = self.sim_table(self.cpu.collections_statistics(&self.field).ok_or_else(|| Error::from(ErrorKind::IllegalState("no statistics".into())))?)?;
        let mut made = GpuCachedFilter { sets: Vec::with_capacity(self.leaves.len()) };
        for leaf in self.cpu.reader().leaves() {
            let mut terms = Vec::with_capacity(n);
            for t in flat.clauses() {
                terms.push(RgpuQueryTerm { state: Self::term_state(&self.block_state(&leaf, &t.term)?), weight: 0.0, sim_table: table }); // nothing is scored
            }
            let q = RgpuQuery { op: flat.op, n_terms: flat.positive.len() as i32, first_term: 0, n_must_not: flat.must_not.len() as i32 };
            let mut set: *mut RgpuDocset = std::ptr::null_mut();
            check(unsafe { rgpu_docset_collect_batch(self.leaves[leaf.ord].seg, &q, 1, terms.as_ptr(), n as i32, &mut set) }, self.ctx)?;
            made.sets.push(set);
        }
        Ok(Some(made))
    }

    /// Upload the points of `field` for every leaf: PointValues::intersect with a visitor that takes every cell
    /// (AllPointsVisitor), then rgpu_points_attach. Ok(None): the field has more than one dimension in some leaf, or values that are
    /// not 4 or 8 bytes wide — such ranges stay on the CPU path (what a multi-dimensional PointRangeQuery matches depends on the
    /// BKD cell layout: PointRangeIntersectVisitor::compare, point_range_query.rs:642-664, slices lower_point without an end).
    pub fn attach_points(&self, field: &str) -> Result<Option<GpuPoints>> {
        let mut made = GpuPoints { field: field.to_string(), bytes_per_dim: 0, per_leaf: Vec::with_capacity(self.leaves.len()) };
        for leaf in self.cpu.reader().leaves() {
            let values = match leaf.reader.point_values() { Some(v) => v, None => { made.per_leaf.push(std::ptr::null_mut()); continue; } };
            if leaf.reader.field_info(field).map_or(true, |fi| fi.point_dimension_count == 0) { made.per_leaf.push(std::ptr::null_mut()); continue; }
            let dims = values.num_dimensions(field)?;
            let width = values.bytes_per_dimension(field)?;
            if dims != 1 || !(width == 4 || width == 8) || (made.bytes_per_dim != 0 && made.bytes_per_dim != width) { return Ok(None); }
            made.bytes_per_dim = width;
            let mut all = AllPointsVisitor { docs: Vec::new(), values: Vec::new() };
            values.intersect(field, &mut all)?;
            let mut points: *mut RgpuPoints = std::ptr::null_mut();
            check(unsafe { rgpu_points_attach(self.leaves[leaf.ord].seg, width as i32, all.docs.as_ptr(), all.values.as_ptr(), all.docs.len() as i64, &mut points) }, self.ctx)?;
            made.per_leaf.push(points);
        }
        if made.bytes_per_dim == 0 { return Ok(None); } // no leaf holds the field
        Ok(Some(made))
    }

    /// PointRangeQuery(points.field, lower, upper) as a cached filter: per leaf the docs holding a point inside the closed range,
    /// built on the GPU (rgpu_docset_from_point_ranges, the library chooses scatter or scan), live docs not applied — what
    /// create_scorer (point_range_query.rs:503-561) collects. A leaf without the field gives the empty set, as the reference's missing
    /// scorer does. The result goes to `try_filtered`: a range under MUST or FILTER among `filters` (both add + 0.0), under MUST_NOT
    /// among `excludes`. `try_filtered`'s `query` is the BooleanQuery WITHOUT its range clauses: build it with the min_should_match
    /// the whole query has ("+range #a b" has 0 where BooleanQuery::build gives "#a b" 1; beside required clauses both match the
    /// same docs — ReqOptScorer's optional side — but a caller that forwards min_should_match elsewhere must keep the original).
    /// A serving layer memoises the filter per (field, lower, upper) with a bound of its own: every distinct range is
    /// ceil(max_doc / 64) * 8 bytes per leaf in HBM until the GpuCachedFilter is dropped. Ok(None): bounds of another width than one value —
    /// the CPU searcher reports the reference's IllegalArgument (:510-522) itself.
    pub fn try_range_filter(&self, points: &GpuPoints, lower: &[u8], upper: &[u8]) -> Result<Option<GpuCachedFilter>> {
        if points.per_leaf.len() != self.leaves.len() { bail!(ErrorKind::IllegalArgument("points of another searcher".into())); }
        if lower.len() != points.bytes_per_dim || upper.len() != points.bytes_per_dim { return Ok(None); }
        let mut range = RgpuPointRange { lower: [0u8; 8], upper: [0u8; 8] };
        range.lower[..lower.len()].copy_from_slice(lower);
        range.upper[..upper.len()].copy_from_slice(upper);
        let mut made = GpuCachedFilter { sets: Vec::with_capacity(self.leaves.len()) };
        for (leaf, &pts) in self.leaves.iter().zip(points.per_leaf.iter()) {
            let mut set: *mut RgpuDocset = std::ptr::null_mut();
            if pts.is_null() {
                check(unsafe { rgpu_docset_from_docs(leaf.seg, std::ptr::null(), 0, &mut set) }, self.ctx)?;
            } else {
                check(unsafe { rgpu_docset_from_point_ranges(pts, &range, 1, 0, &mut set) }, self.ctx)?;
            }
            made.sets.push(set);
        }
        Ok(Some(made))
    }

    /// `query` restricted to the docs every one of `filters` holds and none of `excludes` holds: rgpu_search_batch_masked per leaf.
    /// `as_filter_query`: the caller holds FilterQuery(query, filters) (query/filter_query.rs:155-233), which asks only that `query`
    /// has a scorer of its own; otherwise the sets are FILTER / MUST_NOT clauses of the BooleanQuery `query` was taken out of, and the
    /// rows are the reference's only when (1) what is left contributes a MUST or FILTER clause — "b c #F" is ReqOptScorer(F, b | c) in
    /// the reference and matches ALL of F — and (2) for a MUST_NOT set, min_should_match <= 1 (boolean_query.rs:235-251 reuses it for
    /// the MUST_NOT union). Ok(false): not served here — the CPU searcher takes the whole query. A phrase, or a tree over phrases, is
    /// the CPU's unless `filtered_phrases` is set (try_filtered_phrase; never a sloppy one: its next_limit counts deleted docs, not
    /// docs outside a filter).
    pub fn try_filtered(&self, query: &dyn Query<C>, filters: &[&GpuCachedFilter], excludes: &[&GpuCachedFilter], as_filter_query: bool,
                        top: &mut TopDocsCollector, k: usize) -> Result<bool> {
        if k == 0 || k > RGPU_MAX_K as usize || (filters.is_empty() && excludes.is_empty()) { return Ok(false); }
        if filters.iter().chain(excludes.iter()).any(|f| f.sets.len() != self.leaves.len()) { bail!(ErrorKind::IllegalArgument("a cached filter of another searcher".into())); }
        if self.filtered_phrases {
            if let Some(served) = self.try_filtered_phrase(query, filters, excludes, as_filter_query, top, k)? { return Ok(served); }
        }
        let flat = match self.flatten(query) { Some(f) => f, None => return Ok(false) }; // (a PhraseQuery, a tree over phrases: not flat)
        let base = flat.op & 0xff;
        let msm = (flat.op >> 8) & 0xff;
        if !as_filter_query {
            if !excludes.is_empty() && msm > 1 { return Ok(false); }
            if !(base == RGPU_OP_TERM || base == RGPU_OP_AND) {   // no required clause of its own
                if !self.required_sets || base != RGPU_OP_OR { return Ok(false); }
                // "b c #F": the sets are the only required clauses. "b c -X" gets no MatchAllDocsQuery (boolean_query.rs:76-79 adds one
                // only when there is no MUST, SHOULD or FILTER clause): ReqNotScorer over the disjunction, the masked search below.
                if !filters.is_empty() { return self.try_required_set(Some(&flat), filters, excludes, top, k); }
            }
        }
        let n = flat.n_clauses();
        if n > RGPU_MAX_QUERY_TERMS as usize { return Ok(false); }
        let weights = self.clause_weights(&flat)?;
        for leaf in self.cpu.reader().leaves() {
            let seg = self.leaves[leaf.ord].seg;
            // one set per leaf: the single filter itself, or the AND of the filters minus the excludes (a serving layer memoises this per
            // combination and leaf, as the Python and C++ mirrors do)
            let all: Vec<*mut RgpuDocset> = filters.iter().map(|f| f.sets[leaf.ord]).collect();
            let none: Vec<*mut RgpuDocset> = excludes.iter().map(|f| f.sets[leaf.ord]).collect();
            let mut combined: *mut RgpuDocset = std::ptr::null_mut();
            let mask = if all.len() == 1 && none.is_empty() { all[0] } else {
                check(unsafe { rgpu_docset_combine(seg, all.as_ptr(), all.len() as i32, none.as_ptr(), none.len() as i32, &mut combined) }, self.ctx)?;
                combined
            };
            let mut terms = Vec::with_capacity(n);
            for (i, t) in flat.clauses().enumerate() {
                terms.push(RgpuQueryTerm { state: Self::term_state(&self.block_state(&leaf, &t.term)?), weight: weights[i].0, sim_table: weights[i].1 });
            }
            let q = RgpuQuery { op: flat.op, n_terms: flat.positive.len() as i32, first_term: 0, n_must_not: flat.must_not.len() as i32 };
            let mut hits = vec![RgpuHit { doc: -1, score: 0.0 }; k];
            let mut total: i64 = 0;
            let rc = unsafe { rgpu_search_batch_masked(seg, mask, &q, 1, terms.as_ptr(), n as i32, k as i32, hits.as_mut_ptr(), &mut total) };
            if !combined.is_null() { unsafe { rgpu_docset_free(combined) }; }
            check(rc, self.ctx)?;
            Self::hand_over(top, &hits, total);
        }
        Ok(true)
    }

    /// A lone "#F" / range, or "-X" (which BooleanQuery::build turns into "+*:* -X"): `filters` as the only required clauses, no SHOULD
    /// side. With no filter at all the every-doc set stands in for MatchAllDocsQuery. Ok(false): `required_sets` is off.
    pub fn try_filter_alone(&self, filters: &[&GpuCachedFilter], excludes: &[&GpuCachedFilter], top: &mut TopDocsCollector, k: usize) -> Result<bool> {
        if !self.required_sets || k == 0 || k > RGPU_MAX_K as usize || (filters.is_empty() && excludes.is_empty()) { return Ok(false); }
        if filters.iter().chain(excludes.iter()).any(|f| f.sets.len() != self.leaves.len()) { bail!(ErrorKind::IllegalArgument("a cached filter of another searcher".into())); }
        self.try_required_set(None, filters, excludes, top, k)
    }

    /// The sets are the query's ONLY required clauses: ReqOptScorer(sets, DisjunctionSumScorer(SHOULD clauses)) in the reference, whose
    /// required side scores 0.0 and whose skipping rule therefore never fires — every doc of live AND filters AND NOT excludes is
    /// collected, scored by the disjunction where it matches and 0.0 elsewhere (rgpu_search_batch_required_set, one call per leaf;
    /// min_should_match has no effect there and is dropped). `flat`: the SHOULD side, an RGPU_OP_OR query; None: no optional side.
    /// Ok(false) — the CPU searcher: MUST_NOT term clauses beside the sets (not folded into a set here), a boost <= 0.
    fn try_required_set(&self, flat: Option<&FlatQuery<'_>>, filters: &[&GpuCachedFilter], excludes: &[&GpuCachedFilter], top: &mut TopDocsCollector,
                        k: usize) -> Result<bool> {
        let n = flat.map_or(0, |f| f.positive.len());
        if let Some(f) = flat {
            if !f.must_not.is_empty() || !f.optional.is_empty() || n == 0 || n > RGPU_MAX_QUERY_TERMS as usize { return Ok(false); }
            if f.positive.iter().any(|(_, boost)| !(*boost > 0.0)) { return Ok(false); }
        }
        let weights = match flat { Some(f) => self.clause_weights(f)?, None => Vec::new() };
        for leaf in self.cpu.reader().leaves() {
            let seg = self.leaves[leaf.ord].seg;
            let all: Vec<*mut RgpuDocset> = filters.iter().map(|f| f.sets[leaf.ord]).collect();
            let none: Vec<*mut RgpuDocset> = excludes.iter().map(|f| f.sets[leaf.ord]).collect();
            let mut combined: *mut RgpuDocset = std::ptr::null_mut();
            // (no filter: rgpu_docset_combine starts from every doc of the leaf — MatchAllDocsQuery as a set)
            let mask = if all.len() == 1 && none.is_empty() { all[0] } else {
                check(unsafe { rgpu_docset_combine(seg, all.as_ptr(), all.len() as i32, none.as_ptr(), none.len() as i32, &mut combined) }, self.ctx)?;
                combined
            };
            let mut terms = Vec::with_capacity(n);
            if let Some(f) = flat {
                for (i, (t, _)) in f.positive.iter().enumerate() {
                    terms.push(RgpuQueryTerm { state: Self::term_state(&self.block_state(&leaf, &t.term)?), weight: weights[i].0, sim_table: weights[i].1 });
                }
            }
            let q = RgpuQuery { op: RGPU_OP_OR, n_terms: n as i32, first_term: 0, n_must_not: 0 };
            let terms_ptr = if terms.is_empty() { std::ptr::null() } else { terms.as_ptr() };
            let mut hits = vec![RgpuHit { doc: -1, score: 0.0 }; k];
            let mut total: i64 = 0;
            let rc = unsafe { rgpu_search_batch_required_set(seg, mask, &q, 1, terms_ptr, n as i32, k as i32, hits.as_mut_ptr(), &mut total) };
            if !combined.is_null() { unsafe { rgpu_docset_free(combined) }; }
            check(rc, self.ctx)?;
            Self::hand_over(top, &hits, total);
        }
        Ok(true)
    }

    /// try_filtered for a PhraseQuery or a BooleanQuery with PhraseQuery clauses (`filtered_phrases`): None — `query` is neither;
    /// Some(false) — the CPU searcher; Some(true) — collected through the masked phrase calls, one per leaf. The rules: a required
    /// phrase (alone, or among MUST / FILTER clauses) under either spelling; a disjunction over phrases under FilterQuery, or beside
    /// MUST_NOT sets only with min_should_match <= 1 ("\"a b\" c #F": the set is the only required clause and the reference matches
    /// all of it).
    fn try_filtered_phrase(&self, query: &dyn Query<C>, filters: &[&GpuCachedFilter], excludes: &[&GpuCachedFilter], as_filter_query: bool,
                           top: &mut TopDocsCollector, k: usize) -> Result<Option<bool>> {
        let phrase = query.as_any().downcast_ref::<PhraseQuery>();
        let tree = query.as_any().downcast_ref::<BooleanQuery<C>>().filter(|b| {
            let (must, should, filter, must_not, _) = b.clauses();
            must.iter().chain(should).chain(filter).chain(must_not).any(|q| q.as_any().downcast_ref::<PhraseQuery>().is_some())
        });
        if phrase.is_none() && tree.is_none() { return Ok(None); }
        let disjunction = tree.map_or(false, |b| { let (must, _, filter, _, _) = b.clauses(); must.is_empty() && filter.is_empty() });
        if disjunction && !as_filter_query {
            let msm = tree.map_or(0, |b| b.clauses().4);
            if !filters.is_empty() || msm > 1 { return Ok(Some(false)); }
        }
        // one set per leaf: the single filter itself, or the AND of the filters minus the excludes, freed behind the calls
        let mut masks: Vec<*mut RgpuDocset> = Vec::with_capacity(self.leaves.len());
        let mut combined: Vec<*mut RgpuDocset> = Vec::new();
        let mut rc = 0;
        for (ord, leaf) in self.leaves.iter().enumerate() {
            if filters.len() == 1 && excludes.is_empty() { masks.push(filters[0].sets[ord]); continue; }
            let all: Vec<*mut RgpuDocset> = filters.iter().map(|f| f.sets[ord]).collect();
            let none: Vec<*mut RgpuDocset> = excludes.iter().map(|f| f.sets[ord]).collect();
            let mut made: *mut RgpuDocset = std::ptr::null_mut();
            rc = unsafe { rgpu_docset_combine(leaf.seg, all.as_ptr(), all.len() as i32, none.as_ptr(), none.len() as i32, &mut made) };
            if rc != 0 { break; }
            masks.push(made);
            combined.push(made);
        }
        let served = if rc != 0 { check(rc, self.ctx).map(|_| false) } else if let Some(p) = phrase {
            self.try_phrase(p, Some(&masks), top, k)
        } else if disjunction {
            self.try_phrase_or(tree.unwrap(), Some(&masks), top, k)
        } else {
            self.try_phrase_bool(tree.unwrap(), Some(&masks), top, k)
        };
        for set in combined { unsafe { rgpu_docset_free(set) }; }
        served.map(Some)
    }

    pub fn search_many(&self, queries: &[&dyn Query<C>], collectors: &mut [TopDocsCollector]) -> Result<()> {
        assert_eq!(queries.len(), collectors.len());
        if queries.is_empty() { return Ok(()); }
        let k = collectors[0].estimated_hits();
        let uniform_k = collectors.iter().all(|c| c.estimated_hits() == k);
        let mut flat_ix = Vec::new(); // queries[i] served as a flat clause list
        let mut flats = Vec::new();
        let mut cpu_ix = Vec::new();
        for (i, q) in queries.iter().enumerate() {
            let flat = if uniform_k && k > 0 && k <= RGPU_MAX_K as usize && q.as_any().downcast_ref::<PhraseQuery>().is_none() { self.flatten(*q) } else { None };
            match flat {
                Some(f) if f.n_clauses() <= RGPU_MAX_QUERY_TERMS as usize => { flat_ix.push(i); flats.push(f); }
                _ => cpu_ix.push(i),
            }
        }
        if !flats.is_empty() {
            let mut weights = Vec::new(); // clause weights do not depend on the leaf: once per batch
            for f in &flats { weights.push(self.clause_weights(f)?); }
            let n_terms_total: usize = flats.iter().map(|f| f.n_clauses()).sum();
            let mut served = true;
            let mut per_leaf: Vec<(Vec<RgpuHit>, Vec<i64>)> = Vec::new();
            for leaf in self.cpu.reader().leaves() {
                let mut qs = Vec::with_capacity(flats.len());
                let mut terms = Vec::with_capacity(n_terms_total);
                for (f, w) in flats.iter().zip(weights.iter()) {
                    qs.push(RgpuQuery { op: f.op, n_terms: f.positive.len() as i32, first_term: terms.len() as i32, n_must_not: f.must_not.len() as i32 });
                    for (c, t) in f.clauses().enumerate() {
                        terms.push(RgpuQueryTerm { state: Self::term_state(&self.block_state(&leaf, &t.term)?), weight: w[c].0, sim_table: w[c].1 });
                    }
                }
                let mut hits = vec![RgpuHit { doc: -1, score: 0.0 }; qs.len() * k];
                let mut totals = vec![0i64; qs.len()];
                let rc = unsafe { rgpu_search_batch(self.leaves[leaf.ord].seg, qs.as_ptr(), qs.len() as i32, terms.as_ptr(), terms.len() as i32, k as i32,
                                                    hits.as_mut_ptr(), totals.as_mut_ptr()) };
                if rc == RGPU_ERR_UNSUPPORTED { served = false; break; } // nothing handed over yet: the whole batch takes the CPU path
                check(rc, self.ctx)?;
                per_leaf.push((hits, totals));
            }
            if served {
                for (hits, totals) in &per_leaf {
                    for (j, &i) in flat_ix.iter().enumerate() { Self::hand_over(&mut collectors[i], &hits[j * k..(j + 1) * k], totals[j]); }
                }
            } else {
                cpu_ix.extend(flat_ix.iter().cloned());
            }
        }
        for i in cpu_ix { self.search(queries[i], &mut collectors[i])?; } // phrases go to the GPU from there, one by one
        Ok(())
    }
}

impl<C: Codec, R: IndexReader<Codec = C> + ?Sized, IR: Deref<Target = R>, SP: SimilarityProducer<C>> IndexSearcher<C> for GpuIndexSearcher<C, R, IR, SP> {
    type Reader = R;
    fn reader(&self) -> &R { self.cpu.reader() }

    /// IndexSearcher::search (searcher.rs:487-525). A TopDocsCollector over a tree of term clauses goes to the GPU; every other
    /// collector or query — and any RGPU_ERR_UNSUPPORTED the library answers with — takes the CPU path unchanged.
    fn search<S: SearchCollector>(&self, query: &dyn Query<C>, collector: &mut S) -> Result<()> {
        if let Some(top) = (collector as &mut dyn std::any::Any).downcast_mut::<TopDocsCollector>() {
            let k = top.estimated_hits();
            match self.try_gpu(query, top, k) {
                Ok(true) => return Ok(()),
                Ok(false) | Err(Error(ErrorKind::UnsupportedOperation(_), _)) => {}
                Err(e) => return Err(e),
            }
        }
        self.cpu.search(query, collector)
    }
    fn search_parallel<S: SearchCollector>(&self, query: &dyn Query<C>, collector: &mut S) -> Result<()> { self.search(query, collector) }
    /// IndexSearcher::count (searcher.rs:632-654): what `flatten` accepts is counted on the GPU (rgpu_count_batch per leaf, nothing
    /// scored); every other query - and any RGPU_ERR_UNSUPPORTED the library answers with - takes the CPU path unchanged.
    fn count(&self, query: &dyn Query<C>) -> Result<i32> {
        match self.try_count(query) {
            Ok(Some(n)) => Ok(n),
            Ok(None) | Err(Error(ErrorKind::UnsupportedOperation(_), _)) => self.cpu.count(query),
            Err(e) => Err(e),
        }
    }
    fn explain(&self, query: &dyn Query<C>, doc: DocId) -> Result<core::search::explanation::Explanation> { self.cpu.explain(query, doc) }
}

impl<C: Codec, R: IndexReader<Codec = C> + ?Sized, IR: Deref<Target = R>, SP: SimilarityProducer<C>> SearchPlanBuilder<C> for GpuIndexSearcher<C, R, IR, SP> {
    fn num_docs(&self) -> i32 { self.cpu.num_docs() }
    fn max_doc(&self) -> i32 { self.cpu.max_doc() }
    fn create_weight(&self, q: &dyn Query<C>, needs_scores: bool) -> Result<Box<dyn core::search::query::Weight<C>>> { self.cpu.create_weight(q, needs_scores) }
    fn create_normalized_weight(&self, q: &dyn Query<C>, needs_scores: bool) -> Result<Box<dyn core::search::query::Weight<C>>> { self.cpu.create_normalized_weight(q, needs_scores) }
    fn similarity(&self, field: &str, needs_scores: bool) -> Box<dyn core::search::similarity::Similarity<C>> { self.cpu.similarity(field, needs_scores) }
    fn term_statistics(&self, term: &Term) -> Result<TermStatistics> { self.cpu.term_statistics(term) }
    fn collections_statistics(&self, field: &str) -> Option<&CollectionStatistics> { self.cpu.collections_statistics(field) }
}

impl<C: Codec, R: IndexReader<Codec = C> + ?Sized, IR: Deref<Target = R>, SP: SimilarityProducer<C>> Drop for GpuIndexSearcher<C, R, IR, SP> {
    fn drop(&mut self) {
        for l in &self.leaves { unsafe { rgpu_segment_free(l.seg) }; }
        unsafe { rgpu_shutdown(self.ctx) };
    }
}
