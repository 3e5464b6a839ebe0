// Host-only helpers, no GPU involved: the parsers of host/*.hpp behind the C ABI. struct rgpu_terms, terms_lookup_impl. Entry points:
// rgpu_bm25_compute_weight, rgpu_bm25_term_weights, rgpu_norms_from_lucene53, rgpu_live_docs_from_lucene50, rgpu_terms_open,
// rgpu_terms_close, rgpu_segment_info_from_lucene62, rgpu_commit_from_segments_file, rgpu_compound_entries_from_lucene50,
// rgpu_field_infos_from_lucene60, rgpu_terms_field_stats, rgpu_terms_lookup, rgpu_terms_lookup_positions.
// Uses from rgpu_api.hip itself: fail. It includes host/bm25_similarity.hpp where the single file did: mid-file, in front of its first use.
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

// ---- host helpers: BM25Similarity (no GPU involved) ------------------------------------------------------------
#include "../host/bm25_similarity.hpp"

extern "C" int32_t rgpu_bm25_compute_weight(float k1, float b, int64_t max_doc, int64_t doc_count, int64_t sum_total_term_freq,
                                            const int64_t* doc_freqs, int32_t n_terms, float boost, float* weight_out,
                                            float* idf_out, float* cache_out) {
  if (!doc_freqs || n_terms <= 0 || n_terms > 64) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  rucene::CollectionStatistics cs;
  cs.max_doc = max_doc;
  cs.doc_count = doc_count;
  cs.sum_total_term_freq = sum_total_term_freq;
  rucene::TermStatistics ts[64];
  for (int i = 0; i < n_terms; ++i) ts[i].doc_freq = doc_freqs[i];
  rucene::BM25SimWeight w = rucene::BM25Similarity(k1, b).compute_weight(cs, ts, (size_t)n_terms, boost);
  if (weight_out) *weight_out = w.weight;
  if (idf_out) *idf_out = w.idf;
  if (cache_out) std::memcpy(cache_out, w.cache.data(), 256 * sizeof(float));
  return RGPU_OK;
}

extern "C" int32_t rgpu_bm25_term_weights(int64_t max_doc, int64_t doc_count, const int64_t* doc_freqs, int64_t n, float boost,
                                          float* weights_out) {
  if (!doc_freqs || !weights_out || n < 0) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  rucene::CollectionStatistics cs;
  cs.max_doc = max_doc;
  cs.doc_count = doc_count;
  for (int64_t i = 0; i < n; ++i) {
    rucene::TermStatistics ts;
    ts.doc_freq = doc_freqs[i];
    weights_out[i] = rucene::BM25Similarity::idf(&ts, 1, cs) * boost;  // BM25SimWeight::weight = idf * boost
  }
  return RGPU_OK;
}

extern "C" int32_t rgpu_norms_from_lucene53(const uint8_t* nvm, size_t nvm_len, const uint8_t* nvd, size_t nvd_len,
                                            int32_t field_number, int32_t max_doc, uint8_t* norms_out) {
  std::string why;
  const int rc = rucene::read_lucene53_norms(nvm, nvm_len, nvd, nvd_len, field_number, max_doc, norms_out, &why);
  return rc == 0 ? RGPU_OK : fail(rc, why);
}

extern "C" int32_t rgpu_live_docs_from_lucene50(const uint8_t* liv, size_t liv_len, int32_t max_doc, int32_t del_count,
                                                uint64_t* words_out) {
  std::string why;
  const int rc = rucene::read_lucene50_live_docs(liv, liv_len, max_doc, del_count, words_out, &why);
  return rc == 0 ? RGPU_OK : fail(rc, why);
}

// ---- term dictionary (host) --------------------------------------------------------------------------------------------
struct rgpu_terms {
  std::unique_ptr<rucene::TermDictionary> dict;
};
static_assert(sizeof(rucene::TermState) == sizeof(rgpu_term_state) && offsetof(rucene::TermState, doc_freq) == offsetof(rgpu_term_state, doc_freq) &&
                  offsetof(rucene::TermState, skip_offset) == offsetof(rgpu_term_state, skip_offset),
              "rucene::TermState must mirror rgpu_term_state");
static_assert(sizeof(rucene::TermFieldStats) == sizeof(rgpu_field_stats), "rucene::TermFieldStats must mirror rgpu_field_stats");

extern "C" int32_t rgpu_terms_open(const uint8_t* tim, size_t tim_len, const uint8_t* tip, size_t tip_len, const rgpu_field_info* infos,
                                   int32_t n_infos, int32_t max_doc, rgpu_terms** out_terms) {
  if (!out_terms) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "out_terms is null");
  *out_terms = nullptr;
  if (n_infos < 0 || (n_infos > 0 && !infos)) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad field infos");
  std::vector<rucene::TermFieldInfo> fi((size_t)n_infos);
  for (int32_t i = 0; i < n_infos; ++i) fi[i] = rucene::TermFieldInfo{infos[i].number, infos[i].index_options, infos[i].has_payloads};  // .flags is informational
  std::string why;
  auto h = std::make_unique<rgpu_terms>();
  int rc;
  try {
    rc = rucene::TermDictionary::open(tim, tim_len, tip, tip_len, fi.data(), n_infos, max_doc, &h->dict, &why);
  } catch (const std::bad_alloc&) {
    return fail(RGPU_ERR_RUNTIME, "out of host memory while building the term dictionary");
  }
  if (rc != 0) return fail(rc, why);
  *out_terms = h.release();
  return RGPU_OK;
}

extern "C" void rgpu_terms_close(rgpu_terms* terms) { delete terms; }

extern "C" int32_t rgpu_segment_info_from_lucene62(const uint8_t* si, size_t si_len, const uint8_t* expected_id16_or_null, rgpu_segment_info* out) {
  if (!out) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "out is null");
  rucene::SegmentInfoEntry e;
  std::string why;
  const int rc = rucene::read_lucene62_segment_info(si, si_len, expected_id16_or_null, &e, &why);
  if (rc != 0) return fail(rc, why);
  *out = rgpu_segment_info{};
  out->max_doc = e.max_doc;
  out->is_compound_file = e.is_compound_file ? 1 : 0;
  for (int i = 0; i < 3; ++i) out->version[i] = e.version[i];
  out->n_files = e.n_files;
  out->n_sort_fields = e.n_sort_fields;
  std::memcpy(out->id, e.id, 16);
  return RGPU_OK;
}

extern "C" int32_t rgpu_commit_from_segments_file(const uint8_t* data, size_t len, int64_t generation, rgpu_commit_segment* out, int32_t cap) {
  std::vector<rucene::CommitSegmentEntry> segs;
  std::string why;
  const int rc = rucene::read_segments_file(data, len, generation, &segs, &why);
  if (rc != 0) return fail(rc, why);
  for (size_t i = 0; i < segs.size() && out && (int64_t)i < cap; ++i) {
    const rucene::CommitSegmentEntry& s = segs[i];
    if (s.name.size() >= sizeof(out[i].name) || s.codec.size() >= sizeof(out[i].codec)) return fail(RGPU_ERR_UNSUPPORTED, "segment or codec name too long");
    out[i] = rgpu_commit_segment{};
    std::memcpy(out[i].name, s.name.c_str(), s.name.size());
    std::memcpy(out[i].codec, s.codec.c_str(), s.codec.size());
    std::memcpy(out[i].id, s.id, 16);
    out[i].del_gen = s.del_gen;
    out[i].field_infos_gen = s.field_infos_gen;
    out[i].dv_gen = s.dv_gen;
    out[i].del_count = s.del_count;
  }
  return (int32_t)segs.size();
}

extern "C" int32_t rgpu_compound_entries_from_lucene50(const uint8_t* cfe, size_t cfe_len, const uint8_t* cfs_or_null, size_t cfs_len,
                                                       const uint8_t* expected_id16_or_null, rgpu_compound_entry* out, int32_t cap) {
  std::vector<rucene::CompoundEntry> entries;
  std::string why;
  const int rc = rucene::read_lucene50_compound_entries(cfe, cfe_len, cfs_or_null, cfs_len, expected_id16_or_null, &entries, &why);
  if (rc != 0) return fail(rc, why);
  for (size_t i = 0; i < entries.size() && out && (int64_t)i < cap; ++i) {
    if (entries[i].id.size() >= sizeof(out[i].id)) return fail(RGPU_ERR_UNSUPPORTED, "compound entry name too long");
    out[i] = rgpu_compound_entry{};
    std::memcpy(out[i].id, entries[i].id.c_str(), entries[i].id.size());
    out[i].offset = entries[i].offset;
    out[i].length = entries[i].length;
  }
  return (int32_t)entries.size();
}

extern "C" int32_t rgpu_field_infos_from_lucene60(const uint8_t* fnm, size_t fnm_len, rgpu_field_info* infos_out, int32_t cap, char* names_out,
                                                  size_t names_cap, size_t* names_len_out) {
  std::vector<rucene::FieldInfoEntry> infos;
  std::string why;
  const int rc = rucene::read_lucene60_field_infos(fnm, fnm_len, &infos, &why);
  if (rc != 0) return fail(rc, why);
  size_t names_len = 0;
  for (size_t i = 0; i < infos.size(); ++i) {
    const rucene::FieldInfoEntry& fi = infos[i];
    if (infos_out && (int64_t)i < cap)
      infos_out[i] = rgpu_field_info{fi.number, fi.index_options, fi.store_payloads ? 1 : 0,
                                     (fi.omit_norms ? 1 : 0) | (fi.store_term_vector ? 2 : 0) | (fi.doc_values_type << 8)};
    if (names_out && names_len + fi.name.size() + 1 <= names_cap) std::memcpy(names_out + names_len, fi.name.c_str(), fi.name.size() + 1);
    names_len += fi.name.size() + 1;
  }
  if (names_len_out) *names_len_out = names_len;
  return (int32_t)infos.size();
}

extern "C" int32_t rgpu_terms_field_stats(const rgpu_terms* terms, int32_t field_number, rgpu_field_stats* out) {
  if (!terms || !out) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "null argument");
  const rucene::TermFieldStats* st = terms->dict->field_stats(field_number);
  if (!st) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "no such indexed field in this segment");
  std::memcpy(out, st, sizeof(*out));
  return RGPU_OK;
}

static int32_t terms_lookup_impl(const rgpu_terms* terms, int32_t field_number, const uint8_t* term_bytes, const int64_t* term_offsets,
                                 int32_t n_terms, rgpu_term_state* states_out, rgpu_term_positions* positions_out, uint8_t* found_out) {
  if (!terms || n_terms < 0 || (n_terms > 0 && (!term_offsets || !states_out))) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "null argument");
  for (int32_t i = 0; i < n_terms; ++i)
    if (term_offsets[i] < 0 || term_offsets[i + 1] < term_offsets[i]) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "term_offsets must be non-decreasing");
  static const uint8_t kEmpty = 0;
  if (n_terms > 0 && term_offsets[n_terms] > term_offsets[0] && !term_bytes) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "term_bytes is null");
  static_assert(sizeof(rucene::TermState) == sizeof(rgpu_term_state), "layout");
  static_assert(sizeof(rucene::TermPositions) == sizeof(rgpu_term_positions), "layout");
  terms->dict->lookup_batch(field_number, term_bytes ? term_bytes : &kEmpty, term_offsets, n_terms,
                            reinterpret_cast<rucene::TermState*>(states_out), found_out,
                            reinterpret_cast<rucene::TermPositions*>(positions_out));
  return RGPU_OK;
}

extern "C" int32_t rgpu_terms_lookup(const rgpu_terms* terms, int32_t field_number, const uint8_t* term_bytes, const int64_t* term_offsets,
                                     int32_t n_terms, rgpu_term_state* states_out, uint8_t* found_out) {
  return terms_lookup_impl(terms, field_number, term_bytes, term_offsets, n_terms, states_out, nullptr, found_out);
}

extern "C" int32_t rgpu_terms_lookup_positions(const rgpu_terms* terms, int32_t field_number, const uint8_t* term_bytes,
                                               const int64_t* term_offsets, int32_t n_terms, rgpu_term_state* states_out,
                                               rgpu_term_positions* positions_out, uint8_t* found_out) {
  if (n_terms > 0 && !positions_out) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "positions_out is null");
  return terms_lookup_impl(terms, field_number, term_bytes, term_offsets, n_terms, states_out, positions_out, found_out);
}

