"""The norm-spectrum fixtures of tests/norm_spectrum.py, proven on the CPU before a GPU sees them: for every spectrum the builder's
own rules hold (they are asserted while it builds), the oracle's TERM rows of the planted lists are the float64 ranking of the
plants, every score the oracle returns is finite, and the f32 numpy scoring gives the oracle's score bits."""
import numpy as np
import pytest

import norm_spectrum as ns


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


@pytest.mark.parametrize("name", ns.SPECTRA)
def test_spectrum_holds_the_bytes_it_names(name):
    sp = ns.spectrum(name)
    present = np.unique(sp.norms)
    assert present.tolist() == sorted(ns.BYTES[name])
    assert present.size == {"one": 1, "extremes": 2, "rank64": 64, "raw65": 65, "all256": 256}[name]
    assert sp.rank_mode == (present.size <= 64)
    assert present.max() > 127
    if name == "rank64":  # ranks 0..63 all used, the planted winners on 63, 62, 33, 32
        ranks = np.searchsorted(present, sp.norms[sp.plants[ns.PLANTED][1][:sp.n_winners(ns.PLANTED)]])
        assert set(ranks.tolist()) == {63, 62, 33, 32}
    dfs = sp.seg.terms["doc_freq"]
    assert dfs[ns.PLANTED] >= 128 * 300 + 1 and dfs[ns.PLANTED] % 128 and dfs[ns.EVERY_DOC] == ns.MAX_DOC
    assert dfs[ns.ABSENT] == 0 and dfs[ns.SINGLETON] == 1 and dfs[ns.BELOW_DENSITY] < ns.MAX_DOC // 64 < dfs[ns.ABOVE_DENSITY]


@pytest.mark.parametrize("version", [1, 0], ids=["bp128", "legacy"])
@pytest.mark.parametrize("name", ns.SPECTRA)
def test_planted_rows_are_the_float64_ranking(oracle, name, version):
    sp = ns.spectrum(name, version)
    osr = oracle.Searcher([sp.oracle_segment(oracle)])
    for term in (ns.PLANTED, ns.CROSSED):
        nw = sp.n_winners(term)
        rank = sp.ranking(term)
        assert rank.size == nw + 1
        for k in (1, nw, nw + 1):
            d, s, total = osr.search(oracle.OP_TERM, [term], k, tie_mode=oracle.TIE_CANONICAL)
            assert total == sp.lists[term][0].size and d.size == k
            assert (d == rank[:k]).all(), (name, term, k, d, rank[:k])
            assert np.isfinite(s).all() and (s > 0).all()
            wd, ws = sp.term_rows_f32(term, k)
            assert (wd == d).all() and (ws.view(np.int32) == s.view(np.int32)).all(), (name, term, k)


@pytest.mark.parametrize("name", ns.SPECTRA)
def test_every_list_scores_finite_and_as_the_f32_model(oracle, name):
    """Every list of the spectrum, k = 300: finite scores, sorted rows, and the numpy f32 scoring's doc ids and score bits (the
    byte-0 lists reach scores near 1e-17, the random lists every byte of the spectrum)."""
    sp = ns.spectrum(name)
    osr = oracle.Searcher([sp.oracle_segment(oracle)])
    for term in range(ns.N_TERMS):
        d, s, total = osr.search(oracle.OP_TERM, [term], 300, tie_mode=oracle.TIE_CANONICAL)
        assert total == sp.lists[term][0].size and d.size == min(300, total)
        assert np.isfinite(s).all() and (s > 0).all() and (np.diff(s) <= 0).all()
        wd, ws = sp.term_rows_f32(term, 300)
        assert (wd == d).all() and (ws.view(np.int32) == s.view(np.int32)).all(), (name, term)
    if sp.roles["BG"] == 0:
        d, s, _ = osr.search(oracle.OP_TERM, [ns.ZERO_DEEP], 300, tie_mode=oracle.TIE_CANONICAL)
        assert s[-1] < 1e-15 and s[0] > 1e-3   # the row reaches from ordinary scores down into byte 0's


@pytest.mark.parametrize("name", ns.SPECTRA)
def test_conjunction_with_the_every_doc_list_keeps_the_plants_apart(oracle, name):
    """The AND / OR of a planted list and the every-doc list (what the GPU module ranks in float64): the gap rules hold on the
    summed scores, and the oracle's conjunction rows are that ranking."""
    sp = ns.spectrum(name)
    osr = oracle.Searcher([sp.oracle_segment(oracle)])
    extra = lambda docs: sp.term_score_f64(ns.EVERY_DOC, docs)
    for term in (ns.PLANTED, ns.CROSSED):
        rank = sp.ranking(term, extra=extra)
        nw = sp.n_winners(term)
        for op in (oracle.OP_AND, oracle.OP_OR):
            d, s, _ = osr.search(op, [term, ns.EVERY_DOC], nw, tie_mode=oracle.TIE_CANONICAL)
            assert (d == rank[:nw]).all() and np.isfinite(s).all(), (name, term, op)


def test_positions_segment_matches_the_oracle_writer(oracle):
    """The positions field over a spectrum's norms: phrases match somewhere, scores are finite."""
    import rucene_amd
    sp = ns.spectrum("all256")
    seg, phrases, doc_count, sum_ttf = sp.positions()
    leaf = rucene_amd.LeafReader.from_synthetic_positions(seg)
    ix = oracle.PositionsIndex.from_files(seg.doc_bytes, seg.pos_bytes, seg.terms, leaf.term_positions)
    matched = 0
    for terms, slop in phrases:
        d, s, total = ix.phrase_search(terms, 10, sp.norms, ns.MAX_DOC, doc_count, sum_ttf, slop=slop)
        assert np.isfinite(s).all()
        matched += total > 0
    assert matched >= len(phrases) - 2
    ix.close()
