"""The bit-spectrum fixture of tests/bit_spectrum.py, proven on the CPU before a GPU sees it: for BP128 and legacy .doc files the
FullBlocks it wrote cover every cell the GPU module relies on (a cell missing here is a failure here, not a silent gap there), the
oracle decodes every list back to the arrays it was built from, and the top k of every query the GPU module asks is, in float64,
a relative GAP apart or a full tie that doc ids resolve. The same for the decode-only WIDE segment (max_doc 2^31 - 1: doc widths
28..31 and the 4-byte all-equal doc VInt; no width is left out; building it takes about 4 GB of host memory for a few seconds)
and for the positions segment, whose position-delta blocks take widths 0 (1- and 2-byte VInt) and 1..N, N = 31: positions are
i32, so a block's 128 deltas sum below 2^31 and one of them can need 31 bits."""
import numpy as np
import pytest

import bit_spectrum as bs

VERSIONS = [1, 0]


@pytest.fixture(scope="module")
def fx():
    import __graft_entry__ as g
    g.build()
    return bs.search_fixture()


@pytest.mark.parametrize("version", VERSIONS, ids=["bp128", "legacy"])
def test_every_cell_is_there(fx, version):
    cells = fx.cells[version]
    have, want = bs.cell_sets(cells), bs.wanted_sets()
    for name in want:
        assert want[name] <= have[name], (name, sorted(want[name] - have[name]))
    assert len(want["doc_width_x_mis"]) == 28 * 16 and len(want["freq_width_x_mis"]) == 32 * 16 and len(want["pairs"]) == 169
    # the 5-byte all-equal freq VInt whose fifth byte is the last byte staged, by what stands in front of it
    fifth = cells[(cells["bf"] == 0) & (cells["fvl"] == 5)]
    q = fifth["mis"] + 2 + np.where(fifth["bd"] > 0, 16 * fifth["bd"], fifth["dvl"])
    assert ((q + 4) % 16 == 0).sum() >= 5 and fifth.size >= 16
    # both versions frame the same blocks at the same bytes
    assert (fx.cells[1] == fx.cells[0]).all()
    # the lists serve search too: a chunk edge crossed, tails, either side of the bitmap density
    dfs = fx.seg[version].terms["doc_freq"]
    assert (dfs[:fx.n_long] > 128 * 130).all() and dfs[fx.dense] > bs.MAX_DOC // 64 and (dfs[fx.steered] < bs.MAX_DOC // 64).all()
    assert sum(int(dfs[t]) % 128 > 0 for t in fx.steered) > len(fx.steered) // 2
    for t in range(fx.n_long):   # spectrum blocks on both sides of the edge between blocks 63 and 64
        assert {63, 64} <= set(fx.info[t]["blocks"])


def test_a_dropped_width_is_noticed(fx):
    cells = fx.cells[1]
    assert "doc_width_x_mis" in bs.missing_cells(cells[cells["bd"] != 19])
    assert "freq_width_x_mis" in bs.missing_cells(cells[cells["bf"] != 1])
    assert "fifth_byte_last_staged" in bs.missing_cells(cells[~((cells["fvl"] == 5) & (cells["mis"] == 10))])


@pytest.mark.parametrize("version", VERSIONS, ids=["bp128", "legacy"])
def test_oracle_decodes_every_list(fx, oracle, version):
    seg = fx.seg[version]
    oseg = oracle.Segment(seg.doc_bytes, seg.norms, bs.MAX_DOC, seg.terms, sum_total_term_freq=bs.STTF)
    for t, (docs, freqs) in enumerate(fx.lists):
        d, f = oseg.decode_term(seg.terms[t])
        assert d.size == docs.size and (d == docs).all() and (f == freqs).all(), t


def test_norms_keep_rank_mode_and_noise_below_everything(fx):
    present = np.flatnonzero(np.bincount(fx.norms, minlength=256))
    assert present.size <= 64 and present[0] == bs.NOISE and present[1] == bs.BG
    assert bs.unit_score(2 ** 31 - 1, bs.NOISE) * (1 + bs.GAP) < bs.unit_score(1, bs.BG)
    # an ordinary doc of a steered or long term is in no other steered or long list
    owners = np.zeros(bs.MAX_DOC, np.uint8)
    for t in list(range(fx.n_long)) + fx.steered:
        d = fx.lists[t][0]
        owners[d[fx.norms[d] != bs.NOISE]] += 1
    assert owners.max() == 1


@pytest.mark.parametrize("k", [10, 100])
def test_top_k_of_every_query_is_apart_or_a_full_tie(fx, oracle, k):
    n = 0
    for op, pos, neg in fx.queries(oracle):
        fx.check_separation(op == oracle.OP_AND, pos, neg, k)
        n += 1
    assert n > len(fx.lists) + 40


def test_plants_inside_extreme_blocks_win(fx, oracle):
    """In the steered and long terms the posting of the largest freq of every spectrum block is among the term's first rows."""
    for t in list(range(fx.n_long)) + fx.steered:
        docs, _ = fx.check_separation(False, [t], [], 100)
        plants = fx.info[t]["plants"]
        assert np.isin(plants, docs[:plants.size]).all(), t


# ---- the WIDE segment ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", VERSIONS, ids=["bp128", "legacy"])
def test_wide_segment_has_doc_widths_28_to_31_and_the_four_byte_doc_vint(oracle, version):
    import __graft_entry__ as g
    g.build()
    w = bs.wide_fixture()
    cells = w.cells[version]
    assert bs.wide_wanted() <= bs.wide_cell_set(cells), sorted(bs.wide_wanted() - bs.wide_cell_set(cells), key=str)
    assert len(bs.wide_wanted()) == 10 and bs.WIDE_DOC_WIDTHS == (28, 29, 30, 31)
    assert bs.wide_wanted() - bs.wide_cell_set(cells[cells["bd"] != 31]) == {(31, "packed"), (31, "equal")}
    for shape in bs.WIDE_DOC_WIDTHS:   # as a term's first block and behind another one
        assert {0, 1} <= set(cells["block"][cells["bd"] == shape].tolist())
    assert set(cells["fvl"][(cells["bf"] == 0) & (cells["bd"] >= 28)].tolist()) == {1, 2, 3, 4, 5}
    seg = w.seg[version]
    oseg = oracle.Segment(seg.doc_bytes, None, bs.WIDE_MAX_DOC, seg.terms)
    for t, (docs, freqs) in enumerate(w.lists):
        d, f = oseg.decode_term(seg.terms[t])
        assert d.size == docs.size and (d == docs).all() and (f == freqs).all(), t


# ---- positions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", VERSIONS, ids=["bp128", "legacy"])
def test_position_blocks_take_every_width(oracle, version):
    import __graft_entry__ as g
    import rucene_amd
    g.build()
    p = bs.positions_fixture()
    cells = p.cells[version]
    first = cells[cells["term"] == p.FIRST]
    assert bs.POS_MAX_WIDTH == 31
    assert set(zip(first["b"].tolist(), first["vl"].tolist())) == set(bs.POS_SHAPES) and len(bs.POS_SHAPES) == 33
    assert [(int(c["b"]), int(c["vl"])) for c in first] == p.shapes   # a doc of FIRST is one block of the shape it was given
    assert len(set(first["mis"].tolist())) >= 8
    seg = p.seg[version]
    assert int(seg.terms["total_term_freq"][p.FIRST]) % 128 == 5   # ... and a VInt block at the end
    leaf = rucene_amd.LeafReader.from_synthetic_positions(seg)
    ix = oracle.PositionsIndex.from_files(seg.doc_bytes, seg.pos_bytes, seg.terms, leaf.term_positions)
    for t, pl in enumerate(p.postings):
        got = [(d, ps) for d, _, ps in ix.iterate(t)]
        assert [d for d, _ in got] == [d for d, _ in pl] and all(list(a[1]) == b[1] for a, b in zip(got, pl)), t
    totals = [ix.phrase_search(terms, 10, p.norms, bs.POS_MAX_DOC, p.doc_count, p.sum_ttf, slop=slop)[2] for terms, slop in p.phrases]
    assert totals[0] == len(p.postings[0]) and totals[2] < totals[4] == len(p.postings[2]) and sum(t > 0 for t in totals) >= 7
    ix.close()
