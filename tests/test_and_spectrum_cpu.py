"""The fixtures of tests/and_spectrum.py, proven on the CPU before a GPU sees them: every list and query has the property it is named
for - read back from the built `.doc` bytes with the oracle, BP128 and legacy -, the models of the kernel's bookkeeping (survivor
queue, directory windows, find_block_wave, the block-decode count) hold their own invariants, and for every query of the suite
the oracle's rows are AndRef's - hit sets by set algebra, scores as f32 sums in ConjunctionScorer's order - bit for bit."""
import itertools

import numpy as np
import pytest

import and_spectrum as as_
from and_spectrum import (ABSENT, BLOCK, C_512, C_1172, C_2344, CONST, CORE_LEAD, EDGE_LEAD, EQ_A, EQ_B, EQ_C, EVERY, FP_LEAD,
                          LEAD_127, LEAD_128, MAX_DOC, OVF_CAP, OVF_OVER, OVF_SMALL, Q_C1, Q_LEAD, REG4, S_C1, S_LEAD, SAME_LEAD, SING_EVEN, SING_MISS,
                          SING_ODD, SPREAD, SPREAD_NOTAIL, T_C1, TAIL_2, WIN_LEAD, Query)

VARIANTS = [("rank", "none", 1), ("rank", "seeded", 1), ("raw", "none", 0), ("raw", "seeded", 1), ("none", "seeded", 0), ("none", "none", 1)]
CPU_KS = (1, 10, 129, 300)


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


def _at(leaf, t, doc):
    """Posting index of a doc in a list."""
    d = leaf.lists[t][0]
    i = int(np.searchsorted(d, doc))
    assert d[i] == doc
    return i


def test_the_constants_are_the_kernels():
    """The thresholds the fixtures straddle, read from the sources they were taken from: a constant that moves there fails here."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rucene_amd", "csrc")
    read = lambda *p: open(os.path.join(csrc, *p)).read()   # noqa: E731
    kernel, bitmap, api = read("kernels", "search_and.hpp"), read("kernels", "doc_bitmap.hpp"), read("rgpu_api.hip")
    num = lambda text, pattern: int(re.search(pattern, text).group(1))   # noqa: E731
    assert num(kernel, r"#define RGPU_AND_G (\d+)") == as_.AND_G == 4
    assert "constexpr int AND_Q_CAP = 128 + 128 * AND_G;" in kernel and as_.AND_Q_CAP == 128 + 128 * as_.AND_G == 640
    assert "constexpr uint32_t AND_Q_FREQ_LIMIT = 1u << 20;" in kernel and as_.AND_Q_FREQ_LIMIT == 1 << 20
    assert 32 * num(kernel, r"constexpr int AND_FILTER_WORDS = (\d+);") == as_.FILTER_BITS == 2048
    assert "blk - lw0 > 63 - AND_G" in kernel and num(kernel, r"#define RGPU_AND_WG_WAVES (\d+)") == 4
    assert num(bitmap, r"constexpr int BITMAP_OVF_CAP = (\d+);") == as_.BITMAP_OVF_CAP == 4096
    assert num(bitmap, r"#define RGPU_NIBBLE_DENSITY (\d+)") == as_.NIBBLE_DENSITY == 128
    assert num(api, r"constexpr int64_t MEMB_ONLY_MIN_DF = (\d+);") == as_.MEMB_MIN_DF == 512
    assert "const int64_t den = d == 0 ? 256 : d;" in api and "state.doc_freq >= 128" in api and as_.MEMB_MIN_LEAD == 128
    assert "64 * 4 / AND_WG_WAVES" in api and as_.XCD_ROUND_ITEMS == 8 * 64 * 4 == 2048       # chunks of 64 workgroups of 4 wavefronts, 8 XCDs
    assert "std::max<int64_t>(8, (lead_blocks + RGPU_AND_TARGET_ITEMS - 1) / RGPU_AND_TARGET_ITEMS)" in api and as_.AUTO_ITEM_BLOCKS == 8
    assert as_.OVF_FREQ == 255 and "f >= 255u" in bitmap


def test_the_leaf_has_the_four_doc_freq_ranges():
    assert 131072 < MAX_DOC <= 1 << 24 and MAX_DOC % 32 == 7
    assert as_.BITMAP_MIN_DF == max(1024, -(-MAX_DOC // 256)) == 1172 and as_.NIB_MIN_DF == 2344
    assert (as_.NIB_MIN_DF - 1) * 128 < MAX_DOC <= as_.NIB_MIN_DF * 128
    assert as_.MEMB_MIN_DF < as_.BITMAP_MIN_DF < as_.NIB_MIN_DF < MAX_DOC
    leaf = as_.Leaf()
    assert [leaf.df(t) for t in as_.KINDS] == [511, 512, 1171, 1172, 2343, 2344] == list(as_.KINDS.values())
    assert [leaf.kind(t) for t in as_.KINDS] == ["walked", "memb", "memb", "bitmap", "bitmap", "nib"]
    assert as_.bitmap_min_df(MAX_DOC, 4) == 75002 == leaf.df(REG4) + 1 and as_.bitmap_min_df(MAX_DOC, -1) is None
    # (a quarter of the leaf: REG4 is walked - behind a lead of 128 docs or more its membership bits are asked first)
    assert leaf.kind(REG4) == "nib" and leaf.kind(REG4, 4) == "memb" and leaf.kind(EVERY, 4) == "nib" and leaf.kind(EVERY, -1) == "walked"
    kinds = {}
    for t in range(as_.N_TERMS):
        if leaf.df(t) and leaf.lists[t][0][-1] == MAX_DOC - 1 and leaf.lists[t][0][0] == 0:
            kinds.setdefault(leaf.kind(t), []).append(t)
    assert set(kinds) == {"walked", "memb", "bitmap", "nib"}        # doc 0 and doc max_doc - 1 are held by a list of every kind
    core = as_.core_docs()
    assert core.size == 200 and (np.diff(core) > 0).all() and core[0] == 0 and core[-1] == MAX_DOC - 1
    for t in list(as_.KINDS) + [EQ_A, EQ_B, EQ_C, OVF_SMALL, OVF_CAP, OVF_OVER, EVERY]:
        assert leaf.has[t][core].all() and not leaf.has[t][as_.neigh_docs()].any() or t == EVERY, as_.NAMES[t]
    assert leaf.df(ABSENT) == 0 and [leaf.df(t) for t in (SING_EVEN, SING_ODD, SING_MISS)] == [1, 1, 1]
    assert set(np.flatnonzero(leaf.has[:, 7]).tolist()) == {SING_MISS, EVERY, REG4}      # SING_MISS's doc: in no lead, in no CORE list
    big = as_.Leaf(big=True)
    assert big.full_blocks(as_.EVERY_BIG) == as_.BIG_BLOCKS == 4300 >= 64 + 4096 + 65 and big.tail_n(as_.EVERY_BIG) == 75 and as_.BIG_MAX_DOC % 32
    assert (big.lists[as_.EVERY_BIG][1] == 1).all() and big.seg.doc_bytes.size < 1 << 17      # small in bytes: all-equal blocks


@pytest.mark.parametrize("version", as_.VERSIONS)
def test_the_doc_bytes_decode_to_the_lists(oracle, version):
    for leaf in (as_.Leaf(version=version), as_.Leaf(version=version, big=True)):
        seg = leaf.oracle_segment(oracle)
        assert seg.version == version
        for t, (d, f) in enumerate(leaf.lists):
            gd, gf = seg.decode_term(leaf.seg.terms[t])
            assert (gd == d).all() and (gf == f).all(), t


def test_host_rules_are_straddled():
    leaf = as_.Leaf()
    q = lambda *m: Query(must=m)   # noqa: E731
    # the clause behind the lead: 511 | 512, bitmap_min_df_and - 1 | bitmap_min_df_and, either side of df * 128 >= max_doc
    assert [as_.wants_memb_only(leaf, q(CORE_LEAD, c)) for c in as_.KINDS] == [False, True, True, False, False, False]
    assert [as_.all_bitmaps_behind_the_lead(leaf, q(CORE_LEAD, c)) for c in as_.KINDS] == [False, False, False, True, True, True]
    # lead df 127 | 128
    assert leaf.df(LEAD_127) == 127 and leaf.full_blocks(LEAD_127) == 0 and leaf.df(LEAD_128) == 128 and leaf.tail_n(LEAD_128) == 0
    assert not as_.wants_memb_only(leaf, q(LEAD_127, C_512)) and as_.wants_memb_only(leaf, q(LEAD_128, C_512))
    assert not as_.wants_memb_only(leaf, q(CORE_LEAD, C_512), -1) and not as_.wants_memb_only(leaf, q(C_512, CORE_LEAD, ABSENT))
    # postings of freq >= 255: 4096 | 4097
    assert leaf.n_overflow(OVF_CAP) == as_.BITMAP_OVF_CAP == 4096 and leaf.n_overflow(OVF_OVER) == 4097
    assert leaf.df(OVF_CAP) == leaf.df(OVF_OVER) >= as_.NIB_MIN_DF
    assert leaf.kind(OVF_CAP) == "nib" and leaf.kind(OVF_OVER) == "walked" and leaf.n_overflow(OVF_SMALL) == 4 and leaf.kind(OVF_SMALL) == "bitmap"
    assert as_.bitmap_terms(leaf, [q(CORE_LEAD, OVF_CAP)]) == (1, 0) and as_.bitmap_terms(leaf, [q(CORE_LEAD, OVF_OVER)]) == (0, 1)
    assert as_.bitmap_terms(leaf, [q(CORE_LEAD, c) for c in as_.KINDS]) == (3, 0) and as_.bitmap_terms(leaf, as_.ALL_QUERIES, -1) == (0, 0)
    assert as_.bitmap_terms(leaf, [Query(must=(EVERY,), must_not=(REG4,)), q(EVERY)]) == (2, 0)       # the lead and a MUST_NOT clause too; not a lone term
    assert as_.bitmap_terms(leaf, as_.ALL_QUERIES, 4) == (1, 0)                                            # a quarter of the leaf: EVERY alone
    dense = [t for t in range(as_.N_TERMS) if leaf.df(t) >= as_.BITMAP_MIN_DF]
    assert as_.bitmap_terms(leaf, as_.ALL_QUERIES) == (len(dense) - 1, 1) and OVF_OVER in dense


def test_bitmap_probe_candidates():
    leaf = as_.Leaf()
    core, neigh = as_.core_docs(), as_.neigh_docs()
    lead = leaf.lists[EDGE_LEAD][0]
    assert set(lead.tolist()) == set(core.tolist()) | set(neigh.tolist()) and leaf.full_blocks(EDGE_LEAD) == 1 and leaf.tail_n(EDGE_LEAD) > 0
    for t in (C_512, C_1172, C_2344):          # membership bits alone, a bitmap, a bitmap with the four-bit array
        held = lead[leaf.has[t][lead]]
        assert set(held.tolist()) == set(core.tolist())
        assert {0, 31} <= set((held % 32).tolist()) and {0, 7} <= set((held % 8).tolist())      # bit 0 and bit 31, nibble 0 and nibble 7
        assert held[0] == 0 and held[-1] == MAX_DOC - 1 and (MAX_DOC - 1) // 32 == (MAX_DOC + 31) // 32 - 1 and (MAX_DOC - 1) % 32 < 31
        for d in neigh:                          # absent from the word (and the four-bit word) that holds its neighbour
            assert not leaf.has[t][d] and leaf.has[t][d - 1] and d // 32 == (d - 1) // 32 and d // 8 == (d - 1) // 8
    assert neigh.size >= 20
    # the four-bit array: freq 14 | 15 in one lane's two slots; a vector without a 15 takes the short way
    d, f = leaf.lists[C_2344]
    i14, i15 = (_at(leaf, CORE_LEAD, core[i]) for i in as_.NIB_PLANTS)
    assert (f[_at(leaf, C_2344, core[30])], f[_at(leaf, C_2344, core[31])]) == (14, 15) and (i14, i15) == (30, 31) and i14 // 2 == i15 // 2 and i15 < BLOCK
    assert (np.delete(f, [_at(leaf, C_2344, core[31])]) <= 14).all()
    tail = leaf.lists[CORE_LEAD][0][BLOCK:]
    assert tail.size == 12 and tail[-1] == MAX_DOC - 1 and leaf.has[C_2344][tail].all()
    # the freq bytes: 254 | 255 | 256, the overflow list's first and last posting hold 255, two overflow hits in one lane
    for t in (OVF_SMALL, OVF_CAP, OVF_OVER):
        d, f = leaf.lists[t]
        got = {i: int(f[_at(leaf, t, core[i])]) for i in as_.OVF_PLANTS}
        assert got == as_.OVF_PLANTS == {20: 255, 21: 256, 40: 254, 60: 300, 100: 255}
        ovf = np.flatnonzero(f >= 255)
        assert f[ovf[0]] == 255 and f[ovf[-1]] == 255 and (t != OVF_SMALL or (d[ovf[0]], d[ovf[-1]]) == (core[20], core[100]))
        at = [_at(leaf, CORE_LEAD, core[i]) for i in (20, 21)]
        assert at == [20, 21] and at[0] // 2 == at[1] // 2 and at[0] % 2 == 0       # slot 0 and slot 1 of lane 10
    assert leaf.kind(OVF_CAP) == "nib" and leaf.kind(OVF_SMALL) == "bitmap"         # a code of 15 first, and straight to the freq bytes


def test_batched_probe_groups_and_the_queue():
    leaf = as_.Leaf()
    assert as_.AND_Q_CAP == 640 and as_.AND_G == 4
    # lead FullBlocks per item of 1, 2, 3, 4, 5, 7, 8 and 9: the last group of an item holds 1, 2, 3 or 4 blocks
    per_item = []
    for t, n in as_.G_LEADS.items():
        assert leaf.full_blocks(t) == n and leaf.tail_n(t) == (3 if n % 2 else 0) and leaf.df(t) < leaf.df(as_.G_C1) and leaf.kind(as_.G_C1) == "bitmap"
        (tr,) = as_.queue_trace(leaf, t, as_.G_C1, 200)
        assert sum(tr["blocks"]) == n and sum(tr["survivors"]) == int(leaf.has[as_.G_C1][leaf.lists[t][0][:n * BLOCK]].sum()) == n * BLOCK // 2
        per_item.append(n)
    assert per_item == [1, 2, 3, 4, 5, 7, 8, 9] and {n % 4 for n in per_item} == {0, 1, 2, 3}
    assert [sum(tr["blocks"]) for tr in as_.queue_trace(leaf, as_.G_9, as_.G_C1, 3)] == [3, 3, 3]
    # a lead whose last item is blocks + tail | blocks + nothing
    assert leaf.tail_n(as_.G_9) > 0 and leaf.tail_n(as_.G_8) == 0 and leaf.tail_n(S_LEAD) == 0 and leaf.tail_n(Q_LEAD) == 5
    # 0, 1, 127 and 128 entries waiting; a group with no survivor
    (tr,) = as_.queue_trace(leaf, S_LEAD, S_C1, 200)
    assert tr["survivors"] == list(as_.S_SURVIVORS) and tr["before"] == [0, 0, 0, 1, 127] and tr["after"] == [0, 128, 129, 127, 128]
    assert leaf.df(S_LEAD) == 20 * BLOCK < leaf.df(S_C1)
    # 127 waiting + 512 appended = 639 of 640 cells
    for bpi in (as_.AUTO_ITEM_BLOCKS, 200):
        (tr,) = as_.queue_trace(leaf, Q_LEAD, Q_C1, bpi)
        assert tr["survivors"] == [511, 512] and tr["before"] == [0, 127] and tr["after"] == [511, 639] and max(tr["after"]) == as_.AND_Q_CAP - 1
    assert leaf.full_blocks(Q_LEAD) == 8 and leaf.df(Q_LEAD) < leaf.df(Q_C1) and leaf.kind(Q_C1) == "bitmap"
    missing = leaf.lists[Q_LEAD][0][~leaf.has[Q_C1][leaf.lists[Q_LEAD][0]]]
    assert missing.size == 1 and _at(leaf, Q_LEAD, missing[0]) == as_.Q_MISSING_AT < as_.AND_G * BLOCK
    # a lead freq of 2^20 - 1 | 2^20 in the first group, 2^20 in the third group with survivors queued
    for t, (at, freq) in as_.T_LEADS.items():
        d, f = leaf.lists[t]
        assert f[at] == freq and (np.delete(f, at) <= 10).all() and leaf.has[T_C1][d[at]] and leaf.full_blocks(t) == 12 and leaf.df(t) < leaf.df(T_C1)
        (tr,) = as_.queue_trace(leaf, t, T_C1, 200)
        assert len(tr["blocks"]) == 3 and at // (as_.AND_G * BLOCK) == (2 if t == as_.T_C else 0)
        if t == as_.T_C:
            assert 0 < tr["before"][2] < 128
    assert [fr for _, fr in as_.T_LEADS.values()] == [(1 << 20) - 1, 1 << 20, 1 << 20] == [as_.AND_Q_FREQ_LIMIT - 1] + [as_.AND_Q_FREQ_LIMIT] * 2
    # the lead's directory window: items of 60, 61, 64, 65 and 130 blocks
    assert [leaf.full_blocks(t) for t in as_.W_LEADS] == [60, 61, 64, 65, 130] and all(leaf.tail_n(t) == 0 for t in as_.W_LEADS)
    assert [as_.lead_window_reloads(n, as_.AND_G) for n in as_.W_LEADS.values()] == [0, 1, 1, 1, 2]
    assert [as_.lead_window_reloads(n, 1) for n in as_.W_LEADS.values()] == [0, 1, 1, 1, 2]
    assert all(leaf.df(t) < leaf.df(REG4) and leaf.kind(t) == "nib" for t in as_.W_LEADS)


def test_filter_false_positives_and_block_edges():
    leaf = as_.Leaf()
    sp, lead = leaf.lists[SPREAD][0], leaf.lists[FP_LEAD][0]
    assert leaf.full_blocks(SPREAD) == 2 and leaf.tail_n(SPREAD) == 45 and leaf.kind(SPREAD) == "walked" and leaf.df(FP_LEAD) < leaf.df(SPREAD_NOTAIL)
    spans = [int(sp[(b + 1) * BLOCK - 1] - sp[b * BLOCK]) for b in range(2)]
    assert min(spans) > as_.FILTER_BITS and leaf.full_blocks(FP_LEAD) == 1 and leaf.tail_n(FP_LEAD) > 0
    blk, hit, fp = as_.probe_outcomes(leaf, FP_LEAD, SPREAD)
    assert hit.sum() >= 70 and fp.sum() >= 70 and not (hit & fp).any()
    for d in lead[fp]:
        assert not leaf.has[SPREAD][d] and leaf.has[SPREAD][d - as_.FILTER_BITS]                 # d = e + 2048 for a doc e of the same block
    assert {0, 1} <= set(blk[fp].tolist()) and 2 in set(blk[fp].tolist())                         # in FullBlocks, and in the VInt tail
    assert 2 in set(blk[hit].tolist()) and ((blk == 2) & ~hit & ~fp).any()                        # behind the last FullBlock: the tail holds it | does not
    i = np.arange(lead.size)
    same_lane = [(a, a + 1) for a in i[:-1] if a % 2 == 0 and a // BLOCK == (a + 1) // BLOCK]
    assert any(hit[a] and fp[b] for a, b in same_lane)                                            # a hit and a false positive in one lane's two slots
    assert any(fp[a] and hit[a + 1] for a in i[:-1] if a % 2 == 1 and (a + 1) % BLOCK)            # ... and in neighbouring lanes of one vector
    at = np.array([_at(leaf, SPREAD, d) for d in lead[hit]])
    assert {0, 1} <= set((at % 2).tolist())                                                       # found in slot 0 and in slot 1 of the decoded block
    last0 = int(sp[BLOCK - 1])
    assert leaf.has[FP_LEAD][[last0, last0 + 1]].all() and not leaf.has[SPREAD][last0 + 1]        # a block's last doc and last doc + 1
    assert lead[0] == 1 < sp[0] and not leaf.has[SPREAD][1]                                       # below the first block's first doc
    nblk, nhit, nfp = as_.probe_outcomes(leaf, FP_LEAD, SPREAD_NOTAIL)
    assert leaf.tail_n(SPREAD_NOTAIL) == 0 and (nblk == 2).sum() >= 20 and not nhit[nblk == 2].any()   # behind the last FullBlock, no tail
    # the clause kinds that meet the false positives: MUST (it dies), MUST_NOT (it lives), the VInt tail
    must = as_.ref_docs(leaf, Query(must=(FP_LEAD, SPREAD)))
    nots = as_.ref_docs(leaf, Query(must=(FP_LEAD,), must_not=(SPREAD,)))
    assert set(must.tolist()) == set(lead[hit].tolist()) and set(lead[fp].tolist()) <= set(nots.tolist()) and must.size + nots.size == lead.size
    assert Query(must=(FP_LEAD, SPREAD)) in as_.PLAIN and Query(must=(FP_LEAD,), must_not=(SPREAD,)) in as_.WITH_NOT
    # consecutive lead blocks that land in one clause block: the cursor does not move
    same = leaf.lists[SAME_LEAD][0]
    assert leaf.full_blocks(SAME_LEAD) == 2 and sp[0] <= same[0] and same[-1] <= last0 and leaf.has[SPREAD][same].sum() == 100
    _, _, ev = as_.walked_trace(leaf, Query(must=(SAME_LEAD, SPREAD)))
    assert ev == [] and as_.walked_trace(leaf, Query(must=(SAME_LEAD, SPREAD)))[0] == 2 + 2


def test_register_window_and_find_block_wave():
    leaf = as_.Leaf()
    # the next pending candidate's block 62 | 63 | 64 slots past the window's start
    assert (leaf.lists[REG4][0] == np.arange(as_.REG4_OFF, MAX_DOC, as_.REG4_STEP)).all()
    count, plain, ev = as_.walked_trace(leaf, Query(must=(WIN_LEAD, REG4)))
    assert count == plain == len(as_.WIN_BLOCKS) and [e[3] for e in ev if e[2] == "next"] == [62, 63, 62, 64, 63]
    assert [e[3] for e in ev if e[2] == "find"] == [("first",)] * 3
    assert leaf.kind(REG4, -1) == "walked" and not as_.wants_memb_only(leaf, Query(must=(WIN_LEAD, REG4)), 4) and leaf.df(WIN_LEAD) == 2 * len(as_.WIN_BLOCKS)
    # the big leaf: find_block_wave's first look, its loop entered at hi - lo = 64 | 65, none, one and two rounds, no slot qualifies
    big = as_.Leaf(big=True)
    last = big.dir_last(as_.EVERY_BIG)
    seen, by_lead = set(), {}
    for q in as_.BIG_QUERIES:
        count, plain, ev = as_.walked_trace(big, q)
        finds = [e[3] for e in ev if e[2] == "find"]
        by_lead[as_.BIG_NAMES[q.must[0]]] = finds
        seen.update(finds)
        assert count == plain == big.full_blocks(q.must[0]) * 2 and finds
    loops = [s for s in seen if s[0] == "loop"]
    assert ("first",) in seen and {s[2] for s in loops} == {0, 1, 2} and {64, 65} <= {s[1] for s in loops}
    assert {s[3] for s in loops} == {"final", "none"} and ("loop", 64, 0, "final") in seen and ("loop", 65, 1, "final") in seen
    assert by_lead["B_TAIL_0"][-1][3] == "none" and by_lead["B_0_63"] == by_lead["B_0_126"] == [("first",)]      # 0 and 63 blocks behind `from`
    assert by_lead["B_0_127"][0][2] == 2 and by_lead["B_20_147"][0][2] == 1                                        # 64 behind: two rounds | one round
    assert by_lead["B_0_192"] == [("loop", as_.BIG_BLOCKS - 127, 1, "none")]                                       # a round in which no probe qualifies
    # the port of find_block_wave against a plain search, from every kind of start
    rng = np.random.default_rng(5)
    for frm in (0, 1, 63, 64, 2000, as_.BIG_BLOCKS - 129, as_.BIG_BLOCKS - 128, as_.BIG_BLOCKS - 65, as_.BIG_BLOCKS - 1, as_.BIG_BLOCKS):
        for target in rng.integers(0, as_.BIG_MAX_DOC, size=200):
            want = min(as_.BIG_BLOCKS, max(frm, int(np.searchsorted(last, target, "left"))))
            assert as_.find_block_wave(last, frm, int(target))[0] == want, (frm, target)
    # lead blocks of one item that land thousands of clause blocks apart
    assert ("B_0_%d" % (63 + 64 + 4096)) in by_lead
    # a walked clause at clause positions 1 and 2, and at 62 and 63, of a 64-clause conjunction
    at = set()
    for q in as_.PLAIN:
        if len(q.must) == 64:
            order = [t for t, _ in as_.required(leaf, q)]
            assert order[0] == CORE_LEAD
            at.update(i for i, t in enumerate(order) if i and leaf.kind(t) == "walked")
    assert at == {1, 2, 62, 63}


def test_clause_kinds_and_clause_order(oracle):
    leaf = as_.Leaf()
    lead = leaf.lists[CORE_LEAD][0]
    assert _at(leaf, CORE_LEAD, leaf.lists[SING_EVEN][0][0]) == 10 and _at(leaf, CORE_LEAD, leaf.lists[SING_ODD][0][0]) == 11 and not leaf.has[CORE_LEAD][7]
    assert {Query(must=(CORE_LEAD, C_1172), must_not=(s,)) for s in (SING_EVEN, SING_ODD, SING_MISS)} <= set(as_.WITH_NOT)   # slot 0, slot 1, a miss
    assert as_.lead_of(leaf, Query(must=(EVERY, SING_EVEN))) == SING_EVEN and Query(must=(SING_EVEN, EVERY)) in as_.PLAIN       # a singleton lead
    assert [leaf.df(t) for t in (SING_EVEN, TAIL_2, LEAD_127)] == [1, 2, 127] and lead.size == 140                              # tail-only leads
    assert Query(must=(CORE_LEAD, ABSENT)) in as_.PLAIN and Query(must=(EQ_A, EQ_A)) in as_.PLAIN
    # three clauses of equal doc_freq in all six orders: the stable order is the query's, and the f32 sums differ
    assert leaf.df(EQ_A) == leaf.df(EQ_B) == leaf.df(EQ_C) == 300
    ref = as_.AndRef(oracle, leaf)
    sums = {}
    for p in itertools.permutations((EQ_A, EQ_B, EQ_C)):
        q = Query(must=p)
        assert q in as_.PLAIN and [t for t, _ in as_.required(leaf, q)] == list(p)
        docs, sc = ref.scores(q)
        assert docs.size >= 200
        sums[p] = sc.view(np.int32)
    assert len({s.tobytes() for s in sums.values()}) >= 3                               # (a + b) + c against (a + c) + b against (b + c) + a
    assert as_.required(leaf, Query(must=(C_1172, CORE_LEAD), filt=(EQ_A,))) == [(CORE_LEAD, True), (EQ_A, False), (C_1172, True)]
    assert as_.required(leaf, Query(must=(EQ_B,), filt=(EQ_A,)))[0] == (EQ_B, True) and as_.required(leaf, Query(must=(LEAD_128, LEAD_127)))[0][0] == LEAD_127


@pytest.mark.parametrize("norms", as_.NORMS)
def test_const_ties_across_every_item_edge(oracle, norms):
    leaf = as_.Leaf(norms=norms)
    ref = as_.AndRef(oracle, leaf)
    q = Query(must=(CONST, EVERY))
    docs, sc = ref.scores(q)
    assert docs.tolist() == list(range(as_.CONST_LO, as_.CONST_HI)) and np.unique(sc.view(np.int32)).size == 1 and sc[0] > 0
    assert leaf.full_blocks(CONST) == 8 and leaf.tail_n(CONST) == 76 and [as_.items_of(leaf, q, b) for b in (1, 3, 8, 200)] == [8, 3, 1, 1]
    for k in as_.KS:
        d, s, total = as_.oracle_rows(oracle, ref.osr, [q], k)[0]
        assert total == 1100 and d.tolist() == list(range(as_.CONST_LO, as_.CONST_LO + k))     # every k cuts the tie; from 129 on, past an item edge
    assert q in as_.PLAIN and as_.KS == (1, 10, 64, 65, 128, 129, 300) and max(as_.KS) > 2 * 128


def test_launch_shapes():
    leaf = as_.Leaf()
    assert as_.XCD_ROUND_ITEMS == 2048
    for n in (2047, 2048, 2049, 5000):
        batch = as_.batch_of_items(leaf, n)
        assert sum(as_.items_of(leaf, q, 1) for q in batch) == n and all(q in as_.PLAIN for q in batch) and len(batch) < n
        assert len({q for q in batch}) > 20
    assert as_.items_of(leaf, Query(must=(as_.W_130, EVERY)), 1) == 130 and as_.items_of(leaf, Query(must=(as_.W_130, EVERY)), 200) == 1
    assert as_.items_of(leaf, Query(must=(TAIL_2, EVERY)), 1) == 1 and as_.items_of(leaf, Query(must=(CORE_LEAD, ABSENT)), 1) == 0
    many = [q for q in as_.ALL_QUERIES if as_.items_of(leaf, q, 200) > 1]              # one item per query at 200 blocks per item, but for EVERY as the lead
    assert many == [Query(must=(EVERY,), must_not=(REG4,))]


def test_the_seeded_mask_deletes_what_it_claims():
    leaf = as_.Leaf(live="seeded")
    core = as_.core_docs()
    gone = as_.deleted_for_certain()
    assert not leaf.alive[gone].any() and leaf.alive[as_.alive_for_certain()].all() and 0.8 < leaf.alive.mean() < 0.9
    assert gone[0] % 32 == 0 and gone[1] % 32 == 31                                                  # a candidate at each word edge
    assert leaf.has[EDGE_LEAD][gone[:2]].all() and leaf.has[C_1172][gone[:2]].all()
    blk, hit, fp = as_.probe_outcomes(leaf, FP_LEAD, SPREAD)
    assert hit[_at(leaf, FP_LEAD, gone[2])] and gone[2] == core[0] + 4003                                                          # a real filter hit
    bits = np.unpackbits(leaf.live_docs.view(np.uint8), bitorder="little")
    assert (bits[:MAX_DOC] == leaf.alive).all() and not bits[MAX_DOC:].any() and leaf.live_docs.size == (MAX_DOC + 63) // 64
    assert as_.Leaf().live_docs is None and as_.Leaf().alive.all()


def test_the_families_are_the_ones_named():
    leaf = as_.Leaf()
    assert all(len(q.must) >= 2 and not (q.must_not or q.filt or q.should) for q in as_.PLAIN)
    assert all(q.must and q.must_not and not (q.filt or q.should) for q in as_.WITH_NOT)
    assert all(q.must and q.filt and not (q.must_not or q.should) for q in as_.WITH_FILTER)
    assert all(len(q.must) + len(q.filt) + len(q.must_not) <= 64 and q.msm == 0 for q in as_.ALL_QUERIES)
    assert max(len(q.must) + len(q.must_not) for q in as_.WITH_NOT) == 64
    assert any(as_.required(leaf, q)[0][1] is False for q in as_.WITH_FILTER)         # a FILTER clause leads
    queries, rows = as_.mixed()
    assert sorted(i for r in rows.values() for i in r) == list(range(len(queries))) == list(range(len(as_.ALL_QUERIES)))
    assert all([queries[i] for i in rows[name]] == fam for name, fam in as_.FAMILIES.items())
    kinds = {name: set() for name in as_.FAMILIES}
    for name, fam in as_.FAMILIES.items():
        for q in fam:
            if not as_.matches_nothing(leaf, q):
                kinds[name].update(leaf.kind(t) for t, _ in as_.required(leaf, q)[1:])
                kinds[name].update("not-" + leaf.kind(t) for t in q.must_not)
    assert all({"walked", "memb", "bitmap", "nib"} <= k for k in kinds.values())
    assert {"not-walked", "not-bitmap", "not-nib"} <= kinds["not"]
    hits = [as_.ref_docs(leaf, q).size for q in as_.ALL_QUERIES]
    assert sum(h == 0 for h in hits) < len(hits) // 4 and sum(0 < h < 10 for h in hits) >= 10 and sum(h > 300 for h in hits) >= 40   # fewer hits than k, too


@pytest.mark.parametrize("live", as_.LIVE)
def test_the_decode_count_model(live):
    """blocks_decoded with every clause walked and one item per query: the window model visits exactly the blocks the plain rule
    names, each once and in ascending order, never fewer than the lead's blocks, and only the lead's when nothing survives."""
    leaf = as_.Leaf(live=live)
    total = 0
    for q in as_.ALL_QUERIES:
        count, plain, ev = as_.walked_trace(leaf, q)
        assert count == plain, q
        if as_.matches_nothing(leaf, q):
            assert count == 0
            continue
        lead = as_.lead_of(leaf, q)
        assert count >= leaf.full_blocks(lead)
        rest = [t for t, _ in as_.required(leaf, q)[1:]] + list(q.must_not)
        if all(leaf.df(t) <= 1 for t in rest):
            assert count == leaf.full_blocks(lead)
        total += count
    assert total > 20000
    alive = leaf.lists[LEAD_128][0][leaf.alive[leaf.lists[LEAD_128][0]]]
    assert as_.walked_trace(leaf, Query(must=(LEAD_128, C_512)))[0] == 1 + np.unique(np.searchsorted(leaf.dir_last(C_512), alive)).size


@pytest.mark.parametrize("norms,live,version", VARIANTS, ids=["%s-%s-v%d" % v for v in VARIANTS])
def test_oracle_rows_are_the_numpy_rows(oracle, norms, live, version):
    """Every query of the three families: the oracle's ConjunctionScorer / ReqNotScorer rows against set algebra and f32 sums in
    doc_freq order, bit for bit."""
    leaf = as_.Leaf(norms=norms, live=live, version=version)
    ref = as_.AndRef(oracle, leaf)
    filled = 0
    for k in CPU_KS:
        for name, fam in as_.FAMILIES.items():
            for q, (d, s, total) in zip(fam, as_.oracle_rows(oracle, ref.osr, fam, k)):
                wd, ws, wt = ref.row(q, k)
                assert total == wt == as_.ref_docs(leaf, q).size, (name, q, k, total, wt)
                assert d.size == wd.size == min(k, wt) and (d == wd).all(), (name, q, k, d[:8], wd[:8])
                assert (s.view(np.int32) == ws.view(np.int32)).all(), (name, q, k)
                filled += d.size
    assert filled > 0


def test_the_big_leaf_rows(oracle):
    leaf = as_.Leaf(big=True)
    ref = as_.AndRef(oracle, leaf)
    for k in (10, 300):
        for q, (d, s, total) in zip(as_.BIG_QUERIES, as_.oracle_rows(oracle, ref.osr, as_.BIG_QUERIES, k)):
            wd, ws, wt = ref.row(q, k)
            assert total == wt == leaf.df(q.must[0]) and (d == wd).all() and (s.view(np.int32) == ws.view(np.int32)).all(), q
