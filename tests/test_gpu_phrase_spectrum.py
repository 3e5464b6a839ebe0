"""Phrase parity at every rung of the position-list ladder (`-m gpu`): the fixtures of tests/phrase_spectrum.py (proven on the CPU
by tests/test_phrase_spectrum_cpu.py) through GpuIndexSearcher.search_phrase_batch against the oracle's PositionsIndex.phrase_search -
doc ids, hit counts and score bits equal, nowhere a tolerance.

Every rung case is run as an exact and as a slop-1 phrase, each in a batch of its own, and the kernel statistics of that batch say
which rung answered: 1 / 10 | 11 positions of a term (the 64-candidate kernels | "left by the 64-candidate kernel"), 128 | 129 (the
small | the wide lists), 1024 | 1025 (answered | RGPU_ERR_UNSUPPORTED, after which the context answers the next batch), a sloppy pool
of 256 | 257 and 2048 | 2049, 6 | 7 distinct terms, one to three repetition groups, 16 | 17 terms, a doc's positions ending at value
127 | 128 | 129 of a packed block with a packed, an all-equal, the trailing block or nothing behind, whole blocks to step over,
singleton terms, position - offset on both sides of the 16-bit lists' range. The placement cases run on a legacy segment too, where
the one-candidate kernels answer everything. The collector is met at 8191 .. 16385 candidates with the first match on both sides of
every chunk edge, next_limit on both sides of it, the first chunk deleted, everything deleted, and k on both sides of 64 and 128.
The launches of every batch are printed (`-s` shows them)."""
import os

import numpy as np
import pytest

import phrase_spectrum as ps
from test_gpu_norm_spectrum import _assert_row

pytestmark = pytest.mark.gpu

SEGMENTS = [("freq", 1), ("terms", 1), ("place", 1), ("place", 0)]
IDS = ["%s-%s" % (n, "bp128" if v else "legacy") for n, v in SEGMENTS]


@pytest.fixture(scope="module")
def ctx():
    import rucene_amd
    c = rucene_amd.Context(profile_kernels=True)
    yield c
    c.close()


def _open(oracle, fx, version=1, live_docs=None):
    ix = fx.index(oracle, version)
    return ix, ps.leaf_of(ix, len(fx.postings), fx.norms, fx.max_doc, fx.doc_count, fx.sum_ttf, live_docs=live_docs)


def _gq(q):
    import rucene_amd
    return rucene_amd.PhraseQuery(q.terms, q.positions, slop=q.slop)


def _search(ctx, g, queries, k):
    """One batch -> (hits, totals, {launch name: launches} of this batch)."""
    ctx.kernel_stats_reset()
    hits, totals = g.search_phrase_batch([_gq(q) for q in queries], k)
    return hits, totals, {n: v["launches"] for n, v in ctx.kernel_stats().items() if v["launches"]}


def _same(a, b):
    return (a[1] == b[1]).all() and (a[0]["doc"] == b[0]["doc"]).all() and (a[0]["score"].view(np.int32) == b[0]["score"].view(np.int32)).all()


@pytest.mark.parametrize("name,version", SEGMENTS, ids=IDS)
def test_every_rung_alone(ctx, oracle, name, version):
    """Each case's exact and slop-1 query in a batch of its own: the oracle's row, and the launches the rung's name promises. A
    refused query raises RgpuError with the documented status and leaves the context able to answer the next batch. Then the
    materialising decode of every position of every term of the segment (it has no per-doc cap) against the input."""
    import rucene_amd
    fx = ps.segment(name)
    ix, leaf = _open(oracle, fx, version)
    try:
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
        good = next(q for c in fx.cases for q in c.queries if q.error is None)
        for c in fx.cases:
            for q in c.queries:
                what = (name, version, c.name, "slop", q.slop)
                want = fx.search(ix, q, 10)
                assert want[2] >= 1 and c.designed in fx.search(ix, q, 1000)[0].tolist(), what   # an empty row must not pass for a correct one
                if q.error is not None:
                    with pytest.raises(rucene_amd.RgpuError) as e:
                        g.search_phrase_batch([_gq(q)], 10)
                    assert e.value.status == q.error, (what, e.value.status)
                    print(c.name, "slop", q.slop, "refused with status", e.value.status)
                    hits, totals, st = _search(ctx, g, [good], 10)   # an ordinary error return: the context goes on answering
                    _assert_row(hits[0], totals[0], fx.search(ix, good, 10), (what, "the batch behind the refusal"))
                    continue
                hits, totals, st = _search(ctx, g, [q], 10)
                print(c.name, "slop", q.slop, q.level, st)
                _assert_row(hits[0], totals[0], want, what)
                for launch, wanted in ps.launches(q, legacy=version == 0).items():
                    assert (launch in st) == wanted, (what, q.level, launch, "launched" if launch in st else "not launched", st)
        got = leaf.segment.decode_positions(leaf.terms, leaf.term_positions)
        want = fx.every_position()
        assert got.size == want.size == fx.sum_ttf and (got == want).all(), (name, version)
    finally:
        leaf.segment.close()
        ix.close()


@pytest.mark.parametrize("name,version", SEGMENTS, ids=IDS)
def test_every_rung_in_one_batch_and_the_redo_list_cap(ctx, oracle, name, version):
    """A candidate for every rung of the segment in one mixed batch; then the list of candidates the 64-candidate kernels hand on
    capped at 0 and at 1 entry (the one-candidate kernels then look at every slot): the same rows bit for bit."""
    import rucene_amd
    fx = ps.segment(name)
    ix, leaf = _open(oracle, fx, version)
    try:
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
        mixed = [q for c in fx.cases for q in c.queries if q.error is None]
        assert len(mixed) >= len(fx.cases)
        for k in (10, 129):
            hits, totals, st = _search(ctx, g, mixed, k)
            print(name, version, "mixed batch, k", k, st)
            for i, q in enumerate(mixed):
                _assert_row(hits[i], totals[i], fx.search(ix, q, k), (name, version, "mixed", k, q.terms, q.slop))
        free = _search(ctx, g, mixed, 10)
        for cap in ("0", "1"):
            os.environ["RGPU_PHRASE_REDO_CAP"] = cap
            try:
                capped = _search(ctx, g, mixed, 10)
            finally:
                del os.environ["RGPU_PHRASE_REDO_CAP"]
            print(name, version, "redo list capped at", cap, capped[2])
            assert _same(free, capped), (name, version, cap)
    finally:
        leaf.segment.close()
        ix.close()


# ---- the collector's chunks ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunk_leaves(oracle):
    opened = {}

    def get(n):
        if n not in opened:
            opened[n] = _open(oracle, ps.chunks(n))
        return opened[n]
    yield get
    for ix, leaf in opened.values():
        leaf.segment.close()
        ix.close()


def _check_chunk_rows(fx, ix, queries, hits, totals, k, what, live=None, limit=None):
    for i, q in enumerate(queries):
        _assert_row(hits[i], totals[i], fx.search(ix, q, k, live_docs=live, next_limit=limit), (what, q.terms, q.slop))


@pytest.mark.parametrize("n", ps.CHUNK_NS)
def test_two_phase_cut_off_across_chunks(ctx, oracle, chunk_leaves, n):
    """n candidates, the first phrase match at candidate 0, 8191, 8192, 8193 and n - 1 (a pair of terms each); next_limit one below,
    at and one above that index, 0, n - 1, n and the default: the sloppy phrases yield hits iff at most next_limit candidates precede
    the first collected doc, the exact phrases whatever the limit."""
    import rucene_amd
    fx = ps.chunks(n)
    ix, leaf = chunk_leaves(n)
    limits = sorted({x for j in range(len(fx.first)) for x in fx.limits(j) if x is not None}) + [None]
    unlimited = {}
    cut = kept = 0
    for limit in [None] + limits[:-1]:
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx, next_limit=limit)
        pairs = [j for j in range(len(fx.first)) if limit in fx.limits(j)]
        queries = [q for j in pairs for q in fx.queries(j)]
        hits, totals, st = _search(ctx, g, queries, 10)
        print(n, "next_limit", limit, "pairs", [fx.first[j] for j in pairs], st)
        _check_chunk_rows(fx, ix, queries, hits, totals, 10, (n, "next_limit", limit), limit=limit)
        assert ps.MERGE in st and ps.COLLECT in st, st          # k <= 128: the chunked collector and the fold of its lists
        for row, j in enumerate(j for j in pairs for _ in range(3)):
            q = queries[row]
            yields = q.slop == 0 or fx.first[j] <= (ps.DEFAULT_NEXT_LIMIT if limit is None else limit)
            assert totals[row] == (int(fx.matches[j].sum()) if yields else 0), (n, limit, fx.first[j], q.terms, q.slop, int(totals[row]))
            cut += not yields
            kept += bool(yields and q.slop > 0 and limit is not None)
            if limit is None:
                unlimited[(j, row % 3)] = (hits[row].copy(), totals[row])
            elif q.slop == 0:   # next_limit does not change an exact phrase's row
                assert _same((unlimited[(j, 0)][0], np.asarray(unlimited[(j, 0)][1])), (hits[row], np.asarray(totals[row]))), (n, limit, j)
    assert cut >= 2 and kept >= 2


@pytest.mark.parametrize("n", [ps.CHUNK + 1, 2 * ps.CHUNK + 1])
def test_first_chunk_deleted_and_everything_deleted(ctx, oracle, chunk_leaves, n):
    """Every candidate of the first chunk deleted, the first live one at index 8192: the deleted ones count as approximations
    (next_limit 8191 | 8192 for the pair whose first match is candidate 8192), and a repeated-term phrase's groups come from the
    first LIVE candidate. Every candidate deleted: no hits, no error."""
    import rucene_amd
    fx = ps.chunks(n)
    ix = chunk_leaves(n)[0]
    queries = [q for j in range(len(fx.first)) for q in fx.queries(j)]
    for alive in (np.arange(n) >= ps.CHUNK, np.zeros(n, dtype=bool)):
        live = fx.live_words(alive)
        leaf = ps.leaf_of(ix, len(fx.postings), fx.norms, fx.max_doc, fx.doc_count, fx.sum_ttf, live_docs=live)
        try:
            for limit in (None, ps.CHUNK - 1, ps.CHUNK):
                g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx, next_limit=limit)
                hits, totals, st = _search(ctx, g, queries, 10)
                print(n, "live docs", int(alive.sum()), "next_limit", limit, st)
                _check_chunk_rows(fx, ix, queries, hits, totals, 10, (n, int(alive.sum()), limit), live=live, limit=limit)
                assert ps.S_GROUPS in st and ps.S_RPT in st
                for row, q in enumerate(queries):
                    j = row // 3
                    first = int(np.argmax(fx.matches[j] & alive)) if (fx.matches[j] & alive).any() else None
                    yields = first is not None and (q.slop == 0 or limit is None or first <= limit)
                    assert totals[row] == (int((fx.matches[j] & alive).sum()) if yields else 0), (n, limit, fx.first[j], q.terms, q.slop)
                if alive.any():
                    j = fx.first.index(ps.CHUNK)
                    assert (totals[3 * j + 1] > 0) == (totals[3 * j + 2] > 0) == (limit is None or limit >= ps.CHUNK)
                else:
                    assert not totals.any() and (hits["doc"] == -1).all()
        finally:
            leaf.segment.close()


@pytest.mark.parametrize("k", ps.KS)
@pytest.mark.parametrize("n", [ps.CHUNK + 1, 2 * ps.CHUNK + 1])
def test_collector_at_every_k(ctx, oracle, chunk_leaves, n, k):
    """k on both sides of 64 (the wide top-k) and 128 (the chunked collector | one wavefront per query in passes of 128) over more
    than one chunk of candidates: exact, sloppy and repeated-term sloppy phrases; hit counts against the plain count as well."""
    import rucene_amd
    fx = ps.chunks(n)
    ix, leaf = chunk_leaves(n)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
    queries = [q for j in range(len(fx.first)) for q in fx.queries(j)]
    hits, totals, st = _search(ctx, g, queries, k)
    print(n, "k", k, st)
    _check_chunk_rows(fx, ix, queries, hits, totals, k, (n, "k", k))
    assert totals.tolist() == [int(fx.matches[j].sum()) for j in range(len(fx.first)) for _ in range(3)]
    assert (hits["doc"] >= 0).sum(axis=1).tolist() == [min(k, t) for t in totals.tolist()]
    assert int(fx.matches[0].sum()) > (128 if n == ps.CHUNK + 1 else 300)   # rows that k = 129 (and 300) does not exhaust
    assert ps.COLLECT in st and (ps.MERGE in st) == (k <= ps.PASS_K), (k, st)
