"""Exact phrases under doc-set masks on the device (`-m gpu`): rgpu_search_phrase_batch_masked, _phrase_bool_batch_masked and
_phrase_or_batch_masked against the UNMASKED calls on a twin segment uploaded with live docs = live AND set - every byte of the hit rows
and the totals equal - through the C ABI, the Python mirror (filtered_phrases=True) and the C++ mirror (tests/cpp/phrase_masked_demo.cpp).
The same cases run once more in a fresh child process under RGPU_PHRASE_MASK_COMPACT=0 (the marking instantiation of the candidate
conjunction): rows byte-identical, the other launch name in the kernel statistics. tests/test_phrase_masked_cpu.py proves the twin-leaf
equivalence itself on the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

import phrase_bool as pb
import phrase_masked as pm
import phrase_or as po
import phrase_rescore as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P130, P8191, P8193, P16385, PDE, C, N = pm.P130, pm.P8191, pm.P8193, pm.P16385, pm.PDE, pm.C, pm.N

# (name, kind, queries, deletions?, mask, k). kind "phrase": Ph rows; "bool": pb.Q rows; "or": po.Q rows. One masked call each.
CASES = [("130 -> %d" % n, "phrase", [P130, PDE, P130], False, "first %d" % n, 10) for n in (0, 1, 63, 64, 65)] + [
    ("middle group empty", "phrase", [PDE, P130], False, "middle group empty", 80),
    ("bits at 0, 63 | 64, max_doc - 1", "phrase", [P130, P16385], False, "edges", 10),
    ("empty mask", "phrase", [P130, P8193], False, "empty", 10),
    ("full mask, deletions", "phrase", [P130, P8193, PDE], True, "full", 20),
    ("disjoint mask", "phrase", [P130], False, "disjoint", 10),
    ("deletions and mask overlap", "phrase", [P130, P8193, P16385], True, "overlaps deletions", 70),
    ("bool: 130 -> 65", "bool", [pb.Q([P130, C]), pb.Q([C, P130, PDE])], False, "first 65", 10),
    ("bool: middle group empty", "bool", [pb.Q([P130, C]), pb.Q([P130, pm.B])], True, "middle group empty", 80),
    ("bool: -d and -X both hold a candidate", "bool", [pb.Q([P130, C], [N]), pb.Q([P130], [N, pm.ABSENT])], False, "other", 40),
    ("bool: 1, 2 and 4 phrases", "bool", [pb.Q([P130, C]), pb.Q([P130, PDE]), pb.Q([P130, PDE, P8191, P16385], [N])], True, "other", 12),
    ("or: 130 -> 64", "or", [po.Q([P130, C]), po.Q([P130])], False, "first 64", 10),
    ("or: 1, 2 and 4 phrases, k = 129", "or", [po.Q([P130, pm.D2]), po.Q([PDE, pm.N, P130], [C]), po.Q([P130, PDE, P8191, P16385, pm.D2], msm=2)], True, "other", 129),
    ("or: empty mask", "or", [po.Q([P130, C])], True, "empty", 10),
]
for n in (8191, 8193, 16385):   # cut to a handful; k = 10: the chunked collector (1, 2, 3 chunks), k = 130: one wavefront per query, in passes
    CASES += [("%d -> a handful, k = %d" % (n, k), "phrase", [pm.BY_COUNT[n], P130], False, "handful", k) for k in (10, 130)]
CASES += [("bool: 8193 -> a handful", "bool", [pb.Q([P8193, C])], False, "handful", 10), ("or: 16385 -> a handful", "or", [po.Q([P16385, pm.N])], True, "handful", 10)]
LEGACY = ("130 -> 65", "middle group empty", "bool: -d and -X both hold a candidate", "or: 1, 2 and 4 phrases, k = 129", "8193 -> a handful, k = 10")


class Grid:
    """tests/phrase_masked.py grid() on the device: one index per .doc format, base segments with and without deletions, twins on demand."""

    def __init__(self, oracle, ctx):
        import rucene_amd
        self.rucene, self.oracle, self.ctx, self.fx = rucene_amd, oracle, ctx, pm.grid()
        self.ixs, self.opened, self.sets = {}, {}, []
        self.masks = pm.masks()

    def open(self, version, gone):
        """-> (GpuIndexSearcher, leaf) over the grid with the docs `gone` deleted"""
        key = (version, frozenset(gone))
        if key not in self.opened:
            if version not in self.ixs:
                self.ixs[version] = self.fx.index(self.oracle, version=version)
            leaf = pr.leaf_of(self.ixs[version], self.fx, live_docs=pb.live_words(self.fx.max_doc, gone) if gone else None)
            self.opened[key] = (self.rucene.GpuIndexSearcher([leaf], ctx=self.ctx, filtered_phrases=True), leaf)
        return self.opened[key]

    def base(self, version, deletions):
        return self.open(version, pm.DELETED if deletions else frozenset())

    def twin(self, version, deletions, mask):
        gone = set(pm.DELETED if deletions else ()) | (set(range(self.fx.max_doc)) - set(self.masks[mask]))
        return self.open(version, gone)

    def docset(self, leaf, mask):
        s = leaf.segment.docset_from_docs(np.array(self.masks[mask], dtype=np.int32))
        self.sets.append(s)
        return s

    def close(self):
        for s in self.sets:
            s.close()
        for _, leaf in self.opened.values():
            leaf.segment.close()
        for ix in self.ixs.values():
            ix.close()


def _built(kind, queries):
    import rucene_amd
    if kind == "phrase":
        return [rucene_amd.PhraseQuery(list(p.terms), pb.phrase_positions(p)) for p in queries]
    return [q.build(raw=True) if kind == "or" else _bool(q) for q in queries]


def _bool(q):
    """pb.Q -> the BooleanQuery as it is, also where BooleanQuery::build would hand back its only clause"""
    import rucene_amd
    built = q.build()
    if isinstance(built, rucene_amd.PhraseQuery):
        return rucene_amd.BooleanQuery([built], [], 0, [], [])
    return built


def _call(g, leaf, kind, queries, k, docset=None):
    """one call of the C ABI (masked when a doc set is given) -> (hits, totals)"""
    seg, built = leaf.segment, _built(kind, queries)
    if kind == "phrase":
        packed = g.pack_phrases(built, leaf)
        return seg.search_phrase_batch(*packed, k) if docset is None else seg.search_phrase_batch_masked(docset, *packed, k)
    if kind == "bool":
        packed = g.pack_phrase_bool(built, leaf)
        return seg.search_phrase_bool_batch(*packed, k) if docset is None else seg.search_phrase_bool_batch_masked(docset, *packed, k)
    packed = g.pack_phrase_or(built, leaf)
    return seg.search_phrase_or_batch(*packed, k) if docset is None else seg.search_phrase_or_batch_masked(docset, *packed, k)


def run_cases(grid, ctx):
    """every case through the masked C ABI call -> {(version, name): (hit bytes, total bytes, launch names)}"""
    out = {}
    for version in (1, 0):
        for name, kind, queries, deletions, mask, k in CASES:
            if version == 0 and name not in LEGACY:
                continue
            g, leaf = grid.base(version, deletions)
            ds = grid.docset(leaf, mask)
            ctx.kernel_stats_reset()
            hits, totals = _call(g, leaf, kind, queries, k, ds)
            names = sorted(n for n, v in ctx.kernel_stats().items() if v["launches"])
            out[(version, name)] = (hits.tobytes(), totals.tobytes(), names)
    return out


def child_main(path):
    """the RGPU_PHRASE_MASK_COMPACT=0 run: a process of its own (the switch is read when the context is created)"""
    import pickle

    import rucene_amd
    from oracle import binding as oracle
    assert os.environ.get(pm.SWITCH) == "0"
    oracle.lib()
    ctx = rucene_amd.Context(profile_kernels=True)
    grid = Grid(oracle, ctx)
    try:
        rows = run_cases(grid, ctx)
    finally:
        grid.close()
        ctx.close()
    with open(path, "wb") as f:
        pickle.dump(rows, f)


@pytest.fixture(scope="module")
def ctx():
    import rucene_amd
    assert os.environ.get(pm.SWITCH) in (None, "1"), "the suite runs with the default: compaction on"
    c = rucene_amd.Context(profile_kernels=True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def grid(oracle, ctx):
    g = Grid(oracle, ctx)
    yield g
    g.close()


@pytest.fixture(scope="module")
def compact_rows(grid, ctx):
    return run_cases(grid, ctx)


@pytest.fixture(scope="module")
def marked_rows(tmp_path_factory):
    import pickle
    path = str(tmp_path_factory.mktemp("marked") / "rows.pkl")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_phrase_masked as t; t.child_main(%r)" % (ROOT, os.path.join(ROOT, "tests"), path)
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, **{pm.SWITCH: "0"}), timeout=300)
    with open(path, "rb") as f:
        return pickle.load(f)


RUNS = [(1, i) for i in range(len(CASES))] + [(0, i) for i, c in enumerate(CASES) if c[0] in LEGACY]   # what run_cases runs


@pytest.mark.parametrize("version,case", RUNS, ids=["%s%s" % (CASES[i][0], "" if v else ", legacy .doc format") for v, i in RUNS])
def test_masked_rows_equal_the_unmasked_rows_on_the_twin_segment(grid, compact_rows, case, version):
    name, kind, queries, deletions, mask, k = CASES[case]
    hits, totals, names = compact_rows[(version, name)]
    g, leaf = grid.twin(version, deletions, mask)
    want_hits, want_totals = _call(g, leaf, kind, queries, k)
    got = np.frombuffer(hits, dtype=want_hits.dtype).reshape(want_hits.shape)
    print(name, np.frombuffer(totals, np.int64).tolist(), want_totals.tolist())
    assert np.frombuffer(totals, np.int64).tolist() == want_totals.tolist(), name
    assert hits == want_hits.tobytes(), (name, got["doc"][:, :8].tolist(), want_hits["doc"][:, :8].tolist())
    if mask in ("empty", "disjoint") and kind == "phrase":
        assert not want_totals[[i for i, q in enumerate(queries) if q is P130]].any()
    if mask not in ("empty",):
        assert want_totals.any() or mask == "disjoint", "a case over empty rows shows nothing"


def test_survivor_counts_are_what_the_cases_are_named_for(grid, compact_rows):
    """first n: n candidates survive, those where the phrase holds are the hits; the middle group of the marking kernel's slots holds none."""
    a = pm.A130_DOCS
    for n in (0, 1, 63, 64, 65):
        totals = np.frombuffer(compact_rows[(1, "130 -> %d" % n)][1], np.int64)
        assert totals[0] == totals[2] == sum(pm.phrase_holds(d) for d in a[:n]), n
    totals = np.frombuffer(compact_rows[(1, "middle group empty")][1], np.int64)
    assert totals[1] == sum(pm.phrase_holds(d) for d in a[:128:2] + a[128:])


def test_a_full_mask_on_a_leaf_with_deletions_is_the_unmasked_call(grid, compact_rows):
    name, kind, queries, deletions, mask, k = next(c for c in CASES if c[0] == "full mask, deletions")
    g, leaf = grid.base(1, True)
    hits, totals = _call(g, leaf, kind, queries, k)
    assert compact_rows[(1, name)][0] == hits.tobytes() and compact_rows[(1, name)][1] == totals.tobytes()
    assert totals.all() and not (set(hits["doc"].ravel().tolist()) & pm.DELETED)


@pytest.mark.parametrize("kind", ["phrase", "bool", "or"])
def test_k_below_at_and_above_the_survivor_count(grid, kind):
    queries = {"phrase": [P130], "bool": [pb.Q([P130, C])], "or": [po.Q([P130, pm.ABSENT])]}[kind]
    g, leaf = grid.base(1, True)
    tg, tleaf = grid.twin(1, True, "first 65")
    ds = grid.docset(leaf, "first 65")
    n = int(_call(tg, tleaf, kind, queries, 1)[1][0])
    assert 20 < n < 65
    for k in (n - 1, n, n + 1):
        hits, totals = _call(g, leaf, kind, queries, k, ds)
        want_hits, want_totals = _call(tg, tleaf, kind, queries, k)
        assert hits.tobytes() == want_hits.tobytes() and totals.tolist() == want_totals.tolist() == [n], (kind, k)
        assert (hits["doc"][0] >= 0).sum() == min(k, n)


def test_the_switch_changes_the_launch_and_not_a_byte(compact_rows, marked_rows):
    """Default: the compacting instantiation answers, under its own launch names; RGPU_PHRASE_MASK_COMPACT=0 (a fresh process): the marking
    one, under its own; neither run launches the unmasked names or the other's; hits and totals are byte-identical."""
    assert sorted(compact_rows) == sorted(marked_rows)
    kinds = {c[0]: c[1] for c in CASES}
    for key in sorted(compact_rows):
        version, name = key
        kind = kinds[name]
        names, marked_names = compact_rows[key][2], marked_rows[key][2]
        every = set(pm.COMPACT.values()) | set(pm.MARKED.values()) | set(pm.UNMASKED.values())
        assert set(names) & every == {pm.COMPACT[kind]}, (key, names)
        assert set(marked_names) & every == {pm.MARKED[kind]}, (key, marked_names)
        assert compact_rows[key][0] == marked_rows[key][0] and compact_rows[key][1] == marked_rows[key][1], key
        assert [n for n in names if n != pm.COMPACT[kind]] == [n for n in marked_names if n != pm.MARKED[kind]], (key, names, marked_names)


def test_an_unmasked_phrase_call_launches_neither_new_name(grid, ctx):
    g, leaf = grid.base(1, True)
    for kind, queries in (("phrase", [P130]), ("bool", [pb.Q([P130, C])]), ("or", [po.Q([P130, C])])):
        ctx.kernel_stats_reset()
        _call(g, leaf, kind, queries, 10)
        names = {n for n, v in ctx.kernel_stats().items() if v["launches"]}
        assert pm.UNMASKED[kind] in names and not names & (set(pm.COMPACT.values()) | set(pm.MARKED.values())), (kind, names)


def _raw(fn, leaf, docset, packed, k):
    from rucene_amd import _lib as gpu
    n = packed[0].size
    hits = np.full((n, k), 7, dtype=np.int64).view(gpu.HIT_DTYPE).reshape(n, k)
    totals = np.full(n, -9, dtype=np.int64)
    args = []
    for a in packed:
        args += [a.ctypes.data if a.size else None, a.size]
    rc = getattr(gpu.lib(), fn)(leaf.segment._h, docset._h, *args, k, hits.ctypes.data, totals.ctypes.data)
    return rc, hits, totals


def test_refusals_leave_the_outputs_untouched(grid, ctx):
    """A sloppy phrase (query or clause) under a mask: UnsupportedOperation; a set of another segment: IllegalArgument. Nothing is
    launched, nothing is written."""
    import rucene_amd
    P = rucene_amd.PhraseQuery
    g, leaf = grid.base(1, False)
    og, other = grid.base(1, True)
    mine, foreign = grid.docset(leaf, "other"), grid.docset(other, "other")
    exact, sloppy = P([pm.A130, pm.B]), P([pm.A130, pm.B], slop=1)
    calls = [("rgpu_search_phrase_batch_masked", g.pack_phrases([exact, sloppy], leaf), g.pack_phrases([exact], leaf))]
    qs, ps, pts, ts = g.pack_phrase_bool(_built("bool", [pb.Q([P130, C]), pb.Q([PDE, C])]), leaf)
    bad = ps.copy()
    bad["slop"][1] = 2
    calls.append(("rgpu_search_phrase_bool_batch_masked", (qs, bad, pts, ts), (qs, ps, pts, ts)))
    qs, ps, pts, ts = g.pack_phrase_or(_built("or", [po.Q([P130, C])]), leaf)
    bad = ps.copy()
    bad["slop"][0] = 1
    calls.append(("rgpu_search_phrase_or_batch_masked", (qs, bad, pts, ts), (qs, ps, pts, ts)))
    for fn, with_sloppy, fine in calls:
        ctx.kernel_stats_reset()
        rc, hits, totals = _raw(fn, leaf, mine, with_sloppy, 8)
        assert rc == pm.UNSUPPORTED and (hits.view(np.int64) == 7).all() and (totals == -9).all(), fn
        rc, hits, totals = _raw(fn, leaf, foreign, fine, 8)
        assert rc == pm.ILLEGAL_ARGUMENT and (hits.view(np.int64) == 7).all() and (totals == -9).all(), fn
        assert not any(v["launches"] for n, v in ctx.kernel_stats().items() if n.startswith("k_search_and")), fn
        rc, hits, totals = _raw(fn, leaf, mine, fine, 8)
        assert rc == 0 and totals[0] > 0, fn
    with pytest.raises(rucene_amd.RgpuError) as e:
        g.search_batch([rucene_amd.searcher.FilterQuery(sloppy, [g.filter_from_docs([0, 63])])], 4)
    assert e.value.status == pm.UNSUPPORTED


# ---- the Python mirror ------------------------------------------------------------------------------------------------------------------
def _mirror_pair(oracle, ctx, fxs, deleted, mask_docs):
    """(searcher with filtered_phrases over the leaves, the twin searcher whose live docs are live AND mask, their pb.Index objects)"""
    import rucene_amd
    ix = pb.Index(oracle, fxs, deleted=deleted)
    keep = set(mask_docs)
    gone = [set(deleted[li]) | {d for d in range(fx.max_doc) if d + ix.bases[li] not in keep} for li, fx in enumerate(fxs)]
    tix = pb.Index(oracle, fxs, deleted=gone)
    leaves, tleaves = ix.gpu_leaves(), tix.gpu_leaves()
    return rucene_amd.GpuIndexSearcher(leaves, ctx=ctx, filtered_phrases=True), rucene_amd.GpuIndexSearcher(tleaves, ctx=ctx), (ix, tix, leaves + tleaves)


def _close_pair(rest):
    ix, tix, leaves = rest
    for leaf in leaves:
        if leaf.segment is not None:
            leaf.segment.close()
    ix.close()
    tix.close()


def test_python_mirror_over_three_leaves_one_without_a_phrase_term(oracle, ctx):
    """FilterQuery(phrase, F), +"a b" #F -X, +"a b" +c #F -d, "a b" c -X over tests/phrase_bool.py's three leaves (the third lacks PA),
    doc bases and deletions: the rows of the bare queries on the twin leaves. The refused shapes reach cpu_fallback."""
    import rucene_amd
    from rucene_amd.searcher import FilterQuery
    T, Bq, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery
    fxs = list(pb.leaves())
    total = sum(fx.max_doc for fx in fxs)
    f_docs = [d for d in range(total) if d % 4 != 1]
    x_docs = [0, 72, 254, 700, 772, 954, 1400, 1500]
    deleted = [{24, 48}, {36}, set()]
    g, tg, rest = _mirror_pair(oracle, ctx, fxs, deleted, set(f_docs) - set(x_docs))
    g2, tg2, rest2 = _mirror_pair(oracle, ctx, fxs, deleted, set(range(total)) - set(x_docs))
    try:
        ab, bc = P([pb.PA, pb.PB]), P([pb.PB, pb.PC])
        F, X = g.filter_from_docs(f_docs), g.filter_from_docs(x_docs)
        X2 = g2.filter_from_docs(x_docs)
        filtered = [Bq.build([ab], [], filters=[F], must_nots=[X]), Bq.build([ab, T(pb.D600)], [], filters=[F], must_nots=[X, T(pb.N3)]),
                    Bq.build([ab, bc, T(pb.D600)], [], filters=[F], must_nots=[X])]
        bare = [ab, Bq.build([ab, T(pb.D600)], [], must_nots=[T(pb.N3)]), Bq.build([ab, bc, T(pb.D600)], [])]
        ctx.kernel_stats_reset()
        hits, totals = g.search_batch(filtered, 24)
        names = {n for n, v in ctx.kernel_stats().items() if v["launches"]}
        assert pm.COMPACT["phrase"] in names and pm.COMPACT["bool"] in names, names
        want_hits, want_totals = tg.search_batch(bare, 24)
        assert hits.tobytes() == want_hits.tobytes() and totals.tolist() == want_totals.tolist()
        assert totals.all() and (hits[0]["doc"] >= pb.MAIN_DOCS).any()
        # "a b" c -X and "a b" -X: the disjunction route, masked by NOT X alone
        ors = [Bq.build([], [ab, T(pb.D600)], must_nots=[X2]), Bq.build([], [T(pb.T129), ab, bc], must_nots=[X2, T(pb.N3)]), Bq.build([], [ab], must_nots=[X2])]
        ors_bare = [Bq.build([], [ab, T(pb.D600)]), Bq.build([], [T(pb.T129), ab, bc], must_nots=[T(pb.N3)]), ab]
        hits, totals = g2.search_batch(ors, 129)
        want_hits, want_totals = tg2.search_batch(ors_bare, 129)
        assert hits.tobytes() == want_hits.tobytes() and totals.tolist() == want_totals.tolist() and totals.all()
        # FilterQuery over each kind
        under = [ab, bare[1], ors_bare[0]]
        g3, tg3, rest3 = _mirror_pair(oracle, ctx, fxs, deleted, f_docs)
        try:
            F3 = g3.filter_from_docs(f_docs)
            hits, totals = g3.search_batch([FilterQuery(q, [F3]) for q in under], 16)
            want_hits, want_totals = tg3.search_batch(under, 16)
            assert hits.tobytes() == want_hits.tobytes() and totals.tolist() == want_totals.tolist() and totals.all()
        finally:
            _close_pair(rest3)
        # refused with the opt-in on: sloppy, "a b" c #F; with it off: everything
        seen = []
        g.cpu_fallback = lambda query, collector: seen.append(query) or "cpu"
        for q in (FilterQuery(P([pb.PA, pb.PB], slop=1), [F]), Bq.build([], [ab, T(pb.D600)], filters=[F])):
            with pytest.raises(rucene_amd.RgpuError) as e:
                g.search_batch([q], 4)
            assert e.value.status == pm.UNSUPPORTED
            assert g.search(q, rucene_amd.TopDocsCollector(4)) == "cpu" and seen[-1] is q
        Ft = tg.filter_from_docs(f_docs)
        with pytest.raises(rucene_amd.RgpuError) as e:
            tg.search_batch([FilterQuery(ab, [Ft])], 4)
        assert e.value.status == pm.UNSUPPORTED
    finally:
        _close_pair(rest)
        _close_pair(rest2)


def test_a_mixed_batch_of_two_masks_and_unmasked_rows_keeps_row_order(grid, ctx):
    """Masked phrase rows of two different masks, masked term rows and unmasked rows of every kind in ONE search_batch: every row is
    what its bare query gives on the twin segment of its mask (or on the segment itself), in its place."""
    import rucene_amd
    from rucene_amd.searcher import FilterQuery
    T, Bq, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery
    g, leaf = grid.base(1, True)
    F1, F2 = g.filter_from_docs(grid.masks["other"]), g.filter_from_docs(grid.masks["first 65"])
    p130, pde = P([pm.A130, pm.B]), P([pm.D2, pm.E2])
    inner = [p130, Bq.build([p130, T(C)], [], must_nots=[T(N)]), T(C), Bq.build([], [p130, T(pm.D2)]), pde, Bq.build([p130, pde], []), p130, Bq.build([T(C), T(pm.D2)], [])]
    which = [F1, F1, F1, F2, F2, None, None, F2]
    mixed = [q if f is None else FilterQuery(q, [f]) for q, f in zip(inner, which)]
    ctx.kernel_stats_reset()
    hits, totals = g.search_batch(mixed, 12)
    names = {n for n, v in ctx.kernel_stats().items() if v["launches"]}
    assert set(pm.COMPACT.values()) <= names and pm.UNMASKED["phrase"] in names and pm.UNMASKED["bool"] in names, names
    for mask, f in (("other", F1), ("first 65", F2), (None, None)):
        rows = [i for i, w in enumerate(which) if w is f]
        tg, _ = grid.base(1, True) if mask is None else grid.twin(1, True, mask)
        want_hits, want_totals = tg.search_batch([inner[i] for i in rows], 12)
        assert hits[rows].tobytes() == want_hits.tobytes() and totals[rows].tolist() == want_totals.tolist(), mask
    assert totals.all()


# ---- the C++ mirror ---------------------------------------------------------------------------------------------------------------------
def test_cpp_host_mirror_gives_the_twin_rows(grid, ctx, tmp_path):
    """GpuIndexSearcher::search_many with filtered_phrases on (tests/cpp/phrase_masked_demo.cpp, compiled warnings-as-errors): FilteredQuery
    over a PhraseQuery, a PhraseBooleanQuery and a PhraseDisjunctionQuery under both spellings, beside unmasked rows, on the grid with
    deletions - the rows of the bare queries on the twin segments; the refused shapes stay refused."""
    import rucene_amd
    T, Bq, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery
    fx = grid.fx
    exe = str(tmp_path / "phrase_masked_demo")
    libdir = os.path.join(ROOT, "rucene_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "phrase_masked_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    g, leaf = grid.base(1, True)
    doc_bytes, pos_bytes = grid.ixs[1].files()
    for name, blob in (("doc", doc_bytes), ("pos", pos_bytes), ("norms", fx.norms.tobytes()), ("terms", leaf.terms.tobytes()),
                       ("tpos", leaf.term_positions.tobytes()), ("live", pb.live_words(fx.max_doc, pm.DELETED).tobytes())):
        (tmp_path / (name + ".bin")).write_bytes(bytes(blob))
    f_docs, x_docs = grid.masks["other"], [0, 64, 100, 6000]
    (tmp_path / "f.txt").write_text("\n".join(map(str, f_docs)) + "\n")
    (tmp_path / "x.txt").write_text("\n".join(map(str, x_docs)) + "\n")
    ph = lambda a, b: "p:%d,%d:0,1:1.0" % (a, b)
    p130, pde = P([pm.A130, pm.B]), P([pm.D2, pm.E2])
    b_line = "b m:%s m:t:%d n:t:%d" % (ph(pm.A130, pm.B), C, N)
    o_line = "o1 s:%s s:t:%d s:%s" % (ph(pm.A130, pm.B), pm.D2, ph(pm.D2, pm.E2))
    b_q = Bq.build([p130, T(C)], [], must_nots=[T(N)])
    o_q = Bq.build([], [p130, T(pm.D2), pde])
    lines = ["fq p " + ph(pm.A130, pm.B), "cl p " + ph(pm.A130, pm.B), "fq " + b_line, "cl " + b_line, "fq " + o_line, "cx " + o_line, "un p " + ph(pm.A130, pm.B),
             "cf p " + ph(pm.D2, pm.E2), "un " + b_line]
    bare = [p130, p130, b_q, b_q, o_q, o_q, p130, pde, b_q]
    modes = ["f", "fx", "f", "fx", "f", "x", None, "f", None]
    (tmp_path / "queries.txt").write_text("\n".join(lines) + "\n")
    k = 16
    out = subprocess.check_output([exe, str(tmp_path), str(fx.max_doc), str(fx.doc_count), str(fx.sum_ttf), str(k)], text=True, timeout=120).strip().splitlines()
    assert len(out) == len(lines) + 1 and out[-1] == "refused 1 1 1", out[-2:]
    keep = {"f": set(f_docs), "fx": set(f_docs) - set(x_docs), "x": set(range(fx.max_doc)) - set(x_docs), None: set(range(fx.max_doc))}
    for i, line in enumerate(out[:-1]):
        parts = line.split()
        assert parts[0] == "row" and int(parts[1]) == i
        got = [(int(p.split(":")[0]), int(p.split(":")[1], 16)) for p in parts[3:]]
        tg, _ = grid.open(1, set(pm.DELETED) | (set(range(fx.max_doc)) - keep[modes[i]]))
        hits, totals = tg.search_batch([bare[i]], k)
        row = hits[0][hits[0]["doc"] >= 0]
        assert int(parts[2]) == int(totals[0]) > 0, (i, line)
        assert got == list(zip(row["doc"].tolist(), row["score"].view(np.uint32).tolist())), (i, line)
