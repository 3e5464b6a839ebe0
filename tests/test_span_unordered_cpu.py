"""The fixtures and the model of tests/span_unordered.py, proven without a GPU: restatement (a) - the reference's objects with the
heap as an explicit array - against the width lists written out by hand, (a) against the tie-free closed form (b), the proof that
the fixtures can see the heap's array (a disturbed heap, and two tie rules, give other spans), the carried max cell, where the
ladder's docs lie, and the mirrors' routing (`-m "not gpu"`)."""
import os

import numpy as np
import pytest

import phrase_spectrum as ps
import span_near as sn
import span_unordered as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _designed():
    for name, c in su.all_cases():
        if c.designed is not None:
            for q in c.queries:
                yield name, c, q, su.designed_lists(su.segment(name), c, q)


def test_restatement_a_gives_the_width_lists_written_out_by_hand():
    """Every designed doc: the widths of its spans, in the order they come out, and the f32 frequency they add up to. The ordinary
    doc of every case (the clauses' terms side by side) has one span however the clauses are ordered."""
    seen = 0
    for name, c, q, lists in _designed():
        stated = su.widths_of(q)
        assert stated is not None, (name, c.name)
        hit, freq, widths = su.walk_reference(lists, q.slop)
        assert widths == list(stated) and hit == bool(stated), (name, c.name, q.slop, widths[:16], list(stated)[:16])
        assert freq.view(np.int32) == np.float32(q.want).view(np.int32), (name, c.name, q.slop)
        fx = su.segment(name)
        if c.rung != "singleton":
            ordinary = [dict(fx.postings[t])[c.ordinary] for t in q.terms]
            assert su.walk_reference(ordinary, q.slop)[0], (name, c.name)
        seen += 1
    assert seen >= 60


def test_the_walk_cases_say_what_they_are_named_for():
    fx = su.segment("walk")
    by = {c.name: c for c in fx.cases}
    q = by["transposed"].queries[0]
    lists = su.designed_lists(fx, by["transposed"], q)
    assert su.walk_reference(lists, 0)[2] == [1] and not sn.walk_reference(lists, 5)[0]   # a hit here, none under in_order = true
    assert su.walk_reference([[1, 3], [5]], 3)[1].view(np.int32) == np.float32(0.53333336).view(np.int32)
    c = by["runs-out-in-front"]   # no span, but a candidate: it counts for next_limit
    for q in c.queries:
        assert c.designed in sn.doc_lists(fx.postings, q.terms) and c.designed not in su.search_case(fx, q, 1000)[0].tolist()
        assert not su.walk_reference(su.designed_lists(fx, c, q), q.slop)[0]
    setup = su._NearSpansUnordered(0, 2)
    setup.start_doc([[7], [8]])
    setup.sub_span_cells_to_positions_queue()
    assert setup.at_match()   # "adjacent": true at set-up
    setup.start_doc([[1, 20], [21]])
    setup.sub_span_cells_to_positions_queue()
    assert not setup.at_match() and su.walk_reference([[1, 20], [21]], 0)[2] == [1]   # "match-only-later"
    assert su.f32sum(su.ORDER_WIDTHS).view(np.int32) != su.f32sum(su.ORDER_WIDTHS[::-1]).view(np.int32)
    assert len(su.ORDER_WIDTHS) == 9


def test_the_tie_docs_tell_the_array_from_both_tie_rules():
    """The issue's four-clause doc and three seeded ones: the heap walk, "lowest clause index moves first" and "highest clause index
    moves first" give three different width lists, and three different f32 frequencies."""
    assert su.three_way(su.ISSUE_EXAMPLE, 0) == ([2, 1, 2], [2, 1], [2, 1, 2, 2])
    assert [float(su.f32sum(w)) for w in su.three_way(su.ISSUE_EXAMPLE, 0)] == [np.float32(1.1666667), np.float32(0.8333334), np.float32(1.5000001)]
    fx = su.segment("ties")
    n = 0
    for c in fx.cases:
        if c.name.startswith("three-way"):
            lists = su.designed_lists(fx, c, c.queries[0])
            three = su.three_way(lists, 0)
            assert three is not None and len({su.f32sum(w).view(np.int32).item() for w in three}) == 3, c.name
            assert len({t for t in c.queries[0].terms}) == 4 and not su.tie_free(lists)
            n += 1
    assert n >= 3
    by = {c.name: c for c in fx.cases}
    for k in (2, 3, 4, 5):   # k distinct terms on shared positions
        c = by["stacked-%d" % k]
        lists = su.designed_lists(fx, c, c.queries[0])
        assert len(set(c.queries[0].terms)) == k and len(set.intersection(*map(set, lists))) >= 1
    # one term under two / three clauses: the outcome does not depend on which tied cell moves first
    for name in ("same-term-twice", "same-term-thrice"):
        for q in by[name].queries:
            lists = su.designed_lists(fx, by[name], q)
            if len(set(q.terms)) == 1:
                assert su.walk_reference(lists, q.slop)[2] == su.walk_rule(lists, q.slop, False)[2] == su.walk_rule(lists, q.slop, True)[2]
    c = by["tie-at-the-end"]
    lists = su.designed_lists(fx, c, c.queries[0])
    assert lists[0][-1] == lists[1][-1]


def test_a_equals_b_on_every_tie_free_doc():
    n = 0
    for name, c, q, lists in _designed():
        if su.tie_free(lists):
            a, b = su.walk_reference(lists, q.slop), su.walk_events(lists, q.slop)
            assert a[0] == b[0] and a[2] == b[2] and a[1].view(np.int32) == b[1].view(np.int32), (name, c.name)
            n += 1
    assert n >= 30
    docs = su.random_docs(4000, seed=91, ties=False)
    hits = 0
    for lists, slop in docs:
        a, b = su.walk_reference(lists, slop), su.walk_events(lists, slop)
        assert a[0] == b[0] and a[2] == b[2] and a[1].view(np.int32) == b[1].view(np.int32), (lists, slop)
        hits += a[0]
    assert 400 < hits < 3900   # (both outcomes are well represented)


def test_a_disturbed_heap_shows_on_docs_with_ties():
    """4000 seeded docs of distinct terms that share positions: restatement (a) over a heap that takes the LEFT child on equal differs
    from the reference's on some of them - the expectation depends on the array, so a kernel that re-derives an order cannot pass -
    and on none of 4000 tie-free docs."""
    docs = su.random_docs(4000, seed=92, ties=True)
    assert all(sum(map(len, lists)) <= 12 for lists, _ in docs)
    differ = sum(su.walk_reference(lists, slop)[2] != su.walk_reference(lists, slop, disturbed=True)[2] for lists, slop in docs)
    rule = sum(su.walk_reference(lists, slop)[2] != su.walk_rule(lists, slop, False)[2] for lists, slop in docs)
    print("disturbed heap differs on", differ, "of 4000; 'lowest index first' on", rule)
    assert differ >= 1 and rule >= 1
    for lists, slop in su.random_docs(4000, seed=93, ties=False):
        assert su.walk_reference(lists, slop)[2] == su.walk_reference(lists, slop, disturbed=True)[2]


def test_the_max_cell_carried_from_the_previous_doc_is_harmless():
    """Whatever doc the same NearSpansUnordered saw before - one that ended with clause 0, 1 or 2 exhausted (that cell is then the
    max cell, at NO_MORE_POSITIONS) - the next doc's spans are the ones of a fresh object."""
    docs = su.random_docs(600, seed=94, ties=True)
    three = [(lists, slop) for lists, slop in docs if len(lists) == 3]
    assert len(three) > 60
    carried = set()
    for (prev, _), (lists, slop) in zip(three, three[1:]):
        walk = su.ReferenceWalk()
        walk(prev, slop)
        carried.add(walk.spans.max_end_position_cell_idx)
        fresh, after = su.walk_reference(lists, slop), walk(lists, slop)
        assert fresh[2] == after[2] and fresh[1].view(np.int32) == after[1].view(np.int32), (prev, lists, slop)
    assert carried == {0, 1, 2}


def test_the_fixtures_lie_where_the_rungs_say():
    fx = su.segment("pool")
    assert [c.shape["pool"] for c in fx.cases] == [2, ps.LANE_CAP + 1, ps.LANE_CAP + 2, ps.SMALL_POOL, ps.SMALL_POOL + 1, ps.POOL, ps.POOL + 1]
    assert [c.queries[0].level for c in fx.cases] == ["lanes", "lanes", "left", "left", "wide", "wide", None]
    assert fx.cases[-1].queries[0].error == ps.UNSUPPORTED
    for c in fx.cases:
        assert sum(len(l) for l in su.designed_lists(fx, c, c.queries[0])) == c.shape["pool"]
    fx = su.segment("terms")
    assert [(c.shape["n_terms"], c.queries[0].level, c.queries[0].error) for c in fx.cases] == [
        (6, "lanes", None), (7, "left", None), (16, "left", None), (17, None, ps.ILLEGAL_ARGUMENT)]
    fx = su.segment("place")
    by = {c.name: c for c in fx.cases}
    assert max(max(l) for l in su.designed_lists(fx, by["pos-32767"], by["pos-32767"].queries[0])) == 32767
    assert max(max(l) for l in su.designed_lists(fx, by["pos-32768"], by["pos-32768"].queries[0])) == 32768
    for c in fx.cases:
        if c.rung == "straddle":
            at = ps.place(fx.postings[c.shape["placed"]], c.designed)
            assert (at["block"], at["skip"], at["kind"]) == (2, c.shape["skip"], "packed"), (c.name, at)
            assert at["skip"] + at["freq"] == c.shape["end"] and at["behind"] == c.shape["behind"], (c.name, at)
    assert len(fx.postings[by["singleton"].shape["singleton"]]) == 1
    for name in su.BUILDERS:
        assert 100 <= su.segment(name).max_doc <= 700, name


def test_the_entry_point_is_declared_in_every_layer():
    import rucene_amd
    from rucene_amd import _lib
    name = "rgpu_search_span_unordered_batch"
    for path in ("include/rucene_gpu.h", "rust/gpu/ffi.rs", "INTEGRATION.md", "README.md", "DESIGN.md", "rust/gpu/searcher.rs",
                 "rucene_amd/csrc/host/gpu_index_searcher.hpp"):
        with open(os.path.join(ROOT, path)) as fh:
            assert name in fh.read(), path
    assert name in _lib.EXPORTS and hasattr(_lib.Segment, "search_span_unordered_batch")
    for path in ("rust/gpu/searcher.rs", "rucene_amd/csrc/host/gpu_index_searcher.hpp"):
        with open(os.path.join(ROOT, path)) as fh:
            assert "unordered_spans" in fh.read(), path


class _Seg:
    def __init__(self):
        self.calls = []

    def _rows(self, name, qs, k):
        self.calls.append((name, qs))
        return np.zeros((len(qs), k), dtype=_hit_dtype()), np.zeros(len(qs), dtype=np.int64)

    def search_span_near_batch(self, qs, ts, k):
        return self._rows("near", qs, k)

    def search_span_unordered_batch(self, qs, ts, k):
        return self._rows("unordered", qs, k)


def _hit_dtype():
    from rucene_amd import _lib
    return _lib.HIT_DTYPE


class _Leaf:
    def __init__(self):
        self.segment = _Seg()


def _searcher(**flags):
    import rucene_amd
    g = object.__new__(rucene_amd.GpuIndexSearcher)   # (no context: nothing here reaches the device)
    g.leaves, g.cpu_fallback, g.flatten_nested, g.filtered_phrases, g.required_sets = [_Leaf(), _Leaf()], None, False, False, False
    for key, value in flags.items():
        setattr(g, key, value)
    g.pack_phrases = lambda queries, leaf: (list(queries), None)
    g._merge_leaves = lambda per_leaf, n, k: per_leaf[0]
    return g


def test_the_python_mirror_routes_unordered_rows_only_when_opted_in():
    """unordered_spans off (the default): UnsupportedOperation before any leaf is touched, as before. On: the unordered rows of a
    batch go to search_span_unordered_batch, packed as the ordered ones (which keep going to search_span_near_batch), per leaf."""
    import rucene_amd
    S, N, T, B = rucene_amd.SpanTermQuery, rucene_amd.SpanNearQuery, rucene_amd.TermQuery, rucene_amd.BooleanQuery
    free, kept = N([S(1), S(2)], slop=2, in_order=False), N([S(1), S(2)], slop=2)
    off = _searcher()
    assert not getattr(off, "unordered_spans", False)
    with pytest.raises(rucene_amd.RgpuError) as e:
        off.search_batch([kept, free], 10)
    assert e.value.status == ps.UNSUPPORTED and not any(leaf.segment.calls for leaf in off.leaves)
    assert free.served_by_gpu() is not None and free.served_by_gpu(True) is None and kept.served_by_gpu() is None
    on = _searcher(unordered_spans=True)
    hits, totals = on.search_batch([free, kept, free], 10)
    assert hits.shape == (3, 10)
    for leaf in on.leaves:
        assert sorted(leaf.segment.calls, key=lambda c: c[0]) == [("near", [kept]), ("unordered", [free, free])]
    near = N([S(1), S(2)], in_order=False)
    refused = [N([S(1), N([S(2), S(3)], in_order=False)], in_order=False), N([S(i) for i in range(17)], in_order=False), N([S(1), S(2)], slop=-1, in_order=False),
               B.build([near, T(3)], []), B.build([], [near, T(3)]), rucene_amd.DisjunctionMaxQuery([T(1), near]),
               rucene_amd.BoostingQuery.build(near, T(1), 0.5)]
    for q in refused:   # refused either way
        for g in (off, on):
            with pytest.raises(rucene_amd.RgpuError) as e:
                g.search_batch([q], 10)
            assert e.value.status == ps.UNSUPPORTED, q
    sig = rucene_amd.GpuIndexSearcher.__init__.__defaults__
    assert rucene_amd.GpuIndexSearcher.__init__.__code__.co_varnames[:10][-1] == "unordered_spans" and sig[-1] is False


def test_cpp_unordered_demo_compiles_without_a_gpu(tmp_path):
    """tests/cpp/span_unordered_demo.cpp links against the C ABI on a CPU-only box (running it needs a GPU:
    tests/test_gpu_span_unordered.py)."""
    import subprocess
    import __graft_entry__ as entry
    entry.build()
    libdir = os.path.join(ROOT, "rucene_amd")
    exe = str(tmp_path / "span_unordered_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "cpp", "span_unordered_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-lrucene_indexgen", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)
