"""Hit counts without scoring, the part that needs no GPU: the numpy model of tests/count.py against the oracle's total hits on every
fixture row and mask; the fixtures really contain the edges tests/test_gpu_count.py names; the host plan under the sanitizers; the
C++ demo compiles; the entry point is declared everywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import count as ct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_come_from_the_kernel():
    w, bits = ct.kernel_constants()
    assert w == ct.W and w % 64 == 0 and w >= 128
    assert 2 ** bits > 64, "a counter holds 64 clauses without wrapping"
    assert ct.MAX_DOC == 2 * w + 37 <= 3 * w + 37


def test_the_fixtures_contain_their_edges():
    fx = ct.window_leaf()
    w, d = ct.W, lambda t: fx.lists[t][0]
    assert d(ct.EDGE).tolist() == [w - 1, w]
    assert d(ct.BLK).size == 256 and d(ct.BLK)[127] == w - 1 and d(ct.BLK)[128] == w                  # a block ends at W - 1, the next starts at W
    s = d(ct.SPARSE)
    assert s.size == 128 and s[0] < w <= s[64] < 2 * w <= s[-1]                                       # one block, three windows
    for t, tail in ((ct.TAIL0, 0), (ct.TAIL1, 1), (ct.TAIL127, 127)):
        assert d(t).size % 128 == tail and d(t).size >= 128
    assert d(ct.TAIL0)[0] < w <= d(ct.TAIL0)[-1]                                                      # the block itself straddles
    assert d(ct.TAIL1)[127] == w - 1 and d(ct.TAIL1)[128] == w
    t127 = d(ct.TAIL127)[128:]
    assert t127[0] < w <= t127[-1]                                                                    # the tail straddles
    assert [d(t).tolist() for t in (ct.S0, ct.SW1, ct.SW, ct.SLAST)] == [[0], [w - 1], [w], [ct.MAX_DOC - 1]]
    assert d(ct.ABSENT).size == 0 and d(ct.ALL).size == ct.MAX_DOC and d(ct.EQ1).size == d(ct.EQ2).size
    assert all(d(t).size == 2 and d(t)[0] == ct.H_DOC for t in ct.H) and len(ct.H) == 64
    assert 2 <= d(ct.TAILONLY).size < 128
    assert ct.MAX_DOC % ct.W == 37


def _oracle_totals(oracle, fx, alive, rows):
    forms = [ct.oracle_form(q) for q in rows]
    keep = [i for i, f in enumerate(forms) if f is not None]
    osr = oracle.Searcher([fx.oracle_segment(oracle, alive)])
    ops = [{"term": oracle.OP_TERM, "and": oracle.OP_AND, "or": oracle.OP_OR}[forms[i][0]] for i in keep]
    offs = np.concatenate([[0], np.cumsum([len(forms[i][1]) for i in keep])]).astype(np.int32)
    noffs = np.concatenate([[0], np.cumsum([len(forms[i][2]) for i in keep])]).astype(np.int32)
    tids = np.concatenate([np.asarray(forms[i][1], np.int64) for i in keep] + [np.zeros(0, np.int64)])
    nids = np.concatenate([np.asarray(forms[i][2], np.int64) for i in keep] + [np.zeros(0, np.int64)])
    _, _, _, totals, _, _ = osr.search_batch(ops, offs, tids, 1, threads=4, not_offsets=noffs, not_ids=nids,
                                             min_should_match=np.asarray([forms[i][3] for i in keep], np.int32))
    return keep, totals


@pytest.mark.parametrize("mask", ["none", "seeded-deleted", "set", "set-under-deletions", "empty-set", "all-deleted"])
def test_the_model_equals_the_oracle(oracle, mask):
    """every fixture row the oracle's search_batch can express; a masked row runs on an oracle segment built with live AND set"""
    fx = ct.window_leaf()
    alive, docset = ct.masks(fx.max_doc)[mask]
    m = ct.mask_of(fx.max_doc, alive, docset)
    rows = [q for q in ct.ALL_ROWS if not (q.op == "or" and not q.pos)]     # (an OR of MUST_NOT clauses only: no scorer, nothing to ask the oracle)
    keep, totals = _oracle_totals(oracle, fx, None if mask == "none" else m, rows)
    assert len(keep) >= len(rows) - 4
    for j, i in enumerate(keep):
        assert ct.model_count(fx.has, fx.df, m, rows[i]) == int(totals[j]), (mask, rows[i])
    # the rows left out, by the rules themselves
    assert ct.model_count(fx.has, fx.df, m, ct.OR(nots=(ct.A,))) == 0
    assert ct.model_count(fx.has, fx.df, m, ct.CQ("term", (ct.A,), demote=(ct.ABSENT,))) == 0


def test_the_model_on_rows_worked_by_hand():
    fx = ct.window_leaf()
    every = np.ones(fx.max_doc, bool)
    n = lambda q: ct.model_count(fx.has, fx.df, every, q)
    assert n(ct.T(ct.EDGE)) == 2 and n(ct.OR(*ct.H, msm=64)) == 1 and n(ct.OR(*ct.H[:63], msm=64)) == 0 and n(ct.OR(*ct.H, msm=2)) == 1
    assert n(ct.OR(ct.A, ct.A, msm=2)) == 700 and n(ct.AND(ct.A, nots=(ct.A,))) == 0 and n(ct.T(ct.A, nots=(ct.ALL,))) == 0
    two = fx.has[ct.A] & fx.has[ct.B]
    both, either = fx.has[ct.C] & fx.has[ct.EQ1], fx.has[ct.C] | fx.has[ct.EQ1]
    assert int((two & both).sum()) < int((two & either).sum())                                                          # (the two readings differ on this leaf)
    assert n(ct.OR(ct.A, ct.B, msm=2, nots=(ct.C, ct.EQ1))) == int((two & ~either).sum())     # min_should_match does not narrow the exclusion
    assert n(ct.OR(ct.A, ct.B, msm=2, nots=(ct.C, ct.ABSENT))) == int((two & ~fx.has[ct.C]).sum())


def test_host_plan_under_the_sanitizers(tmp_path):
    """tests/cpp/count_plan_test.cpp: every kind decision, the thresholds and the refusals of csrc/host/count_plan.hpp, as a stand-alone
    program built with -fsanitize=address,undefined."""
    exe = str(tmp_path / "count_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "count_plan_test.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("count_plan_test OK"), out.stdout


def test_header_export_and_bindings():
    import __graft_entry__ as g
    g.build()
    from rucene_amd import _lib
    L = C.CDLL(_lib.lib_path())
    header = open(os.path.join(ROOT, "include", "rucene_gpu.h")).read()
    assert hasattr(L, "rgpu_count_batch") and "rgpu_count_batch" in _lib.EXPORTS and "int32_t rgpu_count_batch(" in header
    assert "searcher.rs:632-654" in header   # the entry point cites the reference, as every other one does
    # argument errors are codes, never crashes; no GPU is needed for that
    out = np.full(1, -7, np.int64)
    assert _lib.lib().rgpu_count_batch(None, None, None, 0, None, 0, out.ctypes.data) == -2 and out[0] == -7


def test_cpp_demo_compiles_without_a_gpu(tmp_path):
    """tests/cpp/count_demo.cpp (count / count_many of csrc/host/gpu_index_searcher.hpp) links against the C ABI on a CPU-only box,
    warnings as errors; running it needs a GPU (tests/test_gpu_count.py)."""
    import __graft_entry__ as g
    g.build()
    libdir = os.path.join(ROOT, "rucene_amd")
    exe = str(tmp_path / "count_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "count_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-lrucene_indexgen", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)
