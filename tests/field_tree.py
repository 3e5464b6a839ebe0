"""Fixtures and reference (plain Python, no GPU) for rgpu_search_fields_tree_batch: cross-field query-string trees - nested should-only
BooleanQuery ("sum") groups, MUST beside SHOULD (ReqOptScorer). Built on tests/cross_field.py (leaves, per-clause scores, the
single-occur composition) and on the rule sequences of tests/opt_spectrum.py (S99 .. TWO: lead terms over doc ranges of their own).

A query is a dict: must and should (lists of groups), msm, must_not (a list of (f, t)). A group is cross_field's ("term", (f, t)) or
("dismax", tie, [(f, t), ...]) or ("sum", msm, [(f, t), ...]): a nested all-SHOULD BooleanQuery of TermQuery clauses.

TreeRef extends CrossRef's composition, in np.float32:
  sum group   ONE DisjunctionSumScorer over the clauses present in the leaf, even when one is left: 0.0f + s_i .. over the present
              clauses that hold the doc, in clause order; cost = the sum of their doc_freq; none present: no scorer
  one side    CrossRef's SHOULD / MUST rules with the sum group's score and cost at its place
  both        hits: every MUST group holds the doc, no MUST_NOT clause does, it is live. req = the MUST side's score (one group: as it
              is; else the stable cost order), opt = 0.0f + g_i .. over the present SHOULD groups on the doc in clause order. Every
              SHOULD group absent: the row is the MUST side's. ReqOptScorer::score (req_opt_scorer.rs:41-66) over the hits in doc
              order: scores_sum (f32) and scores_num start at 0 in every leaf; with scores_num > 100 and 2 * req < scores_sum /
              scores_num the doc scores req and the state stays; else the state takes req and the doc scores req + opt
              (rule=False: req + opt everywhere, rgpu_config.req_opt_rule = -1)
MUTANTS: one model per mistake of the rule, of the two summation orders and of the nesting; tests/test_field_tree_cpu.py shows that
each changes some row of the fixtures, and holds TreeRef against the oracle's own searches where every clause sits in field 0.

The leaf (TreeLeaf): 4099 docs = eight 512-doc windows and a last one of 3 docs, three fields in ONE .doc file.
  field 0 `title`  opt_spectrum.RuleLeaf's lists and norm bytes as they are (rank mode; the statistics RuleLeaf has, so that the
                   searched EQUAL doc keeps 2 * req == sum / num exactly): ALL, THIRD, HOLD, BAN and one lead term per sequence
  field 1 `body`   raw norms (70 distinct bytes): B_ALL, B_THIRD, B_HALF100 (every other doc of S100's range: a lead group of two
                   clauses that share docs), B_400, B_2000, B_0 (absent), B_63 / B_64 / B_65 (that many docs inside ONE 256-doc scan
                   step and nowhere else), B_ENDS (docs 0 and 4098), B_1 (a singleton)
  field 2 `tags`   no norms: G_ALL (freq 2), G_256, G_5"""
import collections

import numpy as np

import cross_field as cf
import opt_spectrum as osp
from cross_field import dismax, term   # noqa: F401  (the tests' vocabulary)

MAX_DOC = osp.R_MAX_DOC
W = cf.W
THRESHOLD = 100
B_ALL, B_THIRD, B_HALF100, B_400, B_2000, B_0, B_63, B_64, B_65, B_ENDS, B_1 = range(11)
G_ALL, G_256, G_5 = range(3)
STEP_OF = {B_63: 6 * W, B_64: 6 * W + 256, B_65: 7 * W}     # the first doc of the scan step that holds the list
T = osp.R_TERM


def sum_(clauses, msm=0):
    return ("sum", int(msm), list(clauses))


def tree(must=(), should=(), msm=0, must_not=()):
    return dict(must=list(must), should=list(should), msm=msm, must_not=list(must_not))


def flat(q):
    """The tree with every sum group replaced by its clauses as term groups: what a parser that does not nest would build"""
    def side(gs):
        return [t for g in gs for t in ([term(*c) for c in g[2]] if g[0] == "sum" else [g])]
    return tree(side(q["must"]), side(q["should"]), q["msm"], q["must_not"])


_built = {}


class TreeLeaf(cf.CrossLeaf):
    def __init__(self, live="none", version=1, which="A"):
        rule = osp.RuleLeaf("rank", live, version, which)
        self.rule = rule
        key = (version, which)
        if key not in _built:
            rng = np.random.default_rng([41, version, ord(which)])
            title = cf.Field(rule.lists, rule.norms, rule.sttf)
            s100 = np.arange(rule.first["S100"], rule.first["S100"] + 120, 2, dtype=np.int32)
            def lst(docs):
                docs = np.asarray(docs, np.int32)
                return docs, cf.freqs_of(rng, docs.size)
            body_lists = [lst(np.arange(MAX_DOC)), lst(np.arange(0, MAX_DOC, 3)), lst(s100), lst(cf.spread(rng, MAX_DOC, 400, (W - 1, W))),
                          lst(cf.spread(rng, MAX_DOC, 2000, (0, MAX_DOC - 1))), lst([])]
            for b, n in ((B_63, 63), (B_64, 64), (B_65, 65)):
                body_lists.append(lst(STEP_OF[b] + np.sort(rng.permutation(256)[:n])))
            body_lists += [lst([0, MAX_DOC - 1]), lst([W + 7])]
            body = cf.Field(body_lists, 60 + rng.permutation(MAX_DOC) % 70, 90 * MAX_DOC)
            tags = cf.Field([(np.arange(MAX_DOC, dtype=np.int32), np.full(MAX_DOC, 2, np.int32)), lst(cf.spread(rng, MAX_DOC, 256, (W - 1, W))),
                             lst(cf.spread(rng, MAX_DOC, 5))], None, 3 * MAX_DOC)
            base = cf.CrossLeaf(MAX_DOC, [title, body, tags], version=version)
            _built[key] = (base.fields, base.doc_bytes)
        fields, doc_bytes = _built[key]
        super().__init__(MAX_DOC, fields, alive=None if live == "none" else rule.alive, version=version, doc_bytes=doc_bytes)


# ---- the reference ------------------------------------------------------------------------------------------------------------------
MUTANTS = collections.OrderedDict([
    ("threshold 99", dict(threshold=99)), ("threshold 101", dict(threshold=101)), (">= for >", dict(ge=True)), ("<= for <", dict(le=True)),
    ("state updated on a skip", dict(update_on_skip=True)), ("state updated only with an optional hit", dict(only_with_opt=True)),
    ("dead lead postings counted", dict(count_dead=True)), ("state carried across leaves", dict(carry=True)),
    ("nested sums flattened", dict(flatten=True)), ("a sum group costs its first clause", dict(sum_cost_first=True)),
    ("the optional side summed in cost order", dict(opt_cost_order=True)), ("the required side summed in clause order", dict(must_clause_order=True)),
    ("the optional sum starts from the required score", dict(opt_into_req=True))])


class State:
    def __init__(self):
        self.sum, self.num = np.float32(0), 0


class TreeRef(cf.CrossRef):
    def __init__(self, oracle, leaf, searchers=None, **mut):
        super().__init__(oracle, leaf, searchers)
        self.mut = mut

    def group(self, g):
        if g[0] != "sum":
            return super().group(g)
        n = self.leaf.max_doc
        present = [c for c in g[2] if self.df(c) > 0]
        if not present:
            return None
        cost = self.df(present[0]) if self.mut.get("sum_cost_first") else sum(self.df(c) for c in present)
        held, total = np.zeros(n, bool), np.zeros(n, np.float32)
        for c in present:
            d, s = self.clause(c)
            total[d] = (np.where(held[d], total[d], np.float32(0.0)) + s).astype(np.float32)
            held[d] = True
        return held, total, cost

    def _side(self, occur, groups, q, order=None):
        return cf.CrossRef.scores(self, dict(occur=occur, groups=groups, msm=q["msm"], must_not=q["must_not"]), order)

    def walk(self, q, rule=True, state=None):
        """-> (hits ascending, final f32 scores, skipped mask, the rule's state afterwards)"""
        mut = self.mut
        if mut.get("flatten"):
            q = flat(q)
        none = np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, bool), state
        if not q["must"] or not q["should"]:
            order = None
            if q["must"] and mut.get("must_clause_order") and self.order(dict(occur="must", groups=q["must"])) is not None:
                order = [self.group(g) for g in q["must"]]
            d, s = self._side("must" if q["must"] else "should", q["must"] or q["should"], q, order)
            return d, s, np.zeros(d.size, bool), state
        req_q = dict(occur="must", groups=q["must"], msm=0, must_not=q["must_not"])
        order = self.order(req_q)
        if order is None:
            return none
        if mut.get("must_clause_order"):
            order = [self.group(g) for g in q["must"]]
        docs, req = self._side("must", q["must"], q, order)
        opts = [o for o in (self.group(g) for g in q["should"]) if o is not None]
        if not opts:
            return docs, req, np.zeros(docs.size, bool), state
        if mut.get("opt_cost_order"):
            opts = sorted(opts, key=lambda o: o[2])
        n = self.leaf.max_doc
        held, opt = np.zeros(n, bool), np.zeros(n, np.float32)
        for h, sc, _ in opts:
            opt[h] = (np.where(held[h], opt[h], np.float32(0.0)) + sc[h]).astype(np.float32)
            held |= h
        o, oh = np.where(held, opt, np.float32(0.0)).astype(np.float32)[docs], held[docs]
        if mut.get("opt_into_req"):    # req + g1 + g2 instead of req + (0.0f + g1 + g2)
            full = req.copy()
            for h, sc, _ in opts:
                full[h[docs]] = (full[h[docs]] + sc[docs][h[docs]]).astype(np.float32)
        else:
            full = (req + o).astype(np.float32)
        if not rule:
            return docs, full, np.zeros(docs.size, bool), state
        st = state if (state is not None and mut.get("carry")) else State()
        thr = mut.get("threshold", THRESHOLD)
        final, skipped = np.zeros(docs.size, np.float32), np.zeros(docs.size, bool)
        lead_held, lead_score, _ = order[0]
        at = {int(d): i for i, d in enumerate(docs)}
        for d in np.flatnonzero(lead_held):          # the lead group's postings in doc order
            i = at.get(int(d))
            if i is None:                            # no hit: another MUST group lacks it, a MUST_NOT clause holds it, or it is deleted
                if mut.get("count_dead"):
                    st.sum, st.num = np.float32(st.sum + lead_score[d]), st.num + 1
                continue
            r = req[i]
            skip = False
            if (st.num >= thr) if mut.get("ge") else (st.num > thr):
                two, mean = np.float32(2.0) * r, np.float32(st.sum) / np.float32(st.num)
                skip = bool(two <= mean) if mut.get("le") else bool(two < mean)
            if skip:
                final[i], skipped[i] = r, True
                if mut.get("update_on_skip"):
                    st.sum, st.num = np.float32(st.sum + r), st.num + 1
                continue
            if not mut.get("only_with_opt") or oh[i]:
                st.sum, st.num = np.float32(st.sum + r), st.num + 1
            final[i] = full[i]
        return docs, final, skipped, st

    def scores(self, q, order=None, rule=True):
        if "occur" in q:      # a cross_field query
            return super().scores(q, order)
        d, s, _, _ = self.walk(q, rule)
        return d, s

    def rows(self, q, k=None, rule=True):
        docs, sc = self.scores(q, rule=rule)
        o = np.lexsort((docs, -sc.astype(np.float64)))
        n = docs.size if k is None else min(int(k), docs.size)
        return docs[o][:n], sc[o][:n], int(docs.size)


def index_refs(oracle, leaves, **mut):
    base = 0
    for leaf in leaves:
        leaf.doc_base = base
        base += leaf.max_doc
    searchers = {f: oracle.Searcher([leaf.oracle_segment(oracle, f) for leaf in leaves], k1=cf.K1) for f in range(len(leaves[0].fields))}
    return [TreeRef(oracle, leaf, searchers, **mut) for leaf in leaves]


def index_rows(refs, q, k, rule=True):
    """The merged row of an index: every leaf sums in its own orders and starts the rule's state afresh (MUTANT carry: it does not)"""
    docs, sc, st = [], [], None
    for r in refs:
        d, s, _, st = r.walk(q, rule, st)
        docs.append(d + np.int32(r.leaf.doc_base))
        sc.append(s)
    docs, sc = np.concatenate(docs), np.concatenate(sc)
    o = np.lexsort((docs, -sc.astype(np.float64)))
    return docs[o][:k], sc[o][:k], int(docs.size)


def check_row(row, total, ref, q, what, rule=True):
    """One row of search_fields_tree_batch against TreeRef: doc ids, score bits, -1 padding and the hit count, exact"""
    k = row.size
    d, s, tot = ref.rows(q, k, rule=rule)
    assert int(total) == tot, (what, "total", int(total), tot)
    n = min(k, tot)
    assert (row["doc"][n:] == -1).all() and (row["score"][n:] == 0).all(), (what, "padding", row["doc"][:8], n)
    assert (row["doc"][:n] == d).all(), (what, "docs", row["doc"][:8], d[:8])
    assert (row["score"][:n].view(np.int32) == s.view(np.int32)).all(), (what, "score bits", row["score"][:4], s[:4])


# ---- the queries ----------------------------------------------------------------------------------------------------------------------
OPT_BOTH = sum_([(0, T["ALL"]), (1, B_ALL)])      # the optional word over title and body: every doc carries it


def rule_query(name, lead="sum"):
    """A sequence of opt_spectrum searched as `+seq word`: the lead group holds the sequence's title term alone (as a sum group of one
    clause or as a term group), so req is the score the sequence was laid out for"""
    t = (0, T[name])
    first = sum_([t]) if lead == "sum" else term(*t)
    if name == "DEAD_LACK":
        return tree([first, term(0, T["HOLD"])], [OPT_BOTH])
    if name == "DEAD_ALL":
        return tree([first, term(0, T["HOLD"])], [OPT_BOTH], must_not=[(0, T["BAN"])])
    if name == "DEAD_NOT" or name.startswith("STEP_"):
        return tree([first], [OPT_BOTH], must_not=[(0, T["BAN"])])
    return tree([first], [OPT_BOTH])


RULE_NAMES = ["S99", "S100", "S101", "KEEPS_STATE", "DEAD_LACK", "DEAD_NOT", "DEAD_DEL", "DEAD_ALL", "STEP_127", "STEP_128", "DF_129", "DF_257", "EQUAL",
              "TWO"]


def rule_queries():
    out = collections.OrderedDict((n, rule_query(n)) for n in RULE_NAMES)
    out["S100 term lead"] = rule_query("S100", "term")
    out["OPT_MISS"] = tree([sum_([(0, T["S100"])])], [sum_([(0, T["THIRD"]), (1, B_THIRD)])])           # docs no optional group holds
    out["two-clause lead"] = tree([sum_([(0, T["S100"]), (1, B_HALF100)])], [OPT_BOTH])              # a lead group whose clauses share docs
    out["KEEPS two-field"] = tree([sum_([(0, T["KEEPS_STATE"]), (1, B_0)]), term(2, G_ALL)], [OPT_BOTH, term(2, G_256)])   # a conjunction, two optional groups
    return out


NINE = [(1, B_400), (0, T["THIRD"]), (2, G_256), (1, B_2000), (0, T["S101"]), (2, G_5), (1, B_1), (1, B_63), (0, T["BAN"])]


def sum_queries():
    """Sum groups on one side, and beside dismax and term groups"""
    a, b, c = (0, T["THIRD"]), (1, B_400), (1, B_2000)
    return collections.OrderedDict([
        ("one clause", tree(should=[sum_([b])])),
        ("two clauses", tree(should=[sum_([a, b])])),
        ("nine clauses", tree(should=[sum_(NINE)])),
        ("eight present of nine", tree(should=[sum_(NINE[:4] + [(1, B_0)] + NINE[4:8])])),
        ("a clause absent", tree(should=[sum_([(1, B_0), b, a])])),
        ("a group absent under SHOULD", tree(should=[sum_([(1, B_0)]), sum_([a, b])])),
        ("every group absent", tree(should=[sum_([(1, B_0)])])),
        ("a group absent under MUST", tree([sum_([(1, B_0)]), sum_([a, b])])),
        ("nested msm 0", tree(should=[sum_([a, b], 0), sum_([c, (2, G_256)], 0)])),
        ("nested msm 1", tree(should=[sum_([a, b], 1), sum_([c, (2, G_256)], 1)], msm=1)),
        ("nested against flat", tree(should=[sum_([(1, B_ALL), b]), sum_([c, (0, T["ALL"])]), sum_([(2, G_256), a])])),
        ("msm 2 counts groups", tree(should=[sum_([a, b]), sum_([c, (2, G_256)]), term(2, G_5)], msm=2)),
        # MUST: a sum group's cost (400 + 2000 = 2400) against a term's doc_freq: B_ALL 4099 above, T_ALL 4099; equal: 256 + 5 = 261 ...
        ("sum cost below a term", tree([term(1, B_ALL), sum_([b, c])])),
        ("sum cost above a term", tree([sum_([(1, B_ALL), b]), term(1, B_2000), term(2, G_ALL)])),
        ("sum cost equal to a term's, sum second", tree([term(1, B_ALL), sum_([(2, G_ALL)]), term(0, T["ALL"])])),     # 4099 each: the stable order
        ("sum cost equal to a term's, sum first", tree([sum_([(2, G_ALL)]), term(0, T["ALL"]), term(1, B_ALL)])),
        ("sum cost equal, sum first", tree([sum_([(1, B_2000), (1, B_ALL)]), sum_([(2, G_ALL), c]), term(0, T["ALL"])])),
        ("sum cost equal, sum second", tree([sum_([(2, G_ALL), c]), term(0, T["ALL"]), sum_([(1, B_2000), (1, B_ALL)])])),
        ("sum, dismax and term under SHOULD", tree(should=[sum_([a, b]), dismax(0.3, [(0, T["HOLD"]), c]), term(2, G_256)], must_not=[(2, G_5)])),
        ("sum, dismax and term under MUST", tree([term(2, G_ALL), dismax(0.3, [(0, T["HOLD"]), c]), sum_([a, b])], must_not=[(1, B_1)])),
        ("MUST side alone", tree([sum_([a, b])], [sum_([(1, B_0)])])),                 # every SHOULD group absent
        ("dead beside SHOULD", tree([sum_([(1, B_0)])], [sum_([a, b])])),              # a MUST group absent
    ])


def emission_queries():
    """Required/optional queries for the record emission: the lead group's entries per item, per scan step, at the leaf's ends"""
    opt = [sum_([(0, T["THIRD"]), (1, B_THIRD)]), term(2, G_256), term(1, B_2000)]      # clause order is not cost order
    out = collections.OrderedDict()
    for b, n in ((B_63, 63), (B_64, 64), (B_65, 65)):
        out["%d hits in a step" % n] = tree([sum_([(1, b)])], opt)                      # every other item has no lead entry
    out["both ends"] = tree([term(1, B_ENDS)], opt)
    out["every doc"] = tree([sum_([(0, T["ALL"])])], opt)                               # every lead entry of every item matches
    out["every doc twice"] = tree([sum_([(0, T["ALL"]), (1, B_ALL)])], opt)             # ... and is counted twice by the capacity
    out["a singleton lead"] = tree([term(1, B_1)], opt)
    out["thin conjunction"] = tree([term(2, G_ALL), term(1, B_2000), sum_([(1, B_400), (2, G_5)])], opt, must_not=[(2, G_256)])   # most lead entries are no hits
    out["msm beside MUST"] = tree([term(1, B_400)], opt, msm=7)                         # accepted, no effect
    return out


# ---- the C ABI's arrays -------------------------------------------------------------------------------------------------------------
KIND = {"term": 0, "dismax": 1, "sum": 2}


def pack(ref, queries, sim_tables, field_of=lambda f: f):
    """queries (dicts) -> (rgpu_fields_tree_query[], rgpu_field_tree_group[], rgpu_field_clause[])"""
    from rucene_amd import _lib
    Q, G, C = [], [], []

    def clause(c, scored=True):
        row = np.zeros(1, _lib.FIELD_CLAUSE_DTYPE)[0]
        row["state"] = ref.leaf.fields[c[0]].terms[c[1]]
        if scored:
            row["weight"], row["sim_table"] = ref.weight(c)[0], sim_tables[c[0]]
        row["field"] = field_of(c[0])
        C.append(row)
    for q in queries:
        g0 = len(G)
        for g in q["must"] + q["should"]:
            c0 = len(C)
            for c in cf.group_clauses(g):
                clause(c)
            tie = np.float32(g[1] if g[0] == "dismax" else 0.0)
            G.append((c0, len(C) - c0, int(tie.view(np.uint32)), KIND[g[0]], g[1] if g[0] == "sum" else 0, 0))
        n0 = len(C)
        for c in q["must_not"]:
            clause(c, scored=False)
        Q.append((g0, len(q["must"]), len(q["should"]), q["msm"], n0, len(C) - n0))
    return (np.array(Q, _lib.FIELDS_TREE_QUERY_DTYPE), np.array(G, _lib.FIELD_TREE_GROUP_DTYPE),
            np.array(C, _lib.FIELD_CLAUSE_DTYPE) if C else np.zeros(0, _lib.FIELD_CLAUSE_DTYPE))
