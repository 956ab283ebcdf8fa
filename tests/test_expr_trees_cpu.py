"""Guards of the expression-tree generator (tests/expr_tree_cases.py), which need no GPU: they evaluate the ORACLE only, so that a
later edit of the generator cannot hollow out test_expr_trees_gpu.py — trees that are the same on every call, that the oracle can
judge, that produce NULLs and values, predicates that select some rows and not all, every node kind and cast pair present.  The last
test builds every case's plan over a device-less leaf: what the compiler refuses at plan time is already visible here."""
from collections import OrderedDict

import numpy as np
import pytest

import ballista_amd as ba
from oracle import engine as og, plan_eval
from oracle.engine import OCol

import expr_tree_cases as X
import plan_nodes as N
import proto_encode as pe

N_BIG = 1537


def _leaf(n):
    return N.MemoryExec([[X.batch(n)]])


@pytest.mark.parametrize("family", X.FAMILIES)
def test_same_seed_same_trees(family):
    for seed in X.SEEDS:
        X.cases.cache_clear()
        a = [X.to_string(t) for c in X.cases(family, seed) for t in c.trees]
        X.cases.cache_clear()
        b = [X.to_string(t) for c in X.cases(family, seed) for t in c.trees]
        assert a == b
        assert len(a) >= X.TREES_PER_FAMILY
    assert [X.to_string(t) for c in X.cases(family, X.SEEDS[0]) for t in c.trees] != [X.to_string(t) for c in X.cases(family, X.SEEDS[1]) for t in c.trees]


@pytest.mark.parametrize("family", X.FAMILIES)
def test_oracle_judges_every_tree(family):
    """no generated tree makes the oracle raise — on the case's own batch and on the 1537-row one; at least half of the trees
    give both NULL and non-NULL rows; the share of NaN results is printed"""
    both = total = nan_rows = rows = 0
    for seed in X.SEEDS:
        for c in X.cases(family, seed):
            plan_eval.collect(X.build_plan(N, c, _leaf(c.n_rows)))            # the whole plan, as the GPU tier compares it
            for t in c.trees:
                v = og.evaluate(t, X.batch(N_BIG))
                ok = v.is_valid()
                total += 1
                both += bool(ok.any() and not ok.all())
                if v.dtype in X.FLOATS:
                    nan_rows += int(np.isnan(v.values[ok]).sum())
                    rows += int(ok.sum())
    print(f"{family}: {total} trees, {both} with NULL and non-NULL rows, NaN share of the valid float rows {nan_rows / max(rows, 1):.3f}")
    assert 2 * both >= total, (family, both, total)


def test_filter_predicates_select_some_rows():
    """at least 80 % of the filter predicates keep between 1 and n-1 of the 1537 rows"""
    some = total = 0
    for seed in X.SEEDS:
        for c in X.cases("filter", seed):
            p = og.evaluate(c.predicate, X.batch(N_BIG))
            kept = int((p.values & p.is_valid()).sum())
            total += 1
            some += 1 <= kept <= N_BIG - 1
    print(f"filter: {some} of {total} predicates keep 1 .. n-1 rows")
    assert some >= 0.8 * total, (some, total)


def test_every_node_kind_and_cast_pair_occurs():
    kinds, casts = set(), set()
    for family in X.FAMILIES:
        for seed in X.SEEDS:
            for c in X.cases(family, seed):
                for t in c.trees:
                    k, cs = X.kinds_of(t)
                    kinds |= k
                    casts |= cs
    assert not set(X.NODE_KINDS) - kinds, sorted(set(X.NODE_KINDS) - kinds)
    assert not set(X.CAST_PAIRS) - casts, sorted(set(X.CAST_PAIRS) - casts)


def test_batch_carries_the_edge_values():
    b = X.batch(N_BIG)
    for name, t in X.SCHEMA.items():
        c = b[name]
        assert c.dtype == t
        if name.startswith("k") or t == "Boolean":
            continue
        share = 1 - c.is_valid().mean()
        assert 0.08 < share < 0.17, (name, share)
        edges = X._F64_EDGES if t == "Float64" and name == "f64" else X._F32_EDGES if t == "Float32" else X._int_edges(t) if t in X.INTS else []
        for on in (True, False):                           # every edge value in a valid row and in a NULL row
            have = c.values[c.is_valid() == on]
            for e in edges:
                e = np.asarray(e).astype(c.values.dtype)
                if name.endswith("nz") and e == 0:
                    continue
                assert (np.isnan(have).any() if e != e else ((have == e) & (np.signbit(have) == np.signbit(e))).any()), (name, e, on)
    for name in ("u8nz", "u16nz", "u32nz", "u64nz"):
        assert (b[name].values != 0).all()
    assert X.batch(1)["f64"].values.shape == (1,)


def _decoded_leaf():
    """a leaf with the batch's schema that needs no device: an empty scan, encoded and decoded as a wire plan"""
    b = X.batch(1)
    cols = [(n, c.dtype, c.valid is not None or n not in ("k3", "k7", "k300")) for n, c in b.items()]
    m = N.MemoryExec([[OrderedDict((n, OCol(t, np.zeros(0, og.NP_TYPES[t]), np.zeros(0, np.bool_) if u else None)) for n, t, u in cols)]], schema=cols)
    m.name = "mem://expr_trees"
    return ba.ExecutionPlan.from_proto(None, pe.plan(m))


@pytest.mark.parametrize("family", X.FAMILIES)
def test_plan_tier_refusals_stay_under_the_cap(family):
    """every case's trees through the compiler at plan time (Projection and Filter compile there; an aggregate's arguments and key
    parts are compiled as the outputs of a projection): at most 10 % may be refused, and only with one of the builder's limit
    messages"""
    leaf = _decoded_leaf()
    refused, total, seen = 0, 0, set()
    for seed in X.SEEDS:
        for c in X.cases(family, seed):
            total += 1
            try:
                if c.predicate is not None:
                    ba.FilterExec(c.predicate, leaf)
                outs = c.exprs or [(a.expr, f"a{j}") for j, a in enumerate(c.aggs) if not isinstance(a.expr, ba.expr.Column)] + \
                    [(e, n) for e, n in c.group if not isinstance(e, ba.expr.Column)]
                if outs:
                    ba.ProjectionExec(outs, leaf)
            except ba.NotImplementedOnGpu as e:
                assert X.is_limit_refusal(str(e)), (c.describe(), str(e))
                refused += 1
                seen.add(str(e))
    print(f"{family}: {total - refused} planned, {refused} refused {sorted(seen)}")
    assert refused <= 0.1 * total, (refused, total, sorted(seen))
