"""The step table of tests/sequence_cases.py meets its own conditions, from the models alone: every step
is the case it claims to be, so an edit of a generator cannot quietly turn a case into an easy one."""
import numpy as np
import pytest

import sequence_cases as sc


@pytest.fixture(scope="module")
def T(oracle):
    return sc.table(oracle)


def _by(T):
    return {s.name: s for steps in T.values() for s in steps}


def test_names_and_sets(T):
    assert {p: [s.name for s in steps] for p, steps in T.items()} == sc.STEP_NAMES
    by = _by(T)
    assert len(by) == sum(len(v) for v in sc.STEP_NAMES.values())
    for s in by.values():
        assert s.src is None or (by[s.src].pset == s.pset and by[s.src].out is not None), s.name
        assert s.refuse or s.want, s.name


def test_route_selecting_sizes(T):
    by = _by(T)
    want = {"add32": 32, "sub32": 32, "add33": 33, "sub33": 33, "add64": 64, "sub64": 64, "add65": 65, "sub65": 65,
            "add_deep": 30001}
    for name, L in want.items():
        s = by[name]
        assert s.want["max_layers"] == L and s.want["n_large"] == 0, name
        assert all(x.nL + y.nL == L for x, y in zip(s.aux["xs"], s.aux["ys"])), name
        assert len(s.aux["xs"]) % 2 == 1, name                      # the pair counts are odd
        assert s.inp["negate"] == name.startswith("sub")
    assert by["add_deep"].limit == sc.LIMIT_DEEP and by["add_deep"].route == {"deep.add": 1}
    assert all(by[n].pset == ("wide" if L in (33, 64) else "main") for n, L in want.items())
    assert by["ref_layer_limit"].limit == sc.LIMIT_DEFAULT


def _depth(layers, l, seen=()):
    if layers[l]["rule"] != 1 or l in seen:
        return 0
    return 1 + max(_depth(layers, int(layers[l][f]), seen + (l,)) for f in ("pa", "pb"))


@pytest.mark.parametrize("name", ["add32", "sub32", "add33", "sub33", "add64", "sub64", "add65", "sub65"])
def test_closure_pairs(T, name):
    s = _by(T)[name]
    G, L, budget = s.aux["G"], s.aux["L"], sc.BUDGET[s.pset]
    for x, y, o, twin in zip(s.aux["xs"], s.aux["ys"], s.out, s.aux["twins"]):
        nE = x.nE + y.nE
        assert nE <= budget and o.nE == nE                          # under the budget: a concatenation
        if G:
            assert nE > sc.PRE * G                                  # both tail loops run
        if twin:
            assert o.nL == L                                        # the identity remap
            continue
        assert 0 < o.nL < L                                         # layers are dropped
        named = set(o.layer_id().tolist())
        base = [l for l in range(o.nL) if o.layers[l]["rule"] == 0]
        assert any(l not in named for l in base)                    # a BASE layer kept through the chain only
        assert max(_depth(o.layers, l) for l in range(o.nL)) >= 3   # a PROD chain three deep
        assert any(o.layers[l]["rule"] == 1 and max(int(o.layers[l]["pa"]), int(o.layers[l]["pb"])) > l
                   for l in range(o.nL))                            # a parent above its child
        # the tail-only layer: B's layer 7, named by edges at positions >= PRE * G of the concatenation only
        lid = np.concatenate([x.layer_id().astype(np.int64), y.layer_id().astype(np.int64) + x.nL])
        at = np.flatnonzero(lid == x.nL + 7)
        assert len(at) == 1 and at[0] == nE - 1
        if G:
            assert at[0] >= sc.PRE * G
        # the last layer is kept and a dropped one lies below it: 1 << l and (1 << l) - 1 at l = L - 1
        assert L - 1 in lid and len(set(range(L - 1)) - set(lid.tolist())) > 0


def test_budget_sides(T):
    by = _by(T)
    for name in ("merge_add", "merge_sub"):
        s = by[name]
        over = [x.nE + y.nE > sc.BUDGET["main"] for x, y in zip(s.aux["xs"], s.aux["ys"])]
        assert over == s.aux["over"] and s.want["n_large"] == sum(over) == 3
        assert s.aux["xs"][1] is s.aux["ys"][1]                      # A op A
        assert (s.aux["xs"][3].w_hi >> np.uint64(63)).any()          # non-canonical weights
        assert len(np.unique(s.aux["xs"][2].meta)) < s.aux["xs"][2].nE // 2   # heavy duplicates
    assert all(o.nE < x.nE + y.nE for s in (by["merge_add"], by["merge_sub"])    # the merge found groups to fold
               for x, y, o, v in zip(s.aux["xs"], s.aux["ys"], s.out, s.aux["over"]) if v)
    # ct_mul: within the budget except where the step says otherwise
    for name in ("mul_fresh", "mul_cancel", "mul_general", "mul_sigma", "mul_pending"):
        s = by[name]
        assert all(sc.product_cells(x, y) <= sc.BUDGET["main"] for x, y in zip(s.inp["xs"], s.inp["ys"])), name
    for name in ("mul_over", "mul_wide"):
        s = by[name]
        assert sum(o.nE > sc.BUDGET["main"] for o in s.out) >= 2, name
    assert by["mul_over"].want["n_small"] == 3 and by["mul_fresh"].want["n_small"] == 5
    assert by["mul_general"].want["n_large"] == 2
    assert all((x.nL, y.nL) == (8, 2) for x, y in zip(by["mul_general"].inp["xs"], by["mul_general"].inp["ys"]))
    la = by["link_add"]
    assert 0 < la.want["n_large"] < len(la.out)                      # the linked add mixes both sides too


@pytest.mark.parametrize("name", ["mul_cancel", "mul_direct"])
def test_cancelling_pair(T, name):
    s = _by(T)[name]
    p = s.aux["cancel"]
    for q, (x, y, o) in enumerate(zip(s.inp["xs"], s.inp["ys"], s.out)):
        cells = sc.product_cells(x, y)
        assert o.nE == cells - (q == p), q                           # fewer keys than distinct products
    assert s.route["mul.redo"] == 1


def test_general_path_modes(T):
    """The direct mode runs in the wide set's mul_direct (and its cancelling pair comes back on the iblk order);
    every other general-path pair of the table keeps the dynamic chains: 8 x 2 layers are 5,392 key slots over
    the 97 buckets of 96 products."""
    by = _by(T)
    d = by["mul_direct"]
    assert (d.want["n_large"], d.route["mul.general"], d.route["mul.direct"], d.route["mul.iblk"]) == (3, 4, 3, 4)
    for s in by.values():
        if s.op in ("mul", "mul_pending") and s is not d:
            assert s.route["mul.iblk"] == 0 and s.route["mul.direct"] == 0, s.name
    assert by["gather"].route["gather.tiles"] > 0


def _in_contract(c):
    prod = c.layers["rule"] == 1
    return bool((c.layer_id() < c.nL).all() and (c.layers["pa"][prod] < c.nL).all() and (c.layers["pb"][prod] < c.nL).all())


def test_lincomb_segments(T):
    by = _by(T)
    for name in ("sum_routes", "sum_fold", "sum_deep", "link_sum"):
        s = by[name]
        pool, so, term = s.aux["pool"], s.inp["seg_off"], s.inp["term"]
        for i, st in enumerate(s.want["status"]):
            terms = [pool[int(t)] for t in term[int(so[i]):int(so[i + 1])]]
            stray = not all(_in_contract(c) for c in terms)
            over = sum(c.nE for c in terms) > sc.BUDGET["main"]
            assert st == (2 if stray else 1 if over else 0), (name, i)
    assert by["sum_fold"].want["status"] == [1, 2, 0, 0]             # the only status 2 of the table
    assert all(2 not in by[n].want["status"] for n in ("sum_routes", "sum_deep", "link_sum"))
    assert by["sum_fold"].out[1].nL == 4                             # the stray edge kept the partner's unused layer
    r = by["sum_routes"]
    assert r.route["lin.wave_terms"] > 0 and r.route["lin.wg_terms"] > 0 and r.inp["flags"].any()
    assert not r.inp["flags"].all()
    assert by["sum_deep"].route["deep.lin_terms"] == 1 and by["sum_deep"].limit == sc.LIMIT_DEEP


def test_other_routes(T):
    by = _by(T)
    assert by["compact_routes"].route == {"compact.small": 4, "compact.merge": 1}
    it = by["recrypt"].want["iters"]
    assert 0 in it and 8 in it and any(0 < k < 8 for k in it) and len(by["recrypt"].inp["pool"]) == 4
    assert by["chain"].want["pair_steps"] == 12 and len(by["chain"].inp["xs"]) == 4
    assert by["check_gsum"].want["status"] == [0] * 5
    for s in by.values():
        assert (s.refuse is not None) == s.name.startswith("ref_")
        assert all(isinstance(v, int) and v >= 0 for v in s.route.values()), s.name


def test_second_build_is_identical(T, oracle):
    again = sc.build(oracle)
    for pset, steps in T.items():
        for a, b in zip(steps, again[pset]):
            assert (a.name, a.op, a.src, a.limit, a.route, a.refuse) == (b.name, b.op, b.src, b.limit, b.route, b.refuse)
            assert a.want.keys() == b.want.keys()
            for key in a.want:
                assert sc.same_value(a.want[key], b.want[key]), (a.name, key)


def test_orders(T):
    for pset, steps in T.items():
        names = [s.name for s in steps]
        src = sc.producers(steps)
        orders = [sc.order_of(steps, w) for w in sc.ORDERS]
        assert len(orders) == 7
        for o in orders:
            assert sorted(o) == sorted(names)
            assert all(src[n] is None or o.index(src[n]) < o.index(n) for n in o)
        assert len({tuple(o) for o in orders}) == 7, pset
    for steps in T.values():                                         # the largest, then at once the smallest
        ls = sc.order_of(steps, "large_small")
        for op in {s.op for s in steps}:
            mine = [s for s in steps if s.op == op and not s.refuse and not s.src]
            if len(mine) >= 2:
                big, small = max(mine, key=lambda s: s.size).name, min(mine, key=lambda s: s.size).name
                assert big != small and ls.index(small) == ls.index(big) + 1, op
    ls = sc.order_of(T["main"], "large_small")
    assert ls.index("add32") == ls.index("add_deep") + 1
