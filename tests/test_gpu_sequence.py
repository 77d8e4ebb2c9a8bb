"""One context held to the CPU models across interleaved operations.

tests/sequence_cases.py is a table of steps, one per family of operation and route, each answered on the
CPU by the oracle and the models on top of it. test_step_alone runs every step on a fresh Engine (a consumer
step after its producers): that is the kernel test, and for the ct_add wave kernels' closure, size and
tail-loop cases the only one. test_sequence runs the whole table on ONE Engine per parameter set in seven
orders, comparing every array of every step exactly and the delta of every counter of the engine with the
step's declared route: a small call after a large one must ignore what the shared plan scratch, merge
state, grown buffers and cached host flags of the context (csrc/ctx.hpp) still hold, and a refused call in
the middle must leave the next result exact. Nothing is sampled and there is no tolerance: integer and
byte work throughout."""
import ctypes as C

import numpy as np
import pytest

import sequence_cases as sc
from helpers import Cipher

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def table(oracle):
    """Inputs and expected values of every step, computed once."""
    return sc.table(oracle)


@pytest.fixture(scope="module")
def key_material():
    return sc.keys()


# ------------------------------------------------------------------------------------ the engine side
def make_engine(pset, k):
    """A context of the set's parameters with the key material every step may need, set once."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pvac_hfhe_cppbyv_amd import Engine
    eng = Engine(device=0, B=sc.B, m_bits=sc.M_BITS, edge_budget=sc.BUDGET[pset], canon_tag=k["canon_tag"])
    assert eng.gen_H() == k["H_digest"]
    eng.set_H_digest(k["H_digest"])
    em = k["em"]
    eng.set_secret(k["prf_k"], k["lpn_s"], em["lpn_n"], em["lpn_t"], em["lpn_tau_num"], em["lpn_tau_den"])
    eng.set_powg(k["powg"])
    eng.set_ubk(k["ubk_inv"])
    eng.drbg_seed(bytes(range(48)))
    return eng


def counters(eng):
    d = {"mul." + a: b for a, b in eng.ct_mul_path_counts().items()}
    d["mul.redo"] = eng.ct_mul_redo_count()
    d["deep.mul"], d["deep.add"] = eng.deep_path_counts()
    d["deep.lin_terms"], d["deep.fold_sums"], d["deep.compact"], d["deep.recrypt"] = eng.deep_route_counts()
    d.update({"lin." + a: b for a, b in eng.ct_lincomb_path_counts().items()})
    d.update({"compact." + a: b for a, b in eng.compact_path_counts().items()})
    d.update({"gather." + a: b for a, b in eng.gather_path_counts().items()})
    d.update({"img." + a: b for a, b in eng.ct_image_path_counts().items()})
    d.update({"metrics." + a: b for a, b in eng.metrics_path_counts().items()})
    d.update({"gsum." + a: b for a, b in eng.check_mul_gsum_path_counts().items()})
    d.update(dict(zip(("enc.narrow", "enc.wide", "enc.sub", "enc.runs"), eng.enc_path_counts())))
    return d


def dev(eng, ciphers, sigma=False):
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    return DeviceBatch.from_host(ciphers, eng.device, sigma=sigma)


def host(batch):
    return [Cipher(c.layers, c.meta, c.w_lo, c.w_hi, c.sigma) for c in batch.to_host()]


def i64(eng, a):
    return eng.torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(eng.device)


def clone(X):
    """The batch in new device arrays of the same layout (capacity padding kept): for the in-place operations."""
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    c = lambda t: None if t is None else t.clone()
    return DeviceBatch(X.n, c(X.l_off), c(X.l_cnt), c(X.layers), c(X.e_off), c(X.e_cnt), c(X.meta), c(X.w_lo), c(X.w_hi),
                       c(X.sigma))


def ct_add(eng, A, Bb, negate, sigma):
    """Engine.ct_add, returning the plan too (its max_layers picks the kernel, its n_large the merge set)."""
    from pvac_hfhe_cppbyv_amd import DeviceBatch, Plan
    torch = eng.torch
    z = lambda: torch.zeros(max(A.n, 1), dtype=torch.int64, device=eng.device)
    C_ = DeviceBatch(A.n, z(), z(), None, z(), z(), None, None, None)
    plan = Plan()
    sa, sb, sc_ = A.struct(), Bb.struct(), C_.struct()
    eng._check(eng.lib.pvac_hip_ct_add_plan(eng.ctx, C.byref(sa), C.byref(sb), C.byref(sc_), C.byref(plan)))
    e = max(plan.total_edge_slots, 1)
    C_.layers = torch.empty((max(plan.total_layer_slots, 1), 5), dtype=torch.int64, device=eng.device)
    C_.meta, C_.w_lo, C_.w_hi = (torch.empty(e, dtype=torch.int64, device=eng.device) for _ in range(3))
    if sigma:
        C_.sigma = torch.empty((e, 128), dtype=torch.int64, device=eng.device)
    sc_ = C_.struct()
    eng._check(eng.lib.pvac_hip_ct_add_exec(eng.ctx, C.byref(plan), C.byref(sa), C.byref(sb), int(negate), C.byref(sc_)))
    return C_, plan


def refused(eng, st, call):
    from pvac_hfhe_cppbyv_amd import PvacError
    code, msg = st.refuse
    with pytest.raises(PvacError) as err:
        call()
    assert f"error {code}:" in str(err.value) and msg in str(err.value), str(err.value)


# ------------------------------------------------------------------------------------ one runner per operation
def between_plan_and_exec(eng, st, A, Bb, Cb, plan):
    """Every operation of sequence_cases.PENDING_SAFE, in its order, on inputs of its own (A, Bb, Cb, plan: the
    pending ct_mul, which fill_nonces reads)."""
    from pvac_hfhe_cppbyv_amd import ENC_ITEM_FP, ENC_ITEM_VALUE, FP_MUL
    torch = eng.torch
    X = dev(eng, st.inp["mid"], True)
    t = torch.empty(128, dtype=torch.int64, device=eng.device)
    F = eng.gen_fresh(3, 0x5EC)                  # 3 ciphers of 2 layers: a triple for check_mul_gsum's reads
    E = {}

    def enc_value():
        E["X"], status = eng.enc_value(st.inp["enc_vals"], st.inp["enc_rnd"])
        assert not status.any()

    def enc_value_depth():
        draws = eng.enc_caps(2)[2]
        _, status = eng.enc_value(st.inp["enc_vals"][:1], np.resize(st.inp["enc_rnd"], (1, draws)), depth=2)
        assert not status.any()

    def enc_items():
        items = [(ENC_ITEM_VALUE, 5, 0), (ENC_ITEM_FP, 7, 2)]
        hint = [int(h) for h in eng.enc_items_caps([(k, v, h, 0, 0) for k, v, h in items])[2]]
        full = [(k, v, h, sum(hint[:i]), hint[i]) for i, (k, v, h) in enumerate(items)]
        _, status = eng.enc_items(full, np.resize(st.inp["enc_rnd"], sum(hint)))
        assert not status.any()

    def chain():
        assert eng.ct_mul_chain(dev(eng, [st.inp["xs"][0], st.inp["xs"][2]]), 1, streams=1, chunk=2)["pair_steps"] == 2

    def limits():
        eng.set_layer_limit(sc.LIMIT_DEEP)
        eng.set_layer_limit(st.limit)

    calls = {
        "dec_value": lambda: eng.dec_value(X, st.inp["mid_R"]),
        "gather_select": lambda: E.update(sel=eng.select(X, [2, 0, 1])),
        "gather_cat": lambda: eng.cat([E["sel"], X]),
        "ct_scale": lambda: eng.ct_scale(clone(X), 5),
        "commit_ct": lambda: eng.commit_ct(X),
        "ct_image": lambda: E.update(img=eng.ct_image(X, sc.M_BITS, return_pos=True)),
        "ct_from_image": lambda: eng.ct_from_image(E["img"][0], E["img"][1], 3, sc.M_BITS, 6, 90),
        "sigma_bytehist": lambda: eng.sigma_bytehist(X),
        "layer_gsum": lambda: eng.layer_gsum(X),
        "sigma_popcount": lambda: eng.sigma_popcount(X),
        "ubk_apply": lambda: eng.ubk_apply(clone(X)),
        "digest": lambda: eng.digest(X),
        "sumdigest": lambda: eng.sumdigest(X),
        "pack": lambda: eng.pack(X),
        "fp_binop": lambda: eng.fp_binop(FP_MUL, t[:16], t[16:32], t[32:48], t[48:64]),
        "fp_inv": lambda: eng.fp_inv(12345),
        "fill_random": lambda: eng.fill_random(t, 1),
        "drbg_fill": lambda: eng.drbg_fill(t),
        "drbg_reseed": lambda: eng.drbg_reseed(bytes(48)),
        "aes256_ctr": lambda: eng.aes256_ctr(bytes(32), bytes(16), 64),
        "prf": lambda: eng.prf(6, np.arange(6, dtype=np.uint64).reshape(2, 3)),
        "enc_value": enc_value,
        "enc_value_depth": enc_value_depth,
        "enc_items": enc_items,
        "base_R": lambda: eng.base_R(E["X"]),
        "sigma": lambda: eng.sigma(clone(X), t),   # 90 edge slots, 128 salts
        "gen_fresh": lambda: eng.gen_fresh(2, 7),
        "fill_nonces": lambda: eng.fill_nonces(A, Bb, Cb, plan, 9),
        "check_mul_gsum": lambda: eng.check_mul_gsum(F, F, F, t),   # slots 0 .. 11 of the nonce array
        "ct_mul_chain": chain,
        "set_layer_limit": limits,
        "timing_reset": lambda: eng.timing_reset(),
    }
    assert list(calls) == sc.PENDING_SAFE
    for name in sc.PENDING_SAFE:
        calls[name]()


def run_mul(eng, st, D, twice=False):
    from pvac_hfhe_cppbyv_amd import MUL_WITH_SIGMA
    A, Bb = dev(eng, st.inp["xs"]), dev(eng, st.inp["ys"])
    Cb, plan = eng.ct_mul_plan(A, Bb)
    if st.op == "mul_pending":
        between_plan_and_exec(eng, st, A, Bb, Cb, plan)
    nz = i64(eng, st.inp["nonces"])
    salts = i64(eng, st.inp["salts"]) if st.inp["sigma"] else None
    flags = MUL_WITH_SIGMA if st.inp["sigma"] else 0
    out = eng.ct_mul(A, Bb, nonces=nz, salts=salts, flags=flags, C_=Cb, plan=plan)
    got = {"out": host(out), "status": [int(s) for s in eng.ct_mul_status(A.n)], "n_small": plan.n_small,
           "n_large": plan.n_large, "layer_slots": plan.total_layer_slots, "edge_slots": plan.total_edge_slots}
    if twice:   # plan + exec again into the same buffers: the argument block is byte-identical
        plan2 = eng.ct_mul_into(A, Bb, out, nz, salts, flags)
        again = {"out": host(out), "status": [int(s) for s in eng.ct_mul_status(A.n)], "n_small": plan2.n_small,
                 "n_large": plan2.n_large, "layer_slots": plan2.total_layer_slots, "edge_slots": plan2.total_edge_slots}
        check(st, again, "second run")
    D[st.name] = {"A": A, "B": Bb, "C": out, "nonces": nz}
    return got


def run_check_gsum(eng, st, D):
    d = D[st.src]
    bad, status = eng.check_mul_gsum(d["A"], d["B"], d["C"], d["nonces"], status=True)
    return {"bad": bad, "status": [int(s) for s in status]}


def run_add(eng, st, D):
    sigma = st.inp["sigma"]
    A = D[st.src]["C"] if st.src else dev(eng, st.inp["xs"], sigma)
    out, plan = ct_add(eng, A, dev(eng, st.inp["ys"], sigma), st.inp["negate"], sigma)
    D[st.name] = {"C": out}
    return {"out": host(out), "n_large": plan.n_large, "max_layers": plan.max_layers}


def run_lincomb(eng, st, D):
    X = D[st.src]["C"] if st.src else dev(eng, st.inp["pool"])
    out = eng.ct_lincomb(X, st.inp["seg_off"], st.inp["term"], st.inp["scales"], st.inp["flags"])
    D[st.name] = {"C": out}
    return {"out": host(out), "status": [int(s) for s in eng.ct_lincomb_status(len(st.inp["seg_off"]) - 1)]}


def run_compact(eng, st, D):
    out = eng.compact(D[st.src]["C"] if st.src else dev(eng, st.inp["cs"], True))
    D[st.name] = {"C": out}
    return {"out": host(out)}


def run_recrypt(eng, st, D):
    out, iters = eng.ct_recrypt(dev(eng, st.inp["cs"], True), dev(eng, st.inp["pool"], True), st.inp["picks"])
    return {"out": host(out), "iters": [int(k) for k in iters]}


def run_commit_image(eng, st, D):
    sigma = st.inp["sigma"]
    X = D[st.src]["C"] if st.src else dev(eng, st.inp["cs"], sigma)
    commit = eng.commit_ct(X, with_sigma=sigma)
    image, pos = eng.ct_image(X, sc.M_BITS, return_pos=True)
    Y = eng.ct_from_image(image, pos, X.n, sc.M_BITS if sigma else 0, st.aux["layer_cap"], st.aux["edge_cap"], sigma=sigma)
    return {"commit": [row.tobytes() for row in commit], "image": image.cpu().numpy().tobytes(), "out": host(Y)}


def run_gather(eng, st, D):
    sel = eng.select(dev(eng, st.inp["x1"], True), st.inp["idx"])
    return {"out": host(eng.cat([sel, dev(eng, st.inp["x2"], True)]))}


def run_metrics(eng, st, D):
    cs = st.inp["cs"]
    X = dev(eng, cs, True)
    hist = eng.sigma_bytehist(X).cpu().numpy().view(np.uint64)
    g, status = eng.layer_gsum(X, status=True)
    g = g.cpu().numpy().view(np.uint64)
    off = sc.dense_off(cs)
    gsum = [[int(g[int(o) + l, 0]) | (int(g[int(o) + l, 1]) << 64) for l in range(c.nL)] for c, o in zip(cs, off)]
    return {"hist": hist, "gsum": gsum, "status": [int(s) for s in status]}


def run_dec(eng, st, D):
    X = D[st.src]["C"] if st.src else dev(eng, st.inp["cs"])
    vals, status = eng.dec_value(X, st.inp["R"])
    return {"values": vals, "status": [int(s) for s in status]}


def run_enc(eng, st, D):
    out, status = eng.enc_value(st.inp["vals"], st.inp["rnd"])
    return {"out": host(out), "status": [int(s) for s in status]}


def run_scale(eng, st, D):
    X = clone(D[st.src]["C"]) if st.src else dev(eng, st.inp["cs"])
    return {"out": host(eng.ct_neg(X) if st.inp["neg"] else eng.ct_scale(X, st.inp["s"]))}


def run_chain(eng, st, D):
    n = len(st.inp["xs"])
    r = eng.ct_mul_chain(dev(eng, st.inp["xs"]), st.inp["depth"], nonce_seed=st.inp["seed"], streams=1, chunk=n,
                         digest_n=n, sumdigest=True)
    return {"counts": [int(v) for v in r["counts"]], "sumdigests": [int(v) for v in r["sumdigests"]],
            "edges": [int(v) for v in r["edges"]], "pair_steps": int(r["pair_steps"])}


def run_ref_stale(eng, st, D):
    xs, ys = st.inp["pairs"]
    A, Bb = dev(eng, xs), dev(eng, ys)
    C1, plan1 = eng.ct_mul_plan(A, Bb)
    eng.ct_mul_plan(A, Bb)
    nz = eng.torch.zeros(2 * plan1.total_layer_slots, dtype=eng.torch.int64, device=eng.device)
    refused(eng, st, lambda: eng.ct_mul(A, Bb, nonces=nz, C_=C1, plan=plan1))
    return {}


def run_ref_sizes(eng, st, D):
    xs, ys = st.inp["pairs"]
    A, B1 = dev(eng, xs), dev(eng, ys[:1])
    refused(eng, st, lambda: eng.ct_add(A, B1))
    refused(eng, st, lambda: eng.ct_mul_plan(A, B1))
    return {}


def run_ref_layer_limit(eng, st, D):
    assert eng.layer_limit == sc.LIMIT_DEFAULT
    A, Bb = dev(eng, st.inp["xs"], True), dev(eng, st.inp["ys"], True)
    refused(eng, st, lambda: eng.ct_add(A, Bb, sigma=True))
    return {}


def run_ref_lincomb_status(eng, st, D):
    eng.ct_sum(dev(eng, st.inp["pool"]), [0, 1, 2])
    refused(eng, st, lambda: eng.ct_lincomb_status(3))
    assert list(eng.ct_lincomb_status(2)) == [0, 0]
    return {}


def run_ref_mul_status(eng, st, D):
    xs, ys = st.inp["pairs"]
    eng.ct_mul(dev(eng, xs), dev(eng, ys), nonces=i64(eng, st.inp["nonces"]))
    refused(eng, st, lambda: eng.ct_mul_status(3))
    assert list(eng.ct_mul_status(2)) == [0, 0]
    return {}


RUN = {"mul": run_mul, "mul_pending": run_mul, "check_gsum": run_check_gsum, "add": run_add, "lincomb": run_lincomb,
       "compact": run_compact, "recrypt": run_recrypt, "commit_image": run_commit_image, "gather": run_gather,
       "metrics": run_metrics, "dec": run_dec, "enc": run_enc, "scale": run_scale, "chain": run_chain,
       "ref_stale": run_ref_stale, "ref_sizes": run_ref_sizes, "ref_layer_limit": run_ref_layer_limit,
       "ref_lincomb_status": run_ref_lincomb_status, "ref_mul_status": run_ref_mul_status}


# ------------------------------------------------------------------------------------ comparing
def check(st, got, what=""):
    assert got.keys() == st.want.keys(), (st.name, what)
    for key, want in st.want.items():
        if key == "out":
            assert len(got[key]) == len(want), (st.name, what)
            for i, (g, w) in enumerate(zip(got[key], want)):
                assert sc.same_value(g, w), (st.name, what, "cipher", i, (g.nL, g.nE), (w.nL, w.nE))
        else:
            assert sc.same_value(got[key], want), (st.name, what, key, got[key] if key != "image" else len(got[key]), want
                                                   if key != "image" else len(want))


def run_step(eng, st, D, twice=False):
    """One step on the context as it is: its layer limit, the call(s), every value and the counters' delta."""
    eng.set_layer_limit(st.limit)
    before = counters(eng)
    if st.op == "mul":
        got = run_mul(eng, st, D, twice)
    else:
        got = RUN[st.op](eng, st, D)
        if twice:
            check(st, RUN[st.op](eng, st, D), "second run")
    after = counters(eng)
    check(st, got)
    moved = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    assert moved == {k: v * (2 if twice else 1) for k, v in st.route.items() if v}, (st.name, moved)


def with_producers(by, name):
    return (with_producers(by, by[name].src) if by[name].src else []) + [name]


# ------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("pset,name", [(p, n) for p in ("main", "wide") for n in sc.STEP_NAMES[p]],
                         ids=[n for p in ("main", "wide") for n in sc.STEP_NAMES[p]])
def test_step_alone(table, key_material, pset, name):
    """The step on a fresh context (after its producers, which have their own case): the kernel at that shape."""
    by = {s.name: s for s in table[pset]}
    eng, D = make_engine(pset, key_material), {}
    for n in with_producers(by, name):
        run_step(eng, by[n], D)


@pytest.mark.parametrize("order", sc.ORDERS)
def test_sequence(table, key_material, order):
    """The whole table on one context per parameter set, every step compared in full. In "reverse" every step
    runs twice in a row: a ct_mul is planned and exec'd again into the same output buffers (the argument
    block's reuse), every other step is simply run again into new ones. In "shuffle1" timing is switched on
    halfway and reset once."""
    for pset in ("main", "wide"):
        steps = table[pset]
        by = {s.name: s for s in steps}
        names = sc.order_of(steps, order)
        eng, D = make_engine(pset, key_material), {}
        for i, n in enumerate(names):
            if order == "shuffle1" and i == len(names) // 2:
                eng.timing(True)
            if order == "shuffle1" and i == 3 * len(names) // 4:
                eng.timing_reset()
            run_step(eng, by[n], D, twice=order == "reverse")
        eng.sync()


def test_regression_mul_status_after_scratch_growth(table, key_material):
    """Reduced order mul_over, add_many, ct_mul_status. The statuses of the last ct_mul_exec live in the
    per-pair plan scratch; a plan of 1,025 pairs regrows it (its floor is 1,024 pairs), and ct_mul_status
    went on copying 3 words out of the new, unwritten array because the host's count of the last exec's
    pairs still said 3. It now refuses until the next exec."""
    from pvac_hfhe_cppbyv_amd import PvacError
    by = {s.name: s for s in table["main"]}
    eng, D = make_engine("main", key_material), {}
    run_step(eng, by["mul_over"], D)
    assert list(eng.ct_mul_status(3)) == [1, 1, 1]
    run_step(eng, by["add32"], D)                      # a plan inside the scratch leaves them in place
    assert list(eng.ct_mul_status(3)) == [1, 1, 1]
    run_step(eng, by["add_many"], D)
    with pytest.raises(PvacError, match="more pairs than the last ct_mul_exec held"):
        eng.ct_mul_status(3)
    run_step(eng, by["mul_cancel"], D)                 # the next exec's statuses are served again
    assert list(eng.ct_mul_status(4)) == [0, 0, 0, 0]
