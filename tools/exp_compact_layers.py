"""A/B timing of the kernels that run compact_layers (csrc/compact_layers.hpp) against the parent commit's
library, in one process on one GPU (GPU box). Build the parent's library from a worktree of it with its own
Makefile and place it at pvac_hfhe_cppbyv_amd/lib/exp/libpvac_hip_parent.so; --lib names another.

Shapes: ct_add / ct_sub on 2^20 fresh pairs (k_ct_add_wave); ct_add of two depth-8 chain results
(k_ct_add); the depth-13-sized self-add of tools/measure_deep.py (k_ct_add_deep); tools/exp_lincomb.py's
three shapes and one with workgroup-route terms (k_lincomb_plan, k_lincomb_plan_wg); Engine.compact on
4,096 fresh products with sigma (k_compact_small); one over-budget ct_add pair (k_merge_layers); a
4,096-input depth-8 chain (k_large_layers). Device time from each engine's HIP-event timers, summed over
the stages named per shape (the chain: wall time of the synchronous call). One warm-up of both libraries,
whose outputs are compared, then the two alternate; medians of --reps passes. The gate of a shape: the new
median exceeds the parent's by no more than the parent's own max - min over its passes.
Prints one JSON line; --out also writes it to a file.
Usage: python tools/exp_compact_layers.py [--reps 7] [--scale 1.0] [--out profiles/compact_layers/ab.json]"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from measure_deep import cipher  # noqa: E402
from pvac_hfhe_cppbyv_amd import DeviceBatch, Engine, _LIB_PATH, load_library  # noqa: E402

PARENT = os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "lib", "exp", "libpvac_hip_parent.so")
TAG = 0x5EED0005


def same(eng, a, b, sigma=False):
    """The used rows of two outputs, packed, are equal."""
    if not (torch.equal(a.l_cnt[:a.n], b.l_cnt[:b.n]) and torch.equal(a.e_cnt[:a.n], b.e_cnt[:b.n])):
        return False
    a, b = eng.pack(a), eng.pack(b)
    nl, ne = int(a.l_cnt[:a.n].sum().item()), int(a.e_cnt[:a.n].sum().item())
    ok = torch.equal(a.layers[:nl], b.layers[:nl])
    for f in ("meta", "w_lo", "w_hi") + (("sigma",) if sigma else ()):
        ok = ok and torch.equal(getattr(a, f)[:ne], getattr(b, f)[:ne])
    return bool(ok)


def ab(name, engines, names, fn, reps, sigma=False, wall=False, fresh=False):
    """fn(engine) -> output batch (or digests), on the new and the parent library in turn. fresh: `engines`
    holds factories, and every pass builds its engine, warms it up with one call and drops it
    (ct_mul_chain's workers size their scratch from the HBM that is free, so the two libraries' engines
    cannot hold theirs at once)."""
    get = lambda k: engines[k]() if fresh else engines[k]
    outs = {}
    for k in engines:   # warm-up
        e = get(k)
        outs[k] = fn(e)
        e.sync()
        del e
    if isinstance(outs["new"], DeviceBatch):
        equal = same(get("new"), outs["new"], outs["parent"], sigma)
    else:
        equal = bool(np.array_equal(outs["new"], outs["parent"]))
    del outs
    t = {"new": [], "parent": []}
    for _ in range(reps):
        for k in engines:
            e = get(k)
            if fresh:
                fn(e)
            e.sync()
            e.timing_reset()
            t0 = time.perf_counter()
            out = fn(e)
            e.sync()
            w = (time.perf_counter() - t0) * 1e3
            t[k].append(w if wall else sum(e.timing_get(nm)[0] for nm in names))
            del out, e
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = max(t["parent"]) - min(t["parent"])
    return {"shape": name, "timed": "wall" if wall else list(names), "outputs_equal": equal,
            "new_ms": [round(x, 4) for x in t["new"]], "parent_ms": [round(x, 4) for x in t["parent"]],
            "new_median_ms": round(med["new"], 4), "parent_median_ms": round(med["parent"], 4),
            "parent_spread_ms": round(spread, 4), "within_gate": bool(med["new"] <= med["parent"] + spread)}


def chain_results(eng, n, depth, seed):
    """c_depth of n fresh inputs by plain ct_mul calls, packed."""
    X = eng.gen_fresh(n, seed, 20)
    c = X
    for d in range(depth):
        c = eng.pack(eng.ct_mul(c, X, nonce_seed=seed + d))
    return c


def products(eng, n, sigma):
    P = eng.pack(eng.ct_mul(eng.gen_fresh(n, 11, 20), eng.gen_fresh(n, 12, 20)))
    if sigma:
        P.sigma = torch.empty((max(P.meta.shape[0], 1), 128), dtype=torch.int64, device=eng.device)
        eng.fill_random(P.sigma, 13)
    return P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink every batch (a quick run)")
    ap.add_argument("--lib", default=PARENT, help="the parent commit's library")
    ap.add_argument("--only", default=None, help="comma-separated shape names")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("exp_compact_layers: needs a GPU")
    if a.reps < 5:
        sys.exit("exp_compact_layers: at least 5 passes")
    libs = {"new": load_library(_LIB_PATH), "parent": load_library(a.lib)}

    def engines(**kw):
        es = {k: Engine(device=0, canon_tag=TAG, lib=lib, **kw) for k, lib in libs.items()}
        for e in es.values():
            e.timing(True)
        return es

    k = lambda x: max(int(x * a.scale) // 16 * 16, 32)
    E = engines()
    e0 = E["new"]   # builds the inputs; they are plain device arrays, read by both libraries
    sha = lambda p: hashlib.sha256(open(p, "rb").read()).hexdigest()
    res = {"reps": a.reps, "scale": a.scale, "library_sha256": sha(_LIB_PATH), "parent_library_sha256": sha(a.lib),
           "shapes": []}
    want = set(a.only.split(",")) if a.only else None

    sel = lambda *names: want is None or any(nm in want for nm in names)

    def run(name, *args, **kw):
        if sel(name):
            res["shapes"].append(ab(name, *args, **kw))
            print(json.dumps(res["shapes"][-1]), file=sys.stderr, flush=True)

    if sel("add_fresh_2p20", "sub_fresh_2p20"):   # the wave kernels
        n = k(1 << 20)
        A, B = e0.gen_fresh(n, 0x5EED0A01, 20), e0.gen_fresh(n, 0x5EED0A02, 20)
        run("add_fresh_2p20", E, ["ct_add"], lambda e: e.ct_add(A, B), a.reps)
        run("sub_fresh_2p20", E, ["ct_add"], lambda e: e.ct_add(A, B, negate=True), a.reps)
        del A, B
    if sel("add_depth8_chains"):   # two depth-8 chain results: k_ct_add
        C1, C2 = chain_results(e0, k(256), 8, 0x31), chain_results(e0, k(256), 8, 0x32)
        res["chain8_layers_max"] = int(C1.l_cnt.max().item())
        run("add_depth8_chains", E, ["ct_add"], lambda e: e.ct_add(C1, C2), a.reps)
        del C1, C2
    if sel("add_deep_self_65584"):   # k_ct_add_deep: 32,792 + 32,792 layers (a depth-13 product's count), four edges per layer
        D = engines(layer_limit=1 << 20)
        X = DeviceBatch.from_host([cipher(np.random.default_rng(13), 32792, 4, 337)], e0.device)
        run("add_deep_self_65584", D, ["ct_add_deep"], lambda e: e.ct_add(X, X), a.reps)
        del X, D

    # ct_lincomb: exp_lincomb.py's shapes, and workgroup-route terms (depth-4 chain results, > 64 layers)
    def lincomb(name, make, m, sigma=False):
        if not sel(name):
            return
        X = make()
        nn = X.n // m
        seg_off = torch.arange(0, nn * m + 1, m, dtype=torch.int64, device=e0.device)
        term = torch.arange(nn * m, dtype=torch.int64, device=e0.device)
        res[name + "_layers_max"] = int(X.l_cnt.max().item())
        run(name, E, ["ct_lincomb_plan", "ct_lincomb"], lambda e: e.ct_lincomb(X, seg_off, term, sigma=sigma), a.reps,
            sigma=sigma)

    lincomb("lincomb_fresh_x16", lambda: e0.gen_fresh(k(1 << 20), 21, 20), 16)
    lincomb("lincomb_products_x16", lambda: products(e0, k(1 << 16), False), 16)
    lincomb("lincomb_products_sigma_x16", lambda: products(e0, k(4096), True), 16, sigma=True)
    lincomb("lincomb_wg_terms_x16", lambda: chain_results(e0, k(2048), 4, 0x33), 16)
    res["lincomb_paths"] = {kk: e.ct_lincomb_path_counts() for kk, e in E.items()}
    if sel("compact_products_4096"):   # k_compact_small: fresh products with sigma
        P = products(e0, k(4096), True)
        run("compact_products_4096", E, ["compact"], lambda e: e.compact(P), a.reps, sigma=True)
        res["compact_paths"] = {kk: e.compact_path_counts() for kk, e in E.items()}
        del P
    if sel("add_over_budget_pair"):   # k_merge_layers: 1.5 M + 1.5 M edges on 3,000 + 3,000 layers
        rng = np.random.default_rng(14)
        ne = max(int(500 * a.scale), 1)
        MA = DeviceBatch.from_host([cipher(rng, 3000, ne, 337)], e0.device)
        MB = DeviceBatch.from_host([cipher(rng, 3000, ne, 337)], e0.device)
        M = engines(edge_budget=min(1200000, 3000 * ne))
        run("add_over_budget_pair", M, ["ct_add", "ct_add_merge"], lambda e: e.ct_add(MA, MB), a.reps)
        del MA, MB, M
    if sel("chain_4096_depth8"):   # k_large_layers at every step
        Xc = e0.gen_fresh(k(4096), 0x41, 20)
        e0.sync()
        E.clear()
        e0 = None
        torch.cuda.empty_cache()
        makers = {kk: (lambda lib=lib: Engine(device=0, canon_tag=TAG, lib=lib)) for kk, lib in libs.items()}
        run("chain_4096_depth8", makers, None,
            lambda e: e.ct_mul_chain(Xc, 8, nonce_seed=0x5EED0040, digest_n=Xc.n)["digests"], a.reps, wall=True, fresh=True)
    res["all_outputs_equal"] = all(s["outputs_equal"] for s in res["shapes"])
    res["all_within_gate"] = all(s["within_gate"] for s in res["shapes"])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
