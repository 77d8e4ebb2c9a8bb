"""Timing of ct_lincomb (GPU box) against the routes that existed before it, in one process:
  (a) the same result by the existing entry points: m successive pvac_hip_ct_add_plan / _exec calls over
      strided views of the pool, from an empty accumulator (the reference's literal fold, batched);
  (b) for two-term segments, one pvac_hip_ct_add over the two views;
  (c) the device copy rate, against the algorithmic bytes: 24 B per edge and 40 B per layer read and
      written, the edge header (8 B) read once more by the plan pass, 1 KiB per edge each way with sigma.
Shapes: 2^16 outputs x 16 fresh ciphers; 2^12 outputs x 16 fresh x fresh products; 256 outputs x 16 of
4,096 products with sigma; 2^20 two-term segments of fresh ciphers. Device time from the engine's
HIP-event timers (ct_lincomb_plan + ct_lincomb against ct_add + ct_add_merge; ct_add's plan kernels
carry no timer, which favours the yardstick), wall time around the calls beside it. One warm-up, then
the routes alternate; medians with min / max. The two routes' outputs are compared after the warm-up.
Prints one JSON line; --out also writes it to a file.
Usage: python tools/exp_lincomb.py [--reps 5] [--scale 1.0] [--out profiles/lincomb/exp_lincomb.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pvac_hfhe_cppbyv_amd import DeviceBatch, Engine  # noqa: E402

COPY_RATE = 6.29e12   # measured device copy rate, bytes/s


def fresh(eng, n):
    return eng.gen_fresh(n, 21, 20)


def products(eng, n, sigma):
    A, B = eng.gen_fresh(n, 11, 20), eng.gen_fresh(n, 12, 20)
    P = eng.pack(eng.ct_mul(A, B))
    if sigma:
        P.sigma = torch.empty((max(P.meta.shape[0], 1), 128), dtype=torch.int64, device=eng.device)
        eng.fill_random(P.sigma, 13)
    return P


def views(X, m):
    """m batches of X.n / m ciphers: view j holds ciphers j, j + m, ... (term j of every output)."""
    n = X.n // m
    c = lambda t, j: t[j:X.n:m].contiguous()
    return [DeviceBatch(n, c(X.l_off, j), c(X.l_cnt, j), X.layers, c(X.e_off, j), c(X.e_cnt, j), X.meta, X.w_lo,
                        X.w_hi, X.sigma) for j in range(m)]


def timed(eng, names, fn):
    """(device ms summed over the timer names, wall ms) of one call of fn."""
    eng.sync()
    eng.timing_reset()
    t0 = time.perf_counter()
    out = fn()
    eng.sync()
    wall = (time.perf_counter() - t0) * 1e3
    return sum(eng.timing_get(k)[0] for k in names), wall, out


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def same_rows(a, b, sigma):
    if not (torch.equal(a.l_cnt[:a.n], b.l_cnt[:b.n]) and torch.equal(a.e_cnt[:a.n], b.e_cnt[:b.n]) and
            torch.equal(a.l_off[:a.n], b.l_off[:b.n]) and torch.equal(a.e_off[:a.n], b.e_off[:b.n])):
        return False
    ne, nl = int(a.e_cnt[:a.n].sum().item()), int(a.l_cnt[:a.n].sum().item())
    # both are dense here (every layer of these inputs is used), so the used rows are the leading ones
    ok = torch.equal(a.layers[:nl], b.layers[:nl])
    for f in ("meta", "w_lo", "w_hi"):
        ok = ok and torch.equal(getattr(a, f)[:ne], getattr(b, f)[:ne])
    if sigma:
        ok = ok and torch.equal(a.sigma[:ne], b.sigma[:ne])
    return bool(ok)


def shape(eng, name, X, m, sigma, reps, with_ct_add=False):
    n = X.n // m
    seg_off = torch.arange(0, n * m + 1, m, dtype=torch.int64, device=eng.device)
    term = torch.arange(n * m, dtype=torch.int64, device=eng.device)
    V = views(X, m)
    empty = DeviceBatch.empty(n, 0, 0, eng.device, sigma=sigma)
    edges, layers = int(X.e_cnt[:n * m].sum().item()), int(X.l_cnt[:n * m].sum().item())
    nbytes = edges * (24 + 8 + 24) + layers * 80 + (edges * 2048 if sigma else 0)

    def lincomb():
        return eng.ct_lincomb(X, seg_off, term, sigma=sigma)

    def fold():
        acc = empty
        for j in range(m):
            acc = eng.ct_add(acc, V[j], sigma=sigma)
        return acc

    def pair():
        return eng.ct_add(V[0], V[1], sigma=sigma)

    a, b = lincomb(), fold()   # warm-up, and the outputs agree
    eng.sync()
    res = {"shape": name, "outputs": n, "terms_per_output": m, "edges": edges, "layers": layers, "sigma": sigma,
           "algorithmic_bytes": nbytes, "outputs_equal_fold": same_rows(a, b, sigma)}
    if with_ct_add:
        res["outputs_equal_ct_add"] = same_rows(a, pair(), sigma)
    del a, b
    t = {"lincomb": [], "lincomb_plan": [], "lincomb_wall": [], "fold": [], "fold_wall": [], "ct_add": [], "ct_add_wall": []}
    for _ in range(reps):   # the routes alternate
        eng.sync()
        eng.timing_reset()
        t0 = time.perf_counter()
        out = lincomb()
        eng.sync()
        t["lincomb_wall"].append((time.perf_counter() - t0) * 1e3)
        t["lincomb_plan"].append(eng.timing_get("ct_lincomb_plan")[0])
        t["lincomb"].append(eng.timing_get("ct_lincomb_plan")[0] + eng.timing_get("ct_lincomb")[0])
        del out
        d, w, out = timed(eng, ["ct_add", "ct_add_merge"], fold)
        t["fold"].append(d)
        t["fold_wall"].append(w)
        del out
        if with_ct_add:
            d, w, out = timed(eng, ["ct_add", "ct_add_merge"], pair)
            t["ct_add"].append(d)
            t["ct_add_wall"].append(w)
            del out
    res["ms"] = {k: stats(v) for k, v in t.items() if v}
    best = statistics.median(t["lincomb"])
    res["TB_per_s"] = round(nbytes / (best * 1e-3) / 1e12, 3)
    res["of_copy_rate"] = round(nbytes / (best * 1e-3) / COPY_RATE, 3)
    res["fold_over_lincomb"] = round(statistics.median(t["fold"]) / best, 2)
    res["fold_over_lincomb_wall"] = round(statistics.median(t["fold_wall"]) / statistics.median(t["lincomb_wall"]), 2)
    res["expected_by_bytes"] = round((m + 1) / 2.33, 2)
    if with_ct_add:
        res["lincomb_over_ct_add"] = round(best / statistics.median(t["ct_add"]), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink every shape (a quick run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("exp_lincomb: needs a GPU")
    eng = Engine(device=0, canon_tag=0x5EED0004)
    eng.timing(True)
    k = lambda x: max(int(x * a.scale) // 16 * 16, 32)
    res = {"copy_rate_TB_per_s": COPY_RATE / 1e12, "reps": a.reps, "shapes": []}
    res["shapes"].append(shape(eng, "fresh_x16", fresh(eng, k(1 << 20)), 16, False, a.reps))
    res["shapes"].append(shape(eng, "products_x16", products(eng, k(1 << 16), False), 16, False, a.reps))
    res["shapes"].append(shape(eng, "products_sigma_x16", products(eng, k(4096), True), 16, True, a.reps))
    res["shapes"].append(shape(eng, "fresh_pairs", fresh(eng, k(1 << 21)), 2, False, a.reps, with_ct_add=True))
    res["paths"] = eng.ct_lincomb_path_counts()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
