"""Timing of ct_recrypt's parts (GPU box): sigma_popcount, ubk_apply and the batched compact on a
batch of fresh x fresh products with sigma (4,096 products: about 5 GB of sigma rows), and compact
against the only route there was before it: ct_add(X, empty) on a context whose edge_budget is 0
(k_add_merge.hip, one cipher at a time). Device time from the engine's HIP-event timers
(pvac_hip_timing_get); bytes are the algorithmic ones: 1 KiB read per edge for the popcount, 2 KiB per
edge for ubk_apply, 2 KiB + 48 B per edge for compact. The two compact routes alternate and their
outputs are compared. Prints one JSON line; --out also writes it to a file.
Usage: python tools/exp_recrypt.py [--n 4096] [--reps 5] [--old-reps 2] [--out profiles/recrypt/exp.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pvac_hfhe_cppbyv_amd import DeviceBatch, Engine  # noqa: E402

COPY_RATE = 6.29e12   # measured device copy rate, bytes/s


def products(eng, n):
    """n fresh x fresh products, packed, with uniformly random sigma rows (density 0.5: in range)."""
    A, B = eng.gen_fresh(n, 11, 20), eng.gen_fresh(n, 12, 20)
    P = eng.pack(eng.ct_mul(A, B))
    P.sigma = torch.empty((max(P.meta.shape[0], 1), 128), dtype=torch.int64, device=eng.device)
    eng.fill_random(P.sigma, 13)
    return P


def timed(eng, names, fn, reps):
    """Device ms per call of fn (sum over the timer names), every repetition's value."""
    out = []
    for _ in range(reps):
        eng.timing_reset()
        fn()
        eng.sync()
        out.append(sum(eng.timing_get(k)[0] for k in names))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--old-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("exp_recrypt: needs a GPU")
    eng = Engine(device=0, canon_tag=0x5EED0003)
    old = Engine(device=0, canon_tag=0x5EED0003, edge_budget=0)
    eng.set_ubk(np.random.default_rng(7).permutation(8192).astype(np.int32))
    X = products(eng, a.n)
    edges = int(X.e_cnt.sum().item())
    empty = DeviceBatch.empty(a.n, 0, 0, eng.device, sigma=True)
    eng.timing(True)
    old.timing(True)
    keep = {}

    def new_compact():
        keep["new"] = eng.compact(X)

    def old_compact():
        keep["old"] = old.ct_add(X, empty, sigma=True)

    # warm-up: every kernel once at the timed shapes
    eng.sigma_popcount(X)
    new_compact()
    old_compact()
    eng.sync()
    same = None
    n_, o_ = keep["new"], keep["old"]
    if torch.equal(n_.e_cnt, o_.e_cnt) and torch.equal(n_.l_cnt, o_.l_cnt) and torch.equal(n_.e_cnt, X.e_cnt):
        same = bool(torch.equal(n_.meta[:edges], o_.meta[:edges]) and torch.equal(n_.w_lo[:edges], o_.w_lo[:edges]) and
                    torch.equal(n_.w_hi[:edges], o_.w_hi[:edges]) and torch.equal(n_.sigma[:edges], o_.sigma[:edges]))
    res = {"n": a.n, "edges": edges, "sigma_bytes": edges * 1024, "compact_outputs_equal": same,
           "paths": eng.compact_path_counts()}
    t_new, t_old = [], []
    for r in range(max(a.reps, a.old_reps)):   # the two routes alternate
        if r < a.reps:
            t_new += timed(eng, ["compact"], new_compact, 1)
        if r < a.old_reps:
            t_old += timed(old, ["ct_add", "ct_add_merge"], old_compact, 1)
    keep.clear()
    t_pop = timed(eng, ["sigma_popcount"], lambda: eng.sigma_popcount(X), a.reps)
    eng.ubk_apply(X)   # warm-up; the rows stay uniformly random under a bit permutation
    t_ubk = timed(eng, ["ubk_apply"], lambda: eng.ubk_apply(X), a.reps)

    def row(ms, bytes_per_edge):
        best = min(ms)
        return {"ms": [round(x, 4) for x in ms], "best_ms": round(best, 4), "bytes": edges * bytes_per_edge,
                "TB_per_s": round(edges * bytes_per_edge / (best * 1e-3) / 1e12, 3),
                "of_copy_rate": round(edges * bytes_per_edge / (best * 1e-3) / COPY_RATE, 3)}

    res["sigma_popcount"] = row(t_pop, 1024)
    res["ubk_apply"] = row(t_ubk, 2048)
    res["compact"] = row(t_new, 2048 + 48)
    res["compact_via_ct_add_budget0"] = row(t_old, 2048 + 48)
    res["compact_speedup"] = round(min(t_old) / min(t_new), 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
