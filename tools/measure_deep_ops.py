#!/usr/bin/env python3
"""Device times of ct_sum, compact and ct_recrypt's sums on a cipher just below and just above 30,000 layers
(GPU box), on an engine whose layer limit was raised: the deep routes next to their nearest shallow
neighbours. B = 337, BASE layers, every layer with an edge (so every layer is kept).
  ct_sum    one term of 29,998 / 30,002 layers, four edges per layer: plan (k_lincomb_plan_wg against
            k_lincomb_split + k_lincomb_plan_deep, one more read-back) and exec.
  compact   one cipher of 29,998 / 30,002 layers, one edge per layer with a sigma row: both take the merge
            path; only the bound differs.
  recrypt   an input of 29,990 / 30,001 layers with all-zero sigma rows (eight iterations) and a pool of one
            1-layer cipher: eight sums of 29,991..29,998 layers (k_ct_add) against 30,002..30,009
            (k_ct_add_deep); the time of one sum is the timing table's total over its calls.
Times come from the engine's timing table (HIP events around each stage), the median of 5 runs after a
warm-up; "wall_ms" is the whole call with a synchronise.

    python3 tools/measure_deep_ops.py --out profiles/deep/ops_times.json
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from measure_deep import cipher, med  # noqa: E402


def with_sigma(c, zero=True, seed=1):
    from pvac_hfhe_cppbyv_amd import HostCipher
    n = len(c.meta)
    s = np.zeros((n, 128), np.uint64) if zero else np.random.default_rng(seed).integers(0, 2**63, (n, 128), dtype=np.uint64)
    return HostCipher(c.layers, c.meta, c.w_lo, c.w_hi, s)


def timed(eng, names, reps, call):
    """reps runs of call() after a warm-up: per name the median of (total ms / calls) and of the calls."""
    import torch
    rec = {k: [] for k in names}
    calls = {k: 0 for k in names}
    wall = []
    for r in range(reps + 1):
        eng.timing_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        eng.sync()
        w = (time.perf_counter() - t0) * 1e3
        if r == 0:
            continue
        wall.append(w)
        for k in names:
            ms, n = eng.timing_get(k)
            rec[k].append(ms / n if n else 0.0)
            calls[k] = int(n)
    return {"ms_per_call": {k: med(v) for k, v in rec.items()}, "calls": calls, "wall_ms": med(wall)}


def run_sum(eng, nl, reps):
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    X = DeviceBatch.from_host([cipher(np.random.default_rng(nl), nl, 4, 337)], eng.device)
    out = {}
    before = eng.deep_route_counts()[0]
    res = timed(eng, ("ct_lincomb_plan", "ct_lincomb"), reps, lambda: out.update(c=eng.ct_sum(X, [0, 1])))
    res.update(layers=nl, edges=4 * nl, out_layers=int(out["c"].l_cnt[0].item()),
               deep_terms=eng.deep_route_counts()[0] - before)
    return res


def run_compact(eng, nl, reps):
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    X = DeviceBatch.from_host([with_sigma(cipher(np.random.default_rng(nl), nl, 1, 337), zero=False)], eng.device, sigma=True)
    out = {}
    before = eng.deep_route_counts()[2]
    res = timed(eng, ("compact",), reps, lambda: out.update(c=eng.compact(X)))
    res.update(layers=nl, edges=nl, out_layers=int(out["c"].l_cnt[0].item()), deep_ciphers=eng.deep_route_counts()[2] - before)
    return res


def run_recrypt(eng, nl, reps):
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    rng = np.random.default_rng(nl)
    X = DeviceBatch.from_host([with_sigma(cipher(rng, nl, 1, 337))], eng.device, sigma=True)
    P = DeviceBatch.from_host([with_sigma(cipher(rng, 1, 3, 337))], eng.device, sigma=True)
    out = {}
    before = eng.deep_route_counts()[3]
    res = timed(eng, ("ct_add", "ct_add_deep", "ct_recrypt"), reps,
                lambda: out.update(r=eng.ct_recrypt(X, P, np.zeros(8, np.uint64))))
    res.update(layers=nl, edges=nl, sums=[nl + 1, nl + 8], iters=int(out["r"][1][0]),
               deep_sums=eng.deep_route_counts()[3] - before)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from pvac_hfhe_cppbyv_amd import Engine, _LIB_PATH
    reps = 5
    eng = Engine(device=0, canon_tag=0xDEEA, layer_limit=1 << 17)
    eng.timing(True)
    eng.set_ubk(np.arange(8192, dtype=np.int32)[::-1].copy())
    res = {"library_sha256": hashlib.sha256(open(_LIB_PATH, "rb").read()).hexdigest(), "runs": reps,
           "ct_sum": [run_sum(eng, nl, reps) for nl in (29998, 30002)],
           "compact": [run_compact(eng, nl, reps) for nl in (29998, 30002)],
           "ct_recrypt": [run_recrypt(eng, nl, reps) for nl in (29990, 30001)]}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
