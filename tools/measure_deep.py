#!/usr/bin/env python3
"""Device times of the deep kernels (k_large_deep.hip) next to the kernels they stand in for, on pairs just
below and just above each limit (GPU box). ct_mul at B = 337: two chain-shaped pairs, |B.L| = 2, 60 edges
per A layer, |A.L| = 5,460 (Lc = 16,382: k_large_lists / k_large_layers) and 5,462 (Lc = 16,388: the deep
kernels). ct_add: 29,998 layers (k_ct_add) against 30,002 (k_ct_add_deep), four edges per layer.
Times come from the engine's timing table (HIP events around each stage), the median of 5 runs after a
warm-up; each ct_mul pair runs at the default edge_budget (its 6.25 M output edges then take the canonical
order, status 1) and at a budget above them (the hash order, status 0); "wall_ms" is plan + exec with a synchronise, the same way.

    python3 tools/measure_deep.py --out profiles/deep/times.json
    rocprofv3 --kernel-trace --stats ... -- python3 tools/measure_deep.py --once      # per-kernel view
    python3 tools/measure_deep.py --merge-trace <kernel_stats.csv> --out profiles/deep/times.json
"""
import argparse
import csv
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYER_DT = np.dtype([("rule", "<u4"), ("pa", "<u4"), ("pb", "<u4"), ("pad", "<u4"),
                     ("ztag", "<u8"), ("nonce_lo", "<u8"), ("nonce_hi", "<u8")])


def cipher(rng, nl, per_layer, B):
    """nl BASE layers with per_layer distinct (idx, ch) cells each, shuffled."""
    from pvac_hfhe_cppbyv_amd import HostCipher
    L = np.zeros(nl, LAYER_DT)
    L["ztag"] = rng.integers(0, 2**63, nl, dtype=np.uint64)
    L["nonce_lo"] = rng.integers(0, 2**63, nl, dtype=np.uint64)
    cells = np.argsort(rng.random((nl, 2 * B)), axis=1)[:, :per_layer].astype(np.uint64)   # distinct per layer
    lay = np.repeat(np.arange(nl, dtype=np.uint64), per_layer)
    cells = cells.reshape(-1)
    order = rng.permutation(len(lay))
    lay, cells = lay[order], cells[order]
    meta = lay | ((cells >> np.uint64(1)) << np.uint64(32)) | ((cells & np.uint64(1)) << np.uint64(48))
    n = len(meta)
    return HostCipher(L, meta, rng.integers(0, 2**63, n, dtype=np.uint64), rng.integers(0, 2**62, n, dtype=np.uint64))


def med(xs):
    return round(statistics.median(xs), 4)


def run_mul(eng, la, reps):
    import torch
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    rng = np.random.default_rng(la)
    A = DeviceBatch.from_host([cipher(rng, la, 60, 337)], eng.device)
    Bb = DeviceBatch.from_host([cipher(rng, 2, 20, 337)], eng.device)
    names = ("ct_mul_large", "large_lists_deep", "large_layers_deep")
    rec = {k: [] for k in names}
    wall = []
    out = None
    for r in range(reps + 1):
        eng.timing_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = eng.ct_mul(A, Bb, nonce_seed=7)
        eng.sync()
        w = (time.perf_counter() - t0) * 1e3
        if r == 0:
            continue   # warm-up: the arena and the output arrays are allocated here
        wall.append(w)
        for k in names:
            rec[k].append(eng.timing_get(k)[0])
    return {"A_layers": la, "Lc": la + 2 + 2 * la, "A_edges": 60 * la, "B_edges": 40,
            "edge_budget": int(eng.params.edge_budget), "status": int(eng.ct_mul_status(1)[0]),
            "out_edges": int(out.e_cnt[0].item()), "out_layers": int(out.l_cnt[0].item()),
            "deep_pair": la + 2 + 2 * la > 16384 and eng.deep_path_counts()[0] > 0,
            "ms": {k: med(v) for k, v in rec.items()}, "wall_ms": med(wall)}


def run_add(eng, nl, reps):
    import torch
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    rng = np.random.default_rng(nl)
    A = DeviceBatch.from_host([cipher(rng, nl, 4, 337)], eng.device)
    Bb = DeviceBatch.from_host([cipher(rng, nl, 4, 337)], eng.device)
    names = ("ct_add", "ct_add_deep")
    rec = {k: [] for k in names}
    wall = []
    for r in range(reps + 1):
        eng.timing_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = eng.ct_add(A, Bb)
        eng.sync()
        w = (time.perf_counter() - t0) * 1e3
        if r == 0:
            continue
        wall.append(w)
        for k in names:
            rec[k].append(eng.timing_get(k)[0])
    return {"layers": 2 * nl, "edges": 8 * nl, "out_layers": int(out.l_cnt[0].item()),
            "ms": {k: med(v) for k, v in rec.items()}, "wall_ms": med(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true", help="one timed run per case (under a kernel trace)")
    ap.add_argument("--merge-trace", default=None, help="kernel_stats.csv of a --once run: added to --out")
    a = ap.parse_args()
    if a.merge_trace:
        res = json.load(open(a.out))
        rows = sorted(csv.DictReader(open(a.merge_trace)), key=lambda r: -float(r["TotalDurationNs"]))
        res["kernel_trace_once"] = {
            "note": "rocprofv3 --kernel-trace --stats over one --once run: all six cases, warm-up run included",
            "kernels": [{"name": r["Name"].replace("void ", "").replace("pvhip::(anonymous namespace)::", "")[:60],
                         "calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 4)}
                        for r in rows[:24]]}
        json.dump(res, open(a.out, "w"), indent=1)
        return
    from pvac_hfhe_cppbyv_amd import Engine, _LIB_PATH
    reps = 1 if a.once else 5
    eng = Engine(device=0, canon_tag=0xDEE9, layer_limit=1 << 20)
    eng.timing(True)
    # the products of these pairs (6.25 M edges) are over the default edge_budget: guard_budget's canonical
    # order (status 1). A second engine with the budget out of the way gives the reference's hash order
    big = Engine(device=0, canon_tag=0xDEE9, layer_limit=1 << 20, edge_budget=1 << 27)
    big.timing(True)
    res = {"library_sha256": hashlib.sha256(open(_LIB_PATH, "rb").read()).hexdigest(), "runs": reps,
           "ct_mul": [run_mul(e, la, reps) for e in (eng, big) for la in (5460, 5462)],
           "ct_add": [run_add(eng, nl, reps) for nl in (14999, 15001)]}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
