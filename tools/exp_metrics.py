"""Timing record of the metrics kernels (k_metrics.hip) against the existing kernels that read the same
bytes once: pvac_hip_sigma_bytehist against pvac_hip_sigma_popcount (HBM-bound), pvac_hip_layer_gsum
against pvac_hip_batch_sumdigest. Same device batch, same process; per launch the kernel's own device
time (pvac_hip_timing_get; sumdigest has no label and is timed with HIP events on the same stream),
median of `reps` launches after `warm` warm-ups.

Histogram shapes at m_bits 8192 (1 KiB rows), random (fill_random) and all-zero contents:
  a  2^16 ciphers x 40 rows      b  256 ciphers x 10,240 rows      c  one cipher of 2^21 rows
Gsum shapes: gen_fresh(2^20), and a chunk of depth-8 chains of fresh ciphers (ct_mul of the running
product with its input, 8 times).

Usage: python tools/exp_metrics.py [--reps 20] [--warm 3] [--chains 64] [--out profiles/metrics/metrics.json]"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lib_sha256():
    with open(os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "lib", "libpvac_hip.so"), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def timed(eng, label, call, reps, warm):
    """Median device milliseconds of `call` under the library's timing label."""
    for _ in range(warm):
        call()
    ms = []
    for _ in range(reps):
        t0, k0 = eng.timing_get(label)
        call()
        t1, k1 = eng.timing_get(label)   # synchronises
        assert k1 == k0 + 1, (label, k0, k1)
        ms.append(t1 - t0)
    return statistics.median(ms), min(ms)


def timed_events(eng, call, reps, warm):
    import torch
    for _ in range(warm):
        call()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--fresh-log2", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pvac_hfhe_cppbyv_amd import DeviceBatch, Engine, powg_table

    eng = Engine(device=0)
    eng.set_powg(powg_table())
    eng.timing(True)
    res = {"library_sha256": lib_sha256(), "device": torch.cuda.get_device_name(0), "reps": args.reps, "warm": args.warm,
           "sigma_bytehist": {}, "layer_gsum": {}}

    rows_total = (1 << 16) * 40
    sigma = torch.empty((rows_total, 128), dtype=torch.int64, device=eng.device)
    shapes = {"a_65536x40": (1 << 16, 40), "b_256x10240": (256, 10240), "c_1x2097152": (1, 1 << 21)}
    z = lambda n: torch.zeros(n, dtype=torch.int64, device=eng.device)
    for content in ("random", "zero"):
        if content == "random":
            eng.fill_random(sigma, 7)
        else:
            sigma.zero_()
        for name, (n, rows) in shapes.items():
            cnt = torch.full((n,), rows, dtype=torch.int64, device=eng.device)
            off = torch.arange(n, dtype=torch.int64, device=eng.device) * rows
            X = DeviceBatch(n, z(n), z(n), z(5).view(1, 5), off, cnt, z(1), z(1), z(1), sigma)
            h_ms, h_min = timed(eng, "sigma_bytehist", lambda: eng.sigma_bytehist(X), args.reps, args.warm)
            p_ms, p_min = timed(eng, "sigma_popcount", lambda: eng.sigma_popcount(X), args.reps, args.warm)
            hist = eng.sigma_bytehist(X).cpu().numpy().view(np.uint64)
            ones = eng.sigma_popcount(X).cpu().numpy().view(np.uint64)
            pop8 = np.array([bin(b).count("1") for b in range(256)], np.uint64)
            assert np.array_equal((hist * pop8).sum(axis=1), ones) and np.all(hist.sum(axis=1) == 1024 * rows)
            gb = n * rows * 1024 / 1e9
            res["sigma_bytehist"][f"{name}_{content}"] = {
                "ciphers": n, "rows": rows, "GB": round(gb, 3), "bytehist_ms": round(h_ms, 4), "bytehist_min_ms": round(h_min, 4),
                "popcount_ms": round(p_ms, 4), "popcount_min_ms": round(p_min, 4), "ratio": round(h_ms / p_ms, 3),
                "bytehist_TB_per_s": round(gb / h_ms, 3), "popcount_TB_per_s": round(gb / p_ms, 3)}
            print(name, content, json.dumps(res["sigma_bytehist"][f"{name}_{content}"]), file=sys.stderr, flush=True)
    del sigma

    def gsum_case(name, X):
        edges = int(X.e_cnt[:X.n].sum().item())
        layers = int(X.l_cnt[:X.n].sum().item())
        before = eng.metrics_path_counts()
        g_ms, g_min = timed(eng, "layer_gsum", lambda: eng.layer_gsum(X), args.reps, args.warm)
        after = eng.metrics_path_counts()
        s_ms, s_min = timed_events(eng, lambda: eng.sumdigest(X), args.reps, args.warm)
        calls = args.reps + args.warm
        res["layer_gsum"][name] = {
            "ciphers": X.n, "edges": edges, "layers": layers, "layer_gsum_ms": round(g_ms, 4), "layer_gsum_min_ms": round(g_min, 4),
            "sumdigest_ms": round(s_ms, 4), "sumdigest_min_ms": round(s_min, 4), "ratio": round(g_ms / s_ms, 3),
            "edges_per_s": round(edges / g_ms * 1e3, 1),
            "routes_per_call": {k: (after[k] - before[k]) // calls for k in ("gsum_wave", "gsum_workgroup", "gsum_large")}}
        print(name, json.dumps(res["layer_gsum"][name]), file=sys.stderr, flush=True)

    gsum_case(f"gen_fresh_2^{args.fresh_log2}", eng.gen_fresh(1 << args.fresh_log2, 11, 20))
    x = eng.gen_fresh(args.chains, 12, 20)
    c = x
    for k in range(8):
        c = eng.ct_mul(c, x, nonce_seed=0x5EED0100 + k)
    gsum_case(f"depth8_chain_chunk_{args.chains}", c)

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
