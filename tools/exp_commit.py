"""Timing of the batched commit_ct (GPU box): k_commit_ct on
  (a) the fresh x fresh products with sigma that tools/exp_recrypt.py uses (4,096 products, about 5 GB
      of sigma rows, one SHA-256 chain of about 20 K blocks per product),
  (b) 2^16 weights-only fresh products from gen_fresh + ct_mul (capacity-padded output, in place),
  and a ragged mix: (a)'s products interleaved with 40-edge fresh ciphers.
Device time from the engine's HIP-event timer (pvac_hip_timing_get "commit_ct"). Blocks are 64-byte
SHA-256 blocks, padding included. The VALU floor is blocks x SHA_VALU_PER_BLOCK / (64 x
pvac_hip_alu_ceiling(4)), the ceiling (wave64 instructions per second) measured in this process and
every wave instruction advancing 64 ciphers by one step: a batch that cannot fill the lanes of every
SIMD stays far under it, and chain_us_per_block (kernel time over the longest cipher's blocks) says
how fast one lane's chain went. The comparison is the only route there was before: to_host() and the CPU
oracle's commit_ct per cipher on one core, timed here on the same box (--host-n limits it to the
first ciphers of each batch and scales linearly; the record says so). Digests of both routes are
compared. Prints one JSON line; --out also writes it to a file.
Usage: python tools/exp_commit.py [--n 4096] [--nw 65536] [--reps 3] [--host-n 0] [--lib lib/exp/libpvac_hip_try.so] [--out profiles/commit/exp_commit.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from helpers import Cipher, Oracle  # noqa: E402
from pvac_hfhe_cppbyv_amd import DeviceBatch, Engine, load_library  # noqa: E402

SHA_VALU_PER_BLOCK = 1370   # sha_compress compiled for gfx950 (csrc/sha256.hpp), VALU instructions
CANON = 0x5EED0003
HD = bytes(range(32))


def products(eng, n):
    """exp_recrypt.py's batch: n fresh x fresh products, packed, with uniformly random sigma rows."""
    A, B = eng.gen_fresh(n, 11, 20), eng.gen_fresh(n, 12, 20)
    P = eng.pack(eng.ct_mul(A, B))
    P.sigma = torch.empty((max(P.meta.shape[0], 1), 128), dtype=torch.int64, device=eng.device)
    eng.fill_random(P.sigma, 13)
    return P


def message_bytes(X, sigma_bytes):
    """Per-cipher message length: 55 + 25 per BASE layer + 17 per other layer + (33 + sigma_bytes) per edge."""
    u = lambda t: t.cpu().numpy().view(np.uint64).astype(np.int64)
    lo, lc, ec = u(X.l_off)[:X.n], u(X.l_cnt)[:X.n], u(X.e_cnt)[:X.n]
    rule = X.layers[:, 0].cpu().numpy().view(np.uint64) & np.uint64(0xFFFFFFFF)
    per = np.where(rule == 0, 25, 17).astype(np.int64)
    cs = np.concatenate([[0], np.cumsum(per)])
    return 55 + (cs[lo + lc] - cs[lo]) + ec * (33 + sigma_bytes)


def timed(eng, fn, reps):
    out = []
    for _ in range(reps):
        eng.timing_reset()
        fn()
        eng.sync()
        out.append(eng.timing_get("commit_ct")[0])
    return out


def host_route(orc, X, k, with_sigma):
    """to_host() of the whole batch, then the oracle's commit_ct of the first k ciphers on one core."""
    t0 = time.perf_counter()
    hs = X.to_host()
    t1 = time.perf_counter()
    out = []
    for i, c in enumerate(hs[:k]):
        out.append(orc.commit(Cipher(c.layers, c.meta, c.w_lo, c.w_hi, c.sigma if with_sigma else None), CANON, HD))
        if i % 512 == 511:
            print(f"  host route: {i + 1} / {k} ciphers, {time.perf_counter() - t1:.1f} s", file=sys.stderr, flush=True)
    t2 = time.perf_counter()
    return out, t1 - t0, t2 - t1


def measure(eng, orc, X, with_sigma, reps, host_n, ceiling):
    sigma_bytes = 1024 if with_sigma else 0
    keep = {}

    def run():
        keep["d"] = eng.commit_ct(X, with_sigma=with_sigma)

    run()   # warm-up at the timed shape
    ms = timed(eng, run, reps)
    lens = message_bytes(X, sigma_bytes)
    blocks = int(((lens + 9 + 63) // 64).sum())
    best = min(ms) * 1e-3
    floor_s = blocks * SHA_VALU_PER_BLOCK / (64 * ceiling)
    longest = int(((lens + 9 + 63) // 64).max())
    res = {"n": X.n, "edges": int(X.e_cnt[:X.n].sum().item()), "message_bytes": int(lens.sum()), "blocks": blocks,
           "longest_cipher_blocks": longest, "chain_us_per_block": round(best * 1e6 / longest, 3),
           "ms": [round(x, 3) for x in ms], "best_ms": round(best * 1e3, 3),
           "blocks_per_s": round(blocks / best, 1), "message_GB_per_s": round(int(lens.sum()) / best / 1e9, 3),
           "valu_floor_ms": round(floor_s * 1e3, 3), "fraction_of_valu_floor": round(floor_s / best, 4)}
    if host_n is not None:
        k = X.n if host_n <= 0 else min(host_n, X.n)
        digs, t_copy, t_hash = host_route(orc, X, k, with_sigma)
        res["digests_equal_host_route"] = bool(all(bytes(keep["d"][i]) == digs[i] for i in range(k)))
        t_hash_all = t_hash * (X.n / k)
        res["host_route"] = {"ciphers_hashed": k, "to_host_s": round(t_copy, 3), "oracle_commit_s": round(t_hash, 3),
                             "oracle_commit_s_scaled_to_n": round(t_hash_all, 3),
                             "total_s": round(t_copy + t_hash_all, 3)}
        res["host_over_gpu"] = round((t_copy + t_hash_all) / best, 1)
    return res


def interleave(P, F):
    """P's and F's ciphers alternating (P0, F0, P1, F1, ...) over the concatenated row arrays."""
    nl, ne = P.layers.shape[0], P.meta.shape[0]
    il = lambda a, b: torch.stack([a[:P.n], b[:F.n]], 1).reshape(-1).contiguous()
    return DeviceBatch(P.n + F.n, il(P.l_off, F.l_off + nl), il(P.l_cnt, F.l_cnt), torch.cat([P.layers, F.layers]),
                       il(P.e_off, F.e_off + ne), il(P.e_cnt, F.e_cnt), torch.cat([P.meta, F.meta]),
                       torch.cat([P.w_lo, F.w_lo]), torch.cat([P.w_hi, F.w_hi]), torch.cat([P.sigma, F.sigma]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--nw", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-n", type=int, default=0, help="ciphers per batch hashed on the host (0 = all, < 0 = none)")
    ap.add_argument("--lib", default=None, help="a variant library (make variant VFILE=k_commit) instead of the built one")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("exp_commit: needs a GPU")
    orc = Oracle.load()
    eng = Engine(device=0, canon_tag=CANON, lib=load_library(a.lib) if a.lib else None)
    host_n = None if a.host_n < 0 else a.host_n
    eng.set_H_digest(HD)
    eng.timing(True)
    ceiling = eng.alu_ceiling(4)
    res = {"alu_ceiling_4_wave_instr_per_s": ceiling, "sha_valu_per_block": SHA_VALU_PER_BLOCK}

    P = products(eng, a.n)
    res["a_products_with_sigma"] = measure(eng, orc, P, True, a.reps, host_n, ceiling)
    print(json.dumps(res["a_products_with_sigma"]), file=sys.stderr, flush=True)

    F = eng.gen_fresh(a.n, 14, 20)
    F.sigma = torch.empty((F.meta.shape[0], 128), dtype=torch.int64, device=eng.device)
    eng.fill_random(F.sigma, 15)
    M = interleave(P, F)
    res["ragged_mix_products_and_40_edge_ciphers"] = measure(eng, orc, M, True, a.reps, None, ceiling)
    del M, F, P
    torch.cuda.empty_cache()

    A, B = eng.gen_fresh(a.nw, 21, 20), eng.gen_fresh(a.nw, 22, 20)
    W = eng.ct_mul(A, B)
    res["b_products_weights_only"] = measure(eng, orc, W, False, a.reps, host_n, ceiling)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
