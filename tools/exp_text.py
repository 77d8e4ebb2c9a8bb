"""Timing of the ragged encryption path (pvac_hip_enc_items) and enc_text on top of it (GPU box).
  1. 2^16 VALUE items at hint 0 through enc_items against pvac_hip_enc_value on the same values and
     draws, in alternating passes (A B A B ...), weights-only and with sigma; outputs compared.
  2. 4,096 messages of 150 bytes (45,056 ciphers) in one enc_text call, against the same cipher count
     issued as one uniform pvac_hip_enc_value_depth launch per hint (the only batched route without
     enc_items; it yields masked two-layer ciphers of u64 plaintexts, so it is a cost proxy, not a
     substitute), and the reference's own enc_text on one core (--ref: the JSON line printed by
     oracle/_ref/mint_text <golden ref> --time on the build machine, recorded with its host name).
  3. One 450-byte message: wall time of the call and the time of k_enc_items_weights; run again with
     --lib on the per-half variant (make variant VFILE=k_enc_items VNAME=perhalf
     VFLAGS=-DPVAC_ENC_ITEMS_PER_HALF) and --only one to compare the two layouts.
Device times are the engine's HIP-event timers (pvac_hip_timing_get: "enc_value", "enc_items" and
"enc_items_<launch>"), after one warm-up call at the timed shape; medians over --reps passes, with
min and max. Prints one JSON line stamped with the library's sha256; --out also writes it.
Usage: python tools/exp_text.py [--n 65536] [--msgs 4096] [--reps 5] [--only items|text|one] [--lib ...]
                                [--ref '{...}'] [--out profiles/text/exp_text.json]"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from helpers import fixture_secret, read_u64  # noqa: E402
from pvac_hfhe_cppbyv_amd import ENC_ITEM_VALUE, Engine, _LIB_PATH, load_library  # noqa: E402

LAUNCHES = ("enc_items_plan", "enc_items_prf", "enc_items_weights", "enc_items_sigma", "enc_items_finish")


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "passes": len(xs)}


def timed(eng, fn, names):
    eng.timing_reset()
    t0 = time.perf_counter()
    fn()
    eng.sync()
    wall = (time.perf_counter() - t0) * 1e3
    return wall, {n: eng.timing_get(n)[0] for n in names}


def items_vs_value(eng, n, reps, sigma):
    rng = np.random.default_rng(1)
    vals = rng.integers(0, 2**64, n, dtype=np.uint64)
    stride = eng.enc_caps(0)[2]
    rnd = torch.empty(n * stride, dtype=torch.int64, device=eng.device)
    eng.fill_random(rnd, 77)
    items = eng._items([(ENC_ITEM_VALUE, int(v), 0, i * stride, stride) for i, v in enumerate(vals)])
    caps = eng.enc_items_caps(items)[:2]
    keep = {}

    def a():
        keep["a"] = eng.enc_value(vals, rnd.view(n, stride), sigma=sigma)

    def b():
        keep["b"] = eng.enc_items(items, rnd, sigma=sigma, caps=caps)

    a(), b()   # warm-up at the timed shape
    same = bool((eng.sumdigest(keep["a"][0]) == eng.sumdigest(keep["b"][0])).all()) and not keep["a"][1].any() and \
        not keep["b"][1].any()
    ta, tb, per = [], [], {k: [] for k in LAUNCHES}
    for _ in range(reps):
        ta.append(timed(eng, a, ("enc_value",))[1]["enc_value"])
        t = timed(eng, b, ("enc_items",) + LAUNCHES)[1]
        tb.append(t["enc_items"])
        for k in LAUNCHES:
            per[k].append(t[k])
    keep.clear()
    torch.cuda.empty_cache()
    ma, mb = statistics.median(ta), statistics.median(tb)
    return {"n": n, "sigma": sigma, "outputs_equal": same, "enc_value": stats(ta), "enc_items": stats(tb),
            "enc_items_launches_median_ms": {k: round(statistics.median(v), 4) for k, v in per.items()},
            "enc_value_spread_ms": round(max(ta) - min(ta), 4), "enc_items_minus_enc_value_ms": round(mb - ma, 4),
            "values_per_s": {"enc_value": round(n / ma * 1e3, 1), "enc_items": round(n / mb * 1e3, 1)}}


def text_throughput(eng, n_msgs, reps, ref):
    rng = np.random.default_rng(2)
    msgs = [rng.integers(0, 256, 150, dtype=np.uint8).tobytes() for _ in range(n_msgs)]
    its, moff = eng.text_items(msgs)
    hint = eng.enc_items_caps([(k, v, h, 0, 0) for k, v, h in its])[2]
    offs = np.concatenate([[0], np.cumsum(hint)]).astype(np.int64)
    rnd = torch.empty(int(offs[-1]), dtype=torch.int64, device=eng.device)
    eng.fill_random(rnd, 78)
    items = eng._items([(k, v, h, int(offs[i]), int(hint[i])) for i, (k, v, h) in enumerate(its)])
    caps = eng.enc_items_caps(items)[:2]
    out = {"messages": n_msgs, "bytes_each": 150, "ciphers": len(its), "blocks": len(its) - n_msgs}
    for sigma in (False, True):
        keep = {}

        def run():
            keep["x"] = eng.enc_items(items, rnd, sigma=sigma, caps=caps)

        run()
        ok = not keep["x"][1].any()
        if not sigma:
            ok = ok and eng.dec_text(keep["x"][0], moff) == msgs
        dev, wall, per = [], [], {k: [] for k in LAUNCHES}
        for _ in range(reps):
            w, t = timed(eng, run, ("enc_items",) + LAUNCHES)
            dev.append(t["enc_items"])
            wall.append(w)
            for k in LAUNCHES:
                per[k].append(t[k])
        keep.clear()
        # the uniform route: the length ciphers at hint 0 and one launch of n_msgs values per block hint
        hints = [0] + sorted({h for _, _, h in its if h})
        vals = rng.integers(0, 2**64, n_msgs, dtype=np.uint64)
        rn = {h: torch.empty(n_msgs * eng.enc_caps(h)[2], dtype=torch.int64, device=eng.device) for h in hints}
        for h in hints:
            eng.fill_random(rn[h], 100 + h)

        def uniform():
            for h in hints:
                keep[h] = eng.enc_value(vals, rn[h].view(n_msgs, -1), sigma=sigma, depth=h)

        uniform()
        udev, uwall = [], []
        for _ in range(reps):
            w, t = timed(eng, uniform, ("enc_value",))
            udev.append(t["enc_value"])
            uwall.append(w)
        keep.clear()
        torch.cuda.empty_cache()
        md = statistics.median(dev)
        out["with_sigma" if sigma else "weights_only"] = {
            "ok": bool(ok), "device": stats(dev), "wall": stats(wall),
            "launches_median_ms": {k: round(statistics.median(v), 4) for k, v in per.items()},
            "blocks_per_s": round(out["blocks"] / md * 1e3, 1), "ciphers_per_s": round(len(its) / md * 1e3, 1),
            "bytes_per_s": round(n_msgs * 150 / md * 1e3, 1),
            "uniform_launches": {"launches": len(hints), "device": stats(udev), "wall": stats(uwall)}}
    if ref:
        out["reference_one_core"] = ref
    return out


def one_message(eng, reps):
    rng = np.random.default_rng(3)
    msg = rng.integers(0, 256, 450, dtype=np.uint8).tobytes()
    its, moff = eng.text_items([msg])
    hint = eng.enc_items_caps([(k, v, h, 0, 0) for k, v, h in its])[2]
    offs = np.concatenate([[0], np.cumsum(hint)]).astype(np.int64)
    rnd = torch.empty(int(offs[-1]), dtype=torch.int64, device=eng.device)
    eng.fill_random(rnd, 79)
    items = eng._items([(k, v, h, int(offs[i]), int(hint[i])) for i, (k, v, h) in enumerate(its)])
    caps = eng.enc_items_caps(items)[:2]
    keep = {}

    def run():
        keep["x"] = eng.enc_items(items, rnd, sigma=True, caps=caps)

    run()
    ok = not keep["x"][1].any() and eng.dec_text(keep["x"][0], moff) == [msg]
    digest = eng.commit_ct(keep["x"][0]).tobytes()
    wall, per = [], {k: [] for k in ("enc_items",) + LAUNCHES}
    for _ in range(reps):
        w, t = timed(eng, run, ("enc_items",) + LAUNCHES)
        wall.append(w)
        for k in per:
            per[k].append(t[k])
    return {"bytes": 450, "ciphers": len(its), "hints": [its[1][2], its[-1][2]], "ok": bool(ok),
            "commit_sha256_of_all": hashlib.sha256(digest).hexdigest(), "wall": stats(wall),
            "device_median_ms": {k: round(statistics.median(v), 4) for k, v in per.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--msgs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, choices=("items", "text", "one"))
    ap.add_argument("--lib", default=None, help="a variant library (make variant VFILE=k_enc_items) instead of the built one")
    ap.add_argument("--ref", default=None, help="JSON of the reference's one-core enc_text timing (mint_text --time)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("exp_text: needs a GPU")
    path = a.lib or _LIB_PATH
    with open(path, "rb") as f:
        res = {"library": os.path.relpath(path, ROOT), "library_sha256": hashlib.sha256(f.read()).hexdigest()}
    sk, man, em = fixture_secret()
    eng = Engine(device=0, canon_tag=man["canon_tag"], lib=load_library(a.lib) if a.lib else None)
    eng.gen_H()
    eng.set_secret(read_u64("sk_prf_k.u64"), read_u64("sk_lpn_s.u64"), em["lpn_n"], em["lpn_t"], em["lpn_tau_num"],
                   em["lpn_tau_den"])
    eng.set_powg(read_u64("powg_B.u64"))
    eng.timing(True)
    if a.only in (None, "items"):
        res["value_items_vs_enc_value"] = [items_vs_value(eng, a.n, a.reps, s) for s in (False, True)]
        print(json.dumps(res["value_items_vs_enc_value"]), file=sys.stderr, flush=True)
    if a.only in (None, "text"):
        res["text_throughput"] = text_throughput(eng, a.msgs, a.reps, json.loads(a.ref) if a.ref else None)
        print(json.dumps(res["text_throughput"]), file=sys.stderr, flush=True)
    if a.only in (None, "one"):
        res["one_message"] = one_message(eng, a.reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
