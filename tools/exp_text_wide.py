"""Timing of the wide encryption route (k_enc_wide.hip behind pvac_hip_enc_items) on the GPU box.
  a. 1,024 FP items at hint 124 (255 pre-merge edges, the largest plan both routes run): the narrow route
     against PVAC_ENC_WIDE_ALL in the same process, in alternating passes, per launch and in total,
     weights-only and with sigma; outputs compared. The totals again at hints 16 and 64.
  b. One 15,000-byte message (1,001 ciphers, hints up to 1001, 975,452 pre-merge edges), weights-only and
     with sigma: the total, every launch, the sub-batches, and the sigma launch's rate in edges per second.
  c. The finish stage's scaling: 256 FP items at hint 200 and at hint 1000 with sigma, enc_items_finish_wide
     per pre-merge edge, next to (b)'s; the stage is linear while the ratios stay within 4x of hint 200's.
  --ref: the JSON line printed by oracle/_ref/mint_text_wide <golden ref> --time on the build machine (the
     reference's own enc_text of 3,000 bytes on one core of a different machine: the order of magnitude only).
Device times are the engine's HIP-event timers (pvac_hip_timing_get), after one warm-up call at the timed
shape; medians over --reps passes. Prints one JSON line stamped with the library's sha256; --out also writes it.
Usage: python tools/exp_text_wide.py [--reps 5] [--only ab|text|finish] [--bytes 15000] [--ref '{...}']
                                     [--out profiles/text_wide/exp_text_wide.json]"""
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

import text_model as tm  # noqa: E402
from helpers import fixture_secret, read_u64  # noqa: E402
from pvac_hfhe_cppbyv_amd import ENC_ITEM_FP, Engine, _LIB_PATH  # noqa: E402

NARROW = ("enc_items_plan", "enc_items_prf", "enc_items_weights", "enc_items_sigma", "enc_items_finish")
WIDE = ("enc_items_plan_wide", "enc_items_prf", "enc_items_order_wide", "enc_items_weights_wide", "enc_items_sigma",
        "enc_items_finish_wide")
ALL = tuple(dict.fromkeys(NARROW + WIDE))


def npre(hint):
    z2, z3 = tm.plan_noise(hint)
    return 8 + 2 * z2 + 3 * z3


def timed(eng, fn, names):
    eng.timing_reset()
    t0 = time.perf_counter()
    fn()
    eng.sync()
    wall = (time.perf_counter() - t0) * 1e3
    return wall, {n: eng.timing_get(n)[0] for n in names}


def med(xs):
    return round(statistics.median(xs), 4)


def fp_items(eng, n, hint, seed):
    rng = np.random.default_rng(seed)
    vals = [int(rng.integers(0, 2**63, dtype=np.uint64)) for _ in range(n)]
    dh = int(eng.enc_items_caps([(ENC_ITEM_FP, 1, hint, 0, 0)])[2][0])
    rnd = torch.empty(n * dh, dtype=torch.int64, device=eng.device)
    eng.fill_random(rnd, seed)
    items = eng._items([(ENC_ITEM_FP, v, hint, i * dh, dh) for i, v in enumerate(vals)])
    return items, rnd, eng.enc_items_caps(items)[:2]


def narrow_vs_wide(eng, n, hint, reps, sigma, launches):
    items, rnd, caps = fp_items(eng, n, hint, 1000 + hint)
    keep = {}

    def a():
        keep["a"] = eng.enc_items(items, rnd, sigma=sigma, caps=caps)

    def b():
        keep["b"] = eng.enc_items(items, rnd, sigma=sigma, caps=caps, wide_all=True)

    a(), b()
    same = bool((eng.sumdigest(keep["a"][0]) == eng.sumdigest(keep["b"][0])).all()) and not keep["a"][1].any() and \
        not keep["b"][1].any()
    ta, tb = {k: [] for k in ("enc_items",) + NARROW}, {k: [] for k in ("enc_items",) + WIDE}
    for _ in range(reps):
        t = timed(eng, a, tuple(ta))[1]
        for k in ta:
            ta[k].append(t[k])
        t = timed(eng, b, tuple(tb))[1]
        for k in tb:
            tb[k].append(t[k])
    keep.clear()
    torch.cuda.empty_cache()
    out = {"items": n, "hint": hint, "pre_edges": n * npre(hint), "sigma": sigma, "outputs_equal": same,
           "narrow_ms": med(ta["enc_items"]), "wide_ms": med(tb["enc_items"])}
    if launches:
        out["narrow_launches_ms"] = {k: med(v) for k, v in ta.items() if k != "enc_items"}
        out["wide_launches_ms"] = {k: med(v) for k, v in tb.items() if k != "enc_items"}
    return out


def long_text(eng, nbytes, reps):
    rng = np.random.default_rng(5)
    msg = rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes()
    its, moff = eng.text_items([msg])
    hint = eng.enc_items_caps([(k, v, h, 0, 0) for k, v, h in its])[2]
    offs = np.concatenate([[0], np.cumsum(hint)]).astype(np.int64)
    rnd = torch.empty(int(offs[-1]), dtype=torch.int64, device=eng.device)
    eng.fill_random(rnd, 81)
    items = eng._items([(k, v, h, int(offs[i]), int(hint[i])) for i, (k, v, h) in enumerate(its)])
    ls, es = eng.enc_items_caps(items)[:2]
    out = {"bytes": nbytes, "ciphers": len(its), "last_hint": its[-1][2], "pre_edges": int(es), "draw_words": int(offs[-1])}
    for sigma in (False, True):
        keep = {}

        def run():
            keep["x"] = eng.enc_items(items, rnd, sigma=sigma, caps=(ls, es))

        c0 = eng.enc_path_counts()
        run()
        c1 = eng.enc_path_counts()
        ok = not keep["x"][1].any()
        if not sigma:
            ok = ok and eng.dec_text(keep["x"][0], moff) == [msg]
        per, wall = {k: [] for k in ("enc_items",) + ALL}, []
        for _ in range(reps):
            w, t = timed(eng, run, tuple(per))
            wall.append(w)
            for k in per:
                per[k].append(t[k])
        keep.clear()
        torch.cuda.empty_cache()
        r = {"ok": bool(ok), "sub_batches": c1[2] - c0[2], "narrow_items": c1[0] - c0[0], "wide_items": c1[1] - c0[1],
             "device_ms": med(per["enc_items"]), "wall_ms": med(wall), "launches_ms": {k: med(per[k]) for k in ALL},
             "finish_wide_ns_per_pre_edge": round(statistics.median(per["enc_items_finish_wide"]) * 1e6 / es, 3)}
        if sigma:
            r["sigma_edges_per_s"] = round(es / statistics.median(per["enc_items_sigma"]) * 1e3, 1)
        out["with_sigma" if sigma else "weights_only"] = r
    return out


def finish_scaling(eng, n, reps):
    out = {}
    for hint in (200, 1000):
        items, rnd, caps = fp_items(eng, n, hint, 2000 + hint)
        keep = {}

        def run():
            keep["x"] = eng.enc_items(items, rnd, sigma=True, caps=caps)

        run()
        ok = not keep["x"][1].any()
        per = {k: [] for k in WIDE}
        for _ in range(reps):
            t = timed(eng, run, WIDE)[1]
            for k in per:
                per[k].append(t[k])
        keep.clear()
        torch.cuda.empty_cache()
        pe = n * npre(hint)
        out[f"hint{hint}"] = {"items": n, "pre_edges": pe, "ok": bool(ok), "launches_ms": {k: med(v) for k, v in per.items()},
                              "finish_wide_ns_per_pre_edge": round(statistics.median(per["enc_items_finish_wide"]) * 1e6 / pe, 3)}
    out["hint1000_over_hint200"] = round(out["hint1000"]["finish_wide_ns_per_pre_edge"] / out["hint200"]["finish_wide_ns_per_pre_edge"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--bytes", type=int, default=15000)
    ap.add_argument("--only", default=None, choices=("ab", "text", "finish"))
    ap.add_argument("--ref", default=None, help="JSON of the reference's one-core enc_text timing (mint_text_wide --time)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("exp_text_wide: needs a GPU")
    with open(_LIB_PATH, "rb") as f:
        res = {"library": os.path.relpath(_LIB_PATH, ROOT), "library_sha256": hashlib.sha256(f.read()).hexdigest()}
    sk, man, em = fixture_secret()
    eng = Engine(device=0, canon_tag=man["canon_tag"], enc_plan_limit=1 << 16)
    eng.gen_H()
    eng.set_secret(read_u64("sk_prf_k.u64"), read_u64("sk_lpn_s.u64"), em["lpn_n"], em["lpn_t"], em["lpn_tau_num"],
                   em["lpn_tau_den"])
    eng.set_powg(read_u64("powg_B.u64"))
    eng.timing(True)
    if a.only in (None, "ab"):
        res["narrow_vs_wide_hint124"] = [narrow_vs_wide(eng, a.n, 124, a.reps, s, True) for s in (False, True)]
        res["narrow_vs_wide_sweep"] = [narrow_vs_wide(eng, a.n, h, a.reps, s, False) for h in (16, 64) for s in (False, True)]
        print(json.dumps(res["narrow_vs_wide_hint124"]), file=sys.stderr, flush=True)
    if a.only in (None, "finish"):
        res["finish_scaling"] = finish_scaling(eng, 256, a.reps)
        print(json.dumps(res["finish_scaling"]), file=sys.stderr, flush=True)
    if a.only in (None, "text"):
        res["long_text"] = long_text(eng, a.bytes, a.reps)
        f200 = res.get("finish_scaling", {}).get("hint200", {}).get("finish_wide_ns_per_pre_edge")
        if f200:
            res["long_text"]["finish_per_edge_over_hint200"] = round(
                res["long_text"]["with_sigma"]["finish_wide_ns_per_pre_edge"] / f200, 3)
    if a.ref:
        res["reference_one_core_other_machine"] = json.loads(a.ref)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
