"""Timing of pvac_hip_batch_gather (GPU box) on four shapes,
  (a) an identity pick over a ct_mul output of 2^20 fresh pairs (capacity-padded, weights only),
  (b) one chunk of 64 depth-8 chain results (weights only),
  (c) 2^16 fresh-shaped ciphers with sigma,
  (d) shape (a) with a random permutation as the pick.
Per shape: device time of pvac_hip_batch_gather_exec from the engine's HIP-event timer "batch_gather" (median
and minimum of --reps launches after warm-up; the plan is made once), the time of plan + exec together
and of pvac_hip_batch_pack on the same source (both between two stream events around the calls: pack has
no timer of its own and plans inside the call), with the spread (max / min) of each, and the rate of a
device-to-device copy of the same bytes in the same process as the ceiling (copies above --copy-cap bytes are
measured at the cap). --variant names a second library (make variant VFILE=k_gather VNAME=wg
VFLAGS=-DPVAC_GATHER_LANES=256: a workgroup per tile instead of a wave) timed on the same arrays. Prints
one JSON line; --out also writes it to a file.
Usage: python tools/exp_gather.py [--reps 20] [--scale 1.0] [--variant lib/exp/libpvac_hip_wg.so] [--out profiles/gather/exp_gather.json]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pvac_hfhe_cppbyv_amd as pv  # noqa: E402
from pvac_hfhe_cppbyv_amd import DeviceBatch, Engine  # noqa: E402


def sha256(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def event_ms(call, reps, warm=2):
    """Milliseconds of `call` between two events on the current stream, per repetition."""
    ms = []
    for k in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        if k >= warm:
            ms.append(a.elapsed_time(b))
    return ms


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
            "spread": round(max(ms) / min(ms), 3)}


class Call:
    """One gather of `src` by `pick` (None: identity given as a pick list) into preallocated rows."""

    def __init__(self, eng, src, pick, dst):
        self.eng, self.dst = eng, dst
        self.structs = (pv.CtBatch * 1)(src.struct())
        self.pi = eng._index_tensor(pick)
        self.G = pv.Gather(C.cast(self.structs, C.c_void_p), 1, 0, len(pick), None, self.pi.data_ptr())
        self.tot = (C.c_uint64 * 2)()
        self.sd = dst.struct()

    def plan(self):
        self.eng._check(self.eng.lib.pvac_hip_batch_gather_plan(self.eng.ctx, C.byref(self.G), C.byref(self.sd), self.tot))

    def exec(self):
        self.eng._check(self.eng.lib.pvac_hip_batch_gather_exec(self.eng.ctx, C.byref(self.G), C.byref(self.sd),
                                                                self.dst.layers.shape[0], self.dst.meta.shape[0]))


def gather_times(eng, X, pick, dst, reps):
    call = Call(eng, X, pick, dst)
    call.plan()
    ms = []
    for k in range(2 + reps):
        t0, k0 = eng.timing_get("batch_gather")
        call.exec()
        t1, k1 = eng.timing_get("batch_gather")   # synchronises
        assert k1 == k0 + 1
        if k >= 2:
            ms.append(t1 - t0)

    def both():
        call.plan()
        call.exec()
    return stats(ms), stats(event_ms(both, reps))


def pack_times(eng, X, dst, reps):
    sx, sd = X.struct(), dst.struct()
    tot = (C.c_uint64 * 2)()
    return stats(event_ms(lambda: eng._check(eng.lib.pvac_hip_batch_pack(eng.ctx, C.byref(sx), C.byref(sd), tot)), reps))


def copy_ms(nbytes, device, reps):
    src = torch.empty(nbytes, dtype=torch.uint8, device=device)
    dst = torch.empty_like(src)
    return statistics.median(event_ms(lambda: dst.copy_(src), reps))


def same_rows(a, b, nl, ne, sigma):
    ok = torch.equal(a.layers[:nl], b.layers[:nl])
    for f in ("meta", "w_lo", "w_hi") + (("sigma",) if sigma else ()):
        ok = ok and torch.equal(getattr(a, f)[:ne], getattr(b, f)[:ne])
    return bool(ok)


def shape(engines, name, X, pick, reps, copy_cap, baseline=True):
    eng = engines[0][1]
    n = X.n
    sigma = X.sigma is not None
    nl, ne = int(X.l_cnt[:n].sum().item()), int(X.e_cnt[:n].sum().item())
    sw = X.sigma.shape[1] if sigma else 0
    nbytes = 40 * nl + (24 + 8 * sw) * ne
    dst = DeviceBatch.empty(n, nl, ne, eng.device)
    if sigma:
        dst.sigma = torch.empty((max(ne, 1), sw), dtype=torch.int64, device=eng.device)
    res = {"shape": name, "ciphers": n, "layers": nl, "edges": ne, "sigma_words": sw, "row_bytes": nbytes,
           "pick": "identity" if np.array_equal(pick, np.arange(n)) else "permutation"}
    for tag, e in engines:
        before = e.gather_path_counts()
        ex, both = gather_times(e, X, pick, dst, reps)
        after = e.gather_path_counts()
        res[tag] = {"exec_ms": ex, "plan_exec_ms": both, "exec_GB_per_s": round(nbytes / ex["median"] / 1e6, 1),
                    "tiles_per_exec": (after["tiles"] - before["tiles"]) // (2 * reps + 4),
                    "sigma_path": "wide" if after["wide"] > before["wide"] else "narrow"}
    if baseline:
        res["pack_ms"] = pack_times(eng, X, dst, reps)
        ref = DeviceBatch.empty(n, nl, ne, eng.device) if nbytes < (8 << 30) else None
        if ref is not None:   # the gather of the identity pick and the pack are the same rows
            if sigma:
                ref.sigma = torch.empty_like(dst.sigma)
            c = Call(eng, X, pick, ref)
            c.plan()
            c.exec()
            eng.sync()
            res["identity_equals_pack"] = same_rows(ref, dst, nl, ne, sigma)
        del ref
        res["gather_exec_over_pack"] = round(res["wave_per_tile"]["exec_ms"]["median"] / res["pack_ms"]["median"], 3)
        res["gather_plan_exec_over_pack"] = round(res["wave_per_tile"]["plan_exec_ms"]["median"] / res["pack_ms"]["median"], 3)
    cb = min(nbytes, copy_cap)
    c_ms = copy_ms(cb, eng.device, reps)
    res["copy"] = {"bytes": cb, "ms": round(c_ms, 4), "GB_per_s": round(cb / c_ms / 1e6, 1)}
    for tag, _ in engines:
        res[tag]["of_copy_rate"] = round(res[tag]["exec_GB_per_s"] / res["copy"]["GB_per_s"], 3)
    print(json.dumps(res), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the fresh shapes (a quick run)")
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--copy-cap", type=int, default=4 << 30)
    ap.add_argument("--variant", default=None, help="a second libpvac_hip build to time on the same arrays")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("exp_gather: needs a GPU")
    main_lib = os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "lib", "libpvac_hip.so")
    engines = [("wave_per_tile", Engine(device=0, canon_tag=0x5EED0006))]
    res = {"library_sha256": sha256(main_lib), "device": torch.cuda.get_device_name(0), "reps": a.reps, "shapes": []}
    if a.variant:
        engines.append(("workgroup_per_tile", Engine(device=0, canon_tag=0x5EED0006, lib=pv.load_library(a.variant))))
        res["variant_sha256"] = sha256(a.variant)
    for _, e in engines:
        e.timing(True)
    eng = engines[0][1]
    k = lambda x: max(int(x * a.scale), 64)
    rng = np.random.default_rng(7)

    n = k(1 << 20)
    X = eng.ct_mul(eng.gen_fresh(n, 31, 20), eng.gen_fresh(n, 32, 20), nonce_seed=33)
    res["shapes"].append(shape(engines, "a_mul_of_fresh_pairs", X, np.arange(n), a.reps, a.copy_cap))
    res["shapes"].append(shape(engines, "d_mul_of_fresh_pairs_permuted", X, rng.permutation(n), a.reps, a.copy_cap, baseline=False))
    del X
    x = eng.gen_fresh(a.chains, 12, 20)
    c = x
    for d in range(8):
        c = eng.ct_mul(c, x, nonce_seed=0x5EED0100 + d)
    res["shapes"].append(shape(engines, f"b_depth8_chain_chunk_{a.chains}", c, np.arange(a.chains), a.reps, a.copy_cap))
    del c
    n = k(1 << 16)
    X = eng.gen_fresh(n, 21, 20)
    X.sigma = torch.empty((X.meta.shape[0], 128), dtype=torch.int64, device=eng.device)
    eng.fill_random(X.sigma, 22)
    res["shapes"].append(shape(engines, "c_fresh_with_sigma", X, np.arange(n), a.reps, a.copy_cap))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
