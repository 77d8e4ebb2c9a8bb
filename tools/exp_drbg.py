"""Measurements of the device CSPRNG (GPU box): pvac_hip_drbg_fill (k_aes256_ctr) against the splitmix
test stream pvac_hip_fill_random, and what secure nonces cost the headline ct_mul step.
  fill:    drbg_fill and fill_random at 2^23 words (the nonce array of 2^20 fresh pairs) and 2^27 words,
           alternated in one process, warmed, timed by device events over windows of at least --window
           seconds each; GB/s of words written. The kernel's own time comes from the engine's HIP-event
           timer "aes256_ctr" (and, with --stats-csv, from a rocprofv3 --kernel-trace --stats run of
           `--only kernel`, which launches nothing but fills). Its floor is its table reads: 224
           ds_read_b32 per block, 2 LDS cycles per wave instruction, so a CU finishes 64 blocks (1 KiB)
           per 448 cycles: floor = CUs x clock x 1024 / 448 bytes/s, the clock from pvac_hip_issue_probe.
  step:    the ct_mul step (plan + exec, pvac_hip_ct_mul) on --pairs fresh pairs, three ways, alternated:
           (1) nonces fixed, as bench.py runs it (also on --parent, a library built from the parent commit),
           (2) nonces refilled by splitmix before every step, (3) refilled by the generator every step.
           Done when (3) is within 1.10 x of (1).
  adapter: ct_mul_batch on --adapter-pairs host pairs, weights only, with os_random_u64 and with device_random
           on the same inputs (tests/cpp/build/test_drbg --time, a process of its own, best of three
           alternated rounds each). No bar: the host conversion dominates both.
Prints one JSON line; --out also writes it.
Usage: python tools/exp_drbg.py [--window 1.0] [--pairs 1048576] [--parent lib/exp/libpvac_hip_parent.so]
                                [--only fill|step|kernel|adapter] [--adapter-pairs 32768] [--variant TAG=LIB] [--stats-csv FILE] [--out profiles/drbg/exp_drbg.json]"""
import argparse
import csv
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import pvac_hfhe_cppbyv_amd as pv  # noqa: E402
from pvac_hfhe_cppbyv_amd import Engine  # noqa: E402

LDS_READS_PER_BLOCK = 224      # 13 rounds x 16 + the last round's 16
LDS_CYCLES_PER_WAVE_READ = 2   # ds_read_b32: two groups of 32 lanes, one LDS cycle each


def sha256(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def load_older(path):
    """A libpvac_hip.so of an earlier commit, bound like load_library() minus the entries it lacks."""
    cur, old = pv.load_library(), C.CDLL(path)
    for name, fn in vars(cur).items():
        if name.startswith("pvac_") and hasattr(old, name):
            f = getattr(old, name)
            f.argtypes, f.restype = fn.argtypes, fn.restype
    return old


def window_ms(call, seconds, warm=3):
    """Per-call milliseconds of `call` over one window of at least `seconds`, between two device events."""
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    reps, total = 8, 0.0
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call()
        b.record()
        b.synchronize()
        total = a.elapsed_time(b)
        if total >= 1000.0 * seconds:
            return total / reps, reps
        reps = max(reps * 2, int(reps * 1200.0 * seconds / max(total, 1e-3)))


def alternate(calls, seconds, rounds=3):
    """{name: per-call ms of every round}, the calls alternated round by round."""
    out = {k: [] for k in calls}
    for _ in range(rounds):
        for k, f in calls.items():
            out[k].append(window_ms(f, seconds)[0])
    return out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5),
            "spread": round(max(ms) / min(ms), 3)}


def fill_rates(eng, seconds, res, variants=()):
    clock = eng.issue_probe(0, 8)[1]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    floor = cus * clock * 64 * 16 / (LDS_READS_PER_BLOCK * LDS_CYCLES_PER_WAVE_READ)
    res["clock_hz"] = clock
    res["compute_units"] = cus
    res["keystream_floor_GB_per_s"] = round(floor / 1e9, 1)
    res["bound"] = ("LDS issue: 224 ds_read_b32 per block at 2 LDS cycles per wave instruction (128 B/clk/CU); "
                    "floor = CUs x clock x 1024 B / 448 cycles")
    res["fill"] = []
    for lg in (23, 27):
        n = 1 << lg
        t = torch.empty(n, dtype=torch.int64, device=eng.device)
        calls = {"drbg_fill": lambda: eng.drbg_fill(t), "fill_random": lambda: eng.fill_random(t, 0x5EED)}
        for tag, v in variants:   # another build of k_drbg.hip on the same array; its keystream must be the same
            key, ctr = bytes(range(32)), bytes(range(200, 216))
            want = eng.aes256_ctr(key, ctr, 1 << 20).clone()
            assert torch.equal(v.aes256_ctr(key, ctr, 1 << 20), want), tag
            calls["drbg_fill_" + tag] = (lambda e: lambda: e.drbg_fill(t))(v)
        ms = alternate(calls, seconds)
        eng.timing_reset()
        eng.timing(True)
        for _ in range(20):
            eng.drbg_fill(t)
        k_ms, k_n = eng.timing_get("aes256_ctr")
        eng.timing(False)
        row = {"words": n, "bytes": 8 * n}
        for k, v in ms.items():
            row[k] = summary(v)
            row[k]["GB_per_s"] = round(8 * n / statistics.median(v) / 1e6, 1)
        row["kernel_ms_event_timer"] = round(k_ms / k_n, 5)
        row["kernel_GB_per_s"] = round(8 * n / (k_ms / k_n) / 1e6, 1)
        row["kernel_share_of_floor"] = round(8 * n / (k_ms / k_n) / 1e6 / (floor / 1e9), 3)
        res["fill"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del t


def step_cost(eng, parent, pairs, seconds, res):
    def setup(e):
        A, B = e.gen_fresh(pairs, 0x5EED0003, 20), e.gen_fresh(pairs, 0x5EED0004, 20)
        Cb, plan = e.ct_mul_plan(A, B)
        nonces = e.fill_nonces(A, B, Cb, plan, 0x5EED0005)
        out = e.ct_mul(A, B, nonces=nonces, C_=Cb, plan=plan)
        return e.ct_mul_step(A, B, out, nonces), nonces

    run, nonces = setup(eng)

    def splitmix():
        eng.fill_random(nonces, 0x5EED0006)
        run()

    def secure():
        eng.drbg_fill(nonces)
        run()

    calls = {"fixed": run, "splitmix_every_step": splitmix, "drbg_every_step": secure}
    if parent is not None:
        calls["fixed_parent_library"] = setup(parent)[0]
    ms = alternate(calls, seconds)
    row = {"pairs": pairs, "nonce_words": int(nonces.numel())}
    for k, v in ms.items():
        row[k] = summary(v)
        row[k]["M_ct_mul_per_s"] = round(pairs / statistics.median(v) / 1e3, 2)
    base = statistics.median(ms["fixed_parent_library" if parent is not None else "fixed"])
    row["baseline"] = "fixed_parent_library" if parent is not None else "fixed"
    row["drbg_over_fixed"] = round(statistics.median(ms["drbg_every_step"]) / base, 4)
    row["splitmix_over_fixed"] = round(statistics.median(ms["splitmix_every_step"]) / base, 4)
    row["within_1_10"] = row["drbg_over_fixed"] <= 1.10
    res["step"] = row
    print(json.dumps(row), file=sys.stderr, flush=True)


def kernel_stats(path):
    """The aes256_ctr row of a rocprofv3 --stats kernel CSV: calls and average nanoseconds."""
    with open(path) as f:
        for r in csv.DictReader(f):
            if "k_aes256_ctr" in r.get("Name", ""):
                return {"calls": int(r["Calls"]), "average_ns": float(r["AverageNs"])}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--parent", default=None, help="a libpvac_hip.so built from the parent commit (the step's baseline)")
    ap.add_argument("--only", choices=["fill", "step", "kernel", "adapter"], default=None)
    ap.add_argument("--adapter-pairs", type=int, default=1 << 15)
    ap.add_argument("--variant", action="append", default=[], metavar="TAG=LIB",
                    help="another build of the library (make variant VFILE=k_drbg ...) whose drbg_fill is timed beside the main one")
    ap.add_argument("--stats-csv", default=None, help="kernel stats of a rocprofv3 run of --only kernel")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("exp_drbg: needs a GPU")
    eng = Engine(device=0, canon_tag=0x5EED0003)
    if a.only == "kernel":   # under the profiler: fills of 2^27 words and nothing else
        t = torch.empty(1 << 27, dtype=torch.int64, device=eng.device)
        for _ in range(50):
            eng.drbg_fill(t)
        eng.sync()
        return
    lib = os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "lib", "libpvac_hip.so")
    res = {"library_sha256": sha256(lib), "device": torch.cuda.get_device_name(0), "window_s": a.window,
           "drbg_tile": eng.drbg_tile()}
    if a.only in (None, "fill"):
        variants = []
        for spec in a.variant:
            tag, path = spec.split("=", 1)
            variants.append((tag, Engine(device=0, canon_tag=0x5EED0003, lib=load_older(path))))
            res.setdefault("variants", {})[tag] = sha256(path)
        fill_rates(eng, a.window, res, variants)
    if a.only in (None, "step"):
        parent = None
        if a.parent:
            parent = Engine(device=0, canon_tag=0x5EED0003, lib=load_older(a.parent))
            res["parent_sha256"] = sha256(a.parent)
        step_cost(eng, parent, a.pairs, a.window, res)
    if a.only in (None, "adapter"):
        exe = os.path.join(ROOT, "tests", "cpp", "build", "test_drbg")
        r = subprocess.run([exe, "--time", str(a.adapter_pairs)], capture_output=True, text=True, timeout=600)
        if r.returncode:
            sys.exit("exp_drbg: test_drbg --time failed: " + r.stderr[-2000:])
        res["adapter"] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(res["adapter"]), file=sys.stderr, flush=True)
    if a.stats_csv:
        ks = kernel_stats(a.stats_csv)
        res["kernel_trace"] = ks
        if ks and "keystream_floor_GB_per_s" in res:
            gbs = 8 * (1 << 27) / ks["average_ns"]
            res["kernel_trace"]["GB_per_s"] = round(gbs, 1)
            res["kernel_trace"]["share_of_floor"] = round(gbs / res["keystream_floor_GB_per_s"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
